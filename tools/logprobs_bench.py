"""Round time with return_logprobs off and on: a single request and a cohort of eight, synthetic weights, a bench prompt.   GPU only.

    python tools/logprobs_bench.py llava7b|qwen7b [reps] [out_dir]      -> <out_dir = profiles>/logprobs_<model>.txt (and stdout)

One process, an otherwise idle GPU, a side stream (the rounds replay their captured graphs, as in bench.py).  A leg = start the
request(s) (untimed: prefill, first token, draft prefill), two warm rounds (the graph of the leg's key is captured or found in the cache
there), then ROUNDS timed rounds between two events.  Both settings generate the same tokens (the flag changes no arithmetic of the
round), so the legs do the same work but for token_logprob_kernel: TREE_RET_W workgroups per request behind the accept kernel, of which
accept_len + 1 read one logits row each.  Legs alternate  off, on, off', on'  for `reps` repetitions: the two interleaved off series give
the spread of off itself, and on-vs-off counts only where it exceeds that spread ("within spread" otherwise).  Off is the path without
the feature: target_logprobs() in csrc/vispec_hip.hip returns before its first launch when no request of the round has the flag, and the
graph-cache key separates the two settings (`captures` below: its own round graphs per setting, never a replay of the other's)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

ROUNDS = 24
BUDGET = 4096  # never reached inside a leg


def main():
    model = sys.argv[1] if len(sys.argv) > 1 else "llava7b"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    bench.MODEL = model
    dev = torch.device("cuda:0")
    lanes, tcfg, _ = bench.build_models(dev, 0, 0, 1, 1, 8)
    models = lanes[0]
    lead = models[0]
    reqs = [bench.make_request(tcfg, 70 + t, dev) for t in range(8)]
    side = torch.cuda.Stream()
    med = statistics.median
    f = lambda v: f"{med(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]"
    lines = [f"# tools/logprobs_bench.py {model} reps={reps}: {ROUNDS} rounds per leg, prompt rows {int(reqs[0][0].shape[1])}, V = {tcfg.vocab_size}, "
             f"{torch.cuda.get_device_name(0)}",
             "# ms per ROUND (stream time of a leg / rounds), median [min .. max]; off / off' = the two interleaved series without the feature",
             "# requests | off | off' | on | on - off | spread of off | verdict | round-graph captures of the first leg (off, on)"]

    def leg(n, on):
        ms = models[:n]
        members = [m.engine for m in ms[1:]]
        for m, (ids, kw) in zip(ms, reqs):
            m._start_request(ids, None, dict(kw), max_new_tokens=BUDGET, **({"return_logprobs": True} if on else {}))
        step = (lambda: lead.engine.cohort_round(members, -1)) if n > 1 else (lambda: (lead.engine.verify_accept(-1), lead.engine.draft_round()))
        for _ in range(2):
            step()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        for _ in range(ROUNDS):
            step()
        e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1) / ROUNDS

    with torch.cuda.stream(side):
        for n in (1, 8):
            caps = []
            for on in (False, True):  # warm-up: both graphs captured
                c0 = lead.engine.graph_stats()["captures"]
                leg(n, on)
                caps.append(lead.engine.graph_stats()["captures"] - c0)
            off, off2, on_ = [], [], []
            for _ in range(reps):
                off.append(leg(n, False))
                on_.append(leg(n, True))
                off2.append(leg(n, False))
                on_.append(leg(n, True))
            off_all = off + off2
            spread = max(abs(med(off) - med(off2)), max(off_all) - min(off_all))
            d = med(on_) - med(off_all)
            verdict = "on costs more" if d > spread else ("on is faster" if -d > spread else "within spread")
            lines.append(f"{n} | {f(off)} | {f(off2)} | {f(on_)} | {d:+7.3f} ms ({100 * d / med(off_all):+5.2f} %) | {spread:.3f} ms | {verdict} | {caps[0]}, {caps[1]}")
            print(lines[-1], flush=True)
            lp = lead.engine.logprobs(lead.engine.state()["n_ctx"])[lead._prompt_len:]
            lines.append(f"#   request 0 after the last on-leg: {len(lp)} values, min {lp.min():.3f}, max {lp.max():.3g}")
    out_dir = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"logprobs_{model}.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[:3]))


if __name__ == "__main__":
    main()
