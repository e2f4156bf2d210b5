"""Round time with return_logprobs off and on, and with top_logprobs = 5 and 20 on top of it: a single request and a cohort of eight,
synthetic weights, a bench prompt.   GPU only.

    python tools/logprobs_bench.py llava7b|qwen7b [reps] [out_dir]      -> <out_dir = profiles>/top_logprobs_<model>.txt (and stdout)

One process, an otherwise idle GPU, a side stream (the rounds replay their captured graphs, as in bench.py).  A leg = start the
request(s) (untimed: prefill, first token, draft prefill), two warm rounds (the graph of the leg's key is captured or found in the cache
there), then ROUNDS timed rounds between two events.  All settings generate the same tokens (the options change no arithmetic of the
round), so the legs do the same work but for the kernel behind the accept kernel: none (off), token_logprob_kernel (logprobs: TREE_RET_W
workgroups per request, of which accept_len + 1 read one logits row each) or token_top_logprob_kernel in its place (top 5 / top 20: the
same workgroups read their row about four more times and select).  Legs alternate  off, logprobs, top 5, top 20, off', logprobs, top 5,
top 20  for `reps` repetitions: the two interleaved off series give the spread of off itself, and a leg-vs-off difference counts only
where it exceeds that spread ("within spread" otherwise).  Off is the path without the feature: target_logprobs() in csrc/vispec_hip.hip
returns before its first launch when no request of the round has the flag, and the graph-cache key separates the settings (`captures`
below: its own round graphs per setting, never a replay of another's)."""
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
             "# ms per ROUND (stream time of a leg / rounds), median [min .. max]; off / off' = the two interleaved series without the feature;",
             "# every other leg: median [min .. max] | leg - off (% of off) | verdict against the spread of off",
             "# requests | off | off' | spread of off | logprobs | logprobs + top 5 | logprobs + top 20 | round-graph captures of the first legs"]
    LEGS = [("off", {}), ("logprobs", {"return_logprobs": True}), ("top5", {"return_logprobs": True, "top_logprobs": 5}),
            ("top20", {"return_logprobs": True, "top_logprobs": 20})]

    def leg(n, kw):
        ms = models[:n]
        members = [m.engine for m in ms[1:]]
        for m, (ids, req_kw) in zip(ms, reqs):
            m._start_request(ids, None, dict(req_kw), max_new_tokens=BUDGET, **kw)
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
            for _, kw in LEGS:  # warm-up: every setting's graphs captured
                c0 = lead.engine.graph_stats()["captures"]
                leg(n, kw)
                caps.append(lead.engine.graph_stats()["captures"] - c0)
            off, off2, on_ = [], [], {name: [] for name, _ in LEGS[1:]}
            for _ in range(reps):
                for series in (off, off2):
                    series.append(leg(n, LEGS[0][1]))
                    for name, kw in LEGS[1:]:
                        on_[name].append(leg(n, kw))
            off_all = off + off2
            spread = max(abs(med(off) - med(off2)), max(off_all) - min(off_all))
            cells = []
            for name, _ in LEGS[1:]:
                d = med(on_[name]) - med(off_all)
                verdict = "costs more" if d > spread else ("is faster" if -d > spread else "within spread")
                cells.append(f"{f(on_[name])} | {d:+7.3f} ms ({100 * d / med(off_all):+5.2f} %) | {verdict}")
            lines.append(f"{n} | {f(off)} | {f(off2)} | {spread:.3f} ms | " + " | ".join(cells) + " | " + ", ".join(str(c) for c in caps))
            print(lines[-1], flush=True)
            n_ctx = lead.engine.state()["n_ctx"]
            lp = lead.engine.logprobs(n_ctx)[lead._prompt_len:]
            ti, tv = (x[lead._prompt_len:] for x in lead.engine.top_logprobs(n_ctx))
            lines.append(f"#   request 0 after the last top-20 leg: {len(lp)} values, min {lp.min():.3f}, max {lp.max():.3g}; top-1 value min {tv[:, 0].min():.3f}, "
                         f"top-20 value min {tv[:, 19].min():.3f}, chosen token listed at {int((ti == lead.engine.tokens(n_ctx)[lead._prompt_len:, None]).any(1).sum())} positions")
    out_dir = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"top_logprobs_{model}.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines[:5]))


if __name__ == "__main__":
    main()
