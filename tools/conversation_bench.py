"""The second question about one image: turn 2 on the prefix turn 1 returned against turn 2 as a whole new request, and the round time with
return_prefix off and on, synthetic weights, a bench prompt.   GPU only.

    python tools/conversation_bench.py llava7b|qwen7b [reps] [out_dir] [new_tokens]   -> <out_dir = profiles>/conversation_<model>.txt (and stdout)

One process, an otherwise idle GPU, a side stream (the rounds replay their captured graphs, as in bench.py).  Turn 1 is a bench request
that generates `new_tokens` (64) tokens with return_prefix=True; turn 2 is turn 1's returned ids followed by QUESTION_ROWS new text ids.

Time to first tree = SpecModel._start_request: everything up to and including the draft prefill and the first tree.  After warm-up the legs
alternate  a, b, a'  for `reps` repetitions:
  (a) turn 2 as a whole new request: the vision front-end on the request's pixels (when HF's vision modules can be built here — the header
      line says whether they were; otherwise the request starts from projected features and the front-end is NOT in the leg), the merge, the
      target prefill of every row, first token, draft prefill;
  (b) turn 2 on the returned prefix: one K/V copy launch, the target prefill of the new rows only, first token, draft prefill.
Leg (a) runs twice per repetition: its two interleaved series a / a' give its own spread, and a difference counts only where it exceeds
that spread ("within spread" otherwise).  Stream time between two events around a leg (ms), medians and ranges.

Round time: a leg = start the request (untimed), two warm rounds (the graph of the leg's key is captured or found in the cache there), then
ROUNDS timed rounds between two events; legs alternate  off, on, off', on'.  Both settings generate the same tokens; on adds one 16-byte
store per lane to the hidden blocks of the post_accept launch (at most TREE_RET_W rows of D bf16 per round).  The harvest itself
(_result_prefix: the K/V copy of every row, the log rows, the embeddings of the generated ids) is timed on its own line: it is paid once per
request, outside the rounds."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from vispec_amd.evaluation.bench_vision import InLoopFrontEnd, build_front_end  # noqa: E402
from vispec_amd.model.spec_model_ours import _result_prefix  # noqa: E402

ROUNDS = 24
BUDGET = 4096  # never reached inside a leg
QUESTION_ROWS = 32


def main():
    model = sys.argv[1] if len(sys.argv) > 1 else "llava7b"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    new_tokens = int(sys.argv[4]) if len(sys.argv) > 4 else 64
    bench.MODEL = model
    dev = torch.device("cuda:0")
    lanes, tcfg, _ = bench.build_models(dev, 0, 0, 1, 1, 1)
    lead = lanes[0]
    try:
        n_img = {"qwen7b": 1024, "qwen7b-hires": 1564, "qwen7b-fp8": 1564, "qwen7b-fp8a8": 1564}.get(model, bench.N_IMG)
        bench.FRONT_END = InLoopFrontEnd(*build_front_end(model, tcfg, dev, n_img))
        lead.base_model.vision = bench.FRONT_END
        vision_note = "IN leg (a): " + bench.FRONT_END.what
    except Exception as e:
        bench.FRONT_END = None
        vision_note = f"NOT in leg (a) (HF vision modules could not be built: {type(e).__name__}: {e})"[:300]
    ids, kw = bench.make_request(tcfg, 70, dev)
    side = torch.cuda.Stream()
    med = statistics.median
    f = lambda v: f"{med(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]"

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(side)
        fn()
        e1.record(side)
        side.synchronize()
        return e0.elapsed_time(e1)

    with torch.cuda.stream(side):
        out1, pfx = lead.specgenerate(ids, max_new_tokens=new_tokens, return_prefix=True, **kw)
        if pfx is None:
            raise SystemExit("turn 1 generated an image / video placeholder id: no prefix was returned, nothing to measure")
        g = torch.Generator().manual_seed(7)
        ids2 = torch.cat([out1, torch.randint(3, 30000, (1, QUESTION_ROWS), generator=g).to(dev)], dim=1)
        Ln, P, L2 = int(ids.shape[1]), pfx.rows, int(ids2.shape[1])
        lines = [f"# tools/conversation_bench.py {model} reps={reps}: turn 1 = {Ln} prompt rows + {P - Ln} generated, turn 2 = {L2} rows of which "
                 f"{L2 - P} are new, prefix {pfx.nbytes / 1e6:.1f} MB ({pfx.store.numel() * 2 / P / 1e6:.3f} MB of K/V per row), "
                 f"hidden-row log {lead.engine.kv_max_pos * tcfg.hidden_size * 2 / 1e6:.1f} MB, {torch.cuda.get_device_name(0)}",
                 f"# vision front-end {vision_note}",
                 "# time to first tree of turn 2, ms (stream time), median [min .. max]; a / a' = the two interleaved series of the whole new request",
                 "# a: whole new request | a' | b: on the returned prefix | a - b | spread of a | verdict"]
        leg_a = lambda: lead._start_request(ids2, None, dict(kw), max_new_tokens=BUDGET)
        leg_b = lambda: lead._start_request(ids2, None, {}, max_new_tokens=BUDGET, prefix=pfx)
        for _ in range(2):
            leg_a(), leg_b()
        a, a2, b = [], [], []
        for _ in range(reps):
            a.append(timed(leg_a))
            b.append(timed(leg_b))
            a2.append(timed(leg_a))
        a_all = a + a2
        spread = max(abs(med(a) - med(a2)), max(a_all) - min(a_all))
        d = med(a_all) - med(b)
        lines.append(f"{f(a)} | {f(a2)} | {f(b)} | {d:+8.3f} ms ({100 * d / med(a_all):+5.1f} %) | {spread:.3f} ms | "
                     f"{'gain' if d > spread else ('loss' if -d > spread else 'within spread')}")
        print(lines[-1], flush=True)

        # the rounds, with the log off and on
        def leg(on):
            lead._start_request(ids, None, dict(kw), max_new_tokens=BUDGET, **({"return_prefix": True} if on else {}))
            step = lambda: (lead.engine.verify_accept(-1), lead.engine.draft_round())
            for _ in range(2):
                step()
            return timed(lambda: [step() for _ in range(ROUNDS)]) / ROUNDS

        caps = []
        for on in (False, True):  # warm-up: both graphs captured
            c0 = lead.engine.graph_stats()["captures"]
            leg(on)
            caps.append(lead.engine.graph_stats()["captures"] - c0)
        off, off2, on_ = [], [], []
        for _ in range(reps):
            off.append(leg(False))
            on_.append(leg(True))
            off2.append(leg(False))
            on_.append(leg(True))
        off_all = off + off2
        spread = max(abs(med(off) - med(off2)), max(off_all) - min(off_all))
        d = med(on_) - med(off_all)
        lines += [f"# ms per ROUND (stream time of {ROUNDS} rounds / {ROUNDS}), median [min .. max]; off / off' = the two interleaved series without the log",
                  "# off | off' | on | on - off | spread of off | verdict | round-graph captures of the first leg (off, on)",
                  f"{f(off)} | {f(off2)} | {f(on_)} | {d:+7.3f} ms ({100 * d / med(off_all):+5.2f} %) | {spread:.3f} ms | "
                  f"{'on costs more' if d > spread else ('on is faster' if -d > spread else 'within spread')} | {caps[0]}, {caps[1]}"]
        print(lines[-1], flush=True)

        # the harvest: the last on-leg left a live request with the log on
        st = lead.engine.state()
        toks = torch.from_numpy(lead.engine.tokens(st["n_ctx"]).astype("int64")).to(dev)[None]
        for _ in range(2):
            _result_prefix(lead, toks)
        h = [timed(lambda: _result_prefix(lead, toks)) for _ in range(reps)]
        lines += [f"# harvest of a request of {st['n_ctx']} rows (K/V copy + log rows + embeddings), ms, once per request", f(h)]
        print(lines[-1], flush=True)
    out_dir = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"conversation_{model}.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
