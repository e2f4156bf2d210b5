"""TargetLM.prefill_batch on k prompts against k sequential TargetLM.prefill calls, at a bench prompt shape.   GPU only.

    python tools/prefill_batch_bench.py llava7b|qwen7b [reps] [out_dir]      -> <out_dir = profiles>/prefill_batch_<model>.txt (and stdout)

One process, an otherwise idle GPU.  For k in {1, 2, 3, 4, 8}: after warm-up the legs alternate  seq, batch, seq', batch, ...  for `reps`
repetitions; the sequential leg therefore runs twice as often, and the two interleaved series seq / seq' give its own spread (the baseline
is the parent's behaviour measured in the same run; a gain counts only where it exceeds that spread).  Times are stream time between two
events around a leg (ms), medians over the repetitions.  The per-kernel split (library GEMMs / attention / element-wise) comes from one
extra profiled repetition of each leg (torch.profiler device times)."""
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

KS = (1, 2, 3, 4, 8)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def kernel_split(fn):
    """device ms of one call by class: (library GEMMs, attention, element-wise)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    gemm = attn = elem = 0.0
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        t = (t if t is not None else getattr(ev, "cuda_time_total", 0.0)) / 1e3
        if not t:
            continue
        if "prefill_attn" in ev.key:
            attn += t
        elif re.search(r"Cijk|gemm|Gemm|GEMM|_mm|MT\d+x\d+", ev.key):
            gemm += t
        else:
            elem += t
    return gemm, attn, elem


def main():
    model = sys.argv[1] if len(sys.argv) > 1 else "llava7b"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    bench.MODEL = model
    dev = torch.device("cuda:0")
    lanes, tcfg, _ = bench.build_models(dev, 0, 0, 1, 1, 8)
    models = lanes[0]
    base = models[0].base_model
    preps = []
    for i, m in enumerate(models):  # the first stage of a request start: embeddings (+ M-RoPE positions) of a bench request
        ids, kw = bench.make_request(tcfg, 70 + i, dev)
        preps.append(m._start_prepare(ids, None, dict(kw)))
    lens = [int(pr.emb.shape[0]) for pr in preps]
    lines = [f"# tools/prefill_batch_bench.py {model} reps={reps}: prompt rows {lens[0]} per request, {torch.cuda.get_device_name(0)}, "
             f"prefill GEMMs: {__import__('vispec_amd.model.target', fromlist=['x']).prefill_gemm_selection()}",
             "# ms per leg (stream time), median [min .. max] over the repetitions; seq / seq' = the two interleaved series of the sequential leg",
             "# k | seq | seq' | batch | batch vs seq median | spread of seq (max |seq - seq'| of medians, and range) | verdict"]
    split_lines = ["# per-kernel device ms of ONE repetition (torch.profiler): library GEMMs / attention / element-wise (incl. rotary, norms, SwiGLU, copies)"]
    for k in KS:
        ms, engines = models[:k], [m.engine for m in models[:k]]
        seq = lambda: [m.base_model.prefill(pr.emb, position_ids=pr.position_ids) for m, pr in zip(ms, preps)]
        bat = lambda: base.prefill_batch(engines, [pr.emb for pr in preps[:k]], [pr.position_ids for pr in preps[:k]])
        for _ in range(2):
            seq()
            bat()
        torch.cuda.synchronize()
        a, a2, b = [], [], []
        for _ in range(reps):
            a.append(timed(seq))
            b.append(timed(bat))
            a2.append(timed(seq))
            b.append(timed(bat))
        med = statistics.median
        seq_all = a + a2
        spread = max(abs(med(a) - med(a2)), 0.0)
        rng_ = max(seq_all) - min(seq_all)
        gain = med(seq_all) - med(b)
        verdict = "gain" if gain > max(spread, rng_) else ("loss" if -gain > max(spread, rng_) else "within the sequential leg's spread")
        f = lambda v: f"{med(v):8.2f} [{min(v):8.2f} .. {max(v):8.2f}]"
        lines.append(f"{k} | {f(a)} | {f(a2)} | {f(b)} | {gain:+7.2f} ms ({100 * gain / med(seq_all):+5.1f} %) | {spread:.2f} ms, range {rng_:.2f} ms | {verdict}")
        print(lines[-1], flush=True)
        try:
            gs, as_, es = kernel_split(seq)
            gb, ab, eb = kernel_split(bat)
            split_lines.append(f"{k} | seq: {gs:8.2f} / {as_:7.2f} / {es:7.2f} | batch: {gb:8.2f} / {ab:7.2f} / {eb:7.2f}")
        except Exception as e:  # the timing table does not depend on the profiler
            split_lines.append(f"{k} | profiler unavailable: {type(e).__name__}: {str(e)[:80]}")
        print(split_lines[-1], flush=True)
    out_dir = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"prefill_batch_{model}.txt"), "w") as fh:
        fh.write("\n".join(lines + split_lines) + "\n")


if __name__ == "__main__":
    main()
