"""TargetLM.prefill in pieces (chunk_rows) against the unchunked prefill of the same prompt, at a bench prompt shape.   GPU only.

    python tools/prefill_chunk_bench.py llava7b|qwen7b [reps] [out_dir]      -> <out_dir = profiles>/prefill_chunk_<model>.txt (and stdout)

One process, an otherwise idle GPU.  Legs: unchunked, chunk_rows = 2048, 1024, 512, 256 (a chunk size of at least the prompt's rows is the
unchunked call and is reported as such).  After warm-up the legs alternate  whole, c2048, c1024, c512, c256, whole, ...  for `reps`
repetitions; the yardstick of every chunked leg is the unchunked leg of the same process.  Times are stream time between two events around
a leg (ms), medians over the repetitions.  Memory: torch.cuda.max_memory_allocated above the resident baseline (weights, caches, the
prompt's embeddings) over one call of the leg, measured after the timing.  Chunking re-reads the weights once per piece and runs its GEMMs
at M = chunk_rows, shapes the recorded TunableOp table does not hold: it is expected to cost time and to save workspace; no threshold."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

CHUNKS = (None, 2048, 1024, 512, 256)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def peak_above_baseline(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    floor = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - floor


def main():
    model = sys.argv[1] if len(sys.argv) > 1 else "llava7b"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    bench.MODEL = model
    dev = torch.device("cuda:0")
    lanes, tcfg, _ = bench.build_models(dev, 0, 0, 1, 1, 1)
    sm = lanes[0]
    base = sm.base_model
    ids, kw = bench.make_request(tcfg, 70, dev)
    prep = sm._start_prepare(ids, None, dict(kw))  # the first stage of a request start: embeddings (+ M-RoPE positions) of a bench request
    Ln = int(prep.emb.shape[0])
    legs = [(c, (lambda c=c: base.prefill(prep.emb, position_ids=prep.position_ids, chunk_rows=c))) for c in CHUNKS]
    for _ in range(2):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in legs]
    for _ in range(reps):
        for i, (_, fn) in enumerate(legs):
            ms[i].append(timed(fn))
    peaks = [peak_above_baseline(fn) for _, fn in legs]
    med = statistics.median
    lines = [f"# tools/prefill_chunk_bench.py {model} reps={reps}: prompt rows {Ln}, {torch.cuda.get_device_name(0)}, "
             f"prefill GEMMs: {__import__('vispec_amd.model.target', fromlist=['x']).prefill_gemm_selection()}",
             "# prefill ms (stream time), median [min .. max] over the repetitions; peak = max_memory_allocated above the resident baseline",
             "# chunk_rows | pieces | ms | vs unchunked | peak MiB | vs unchunked"]
    for (c, _), v, pk in zip(legs, ms, peaks):
        whole = c is None or c >= Ln
        name = "unchunked" if c is None else (f"{c} (>= {Ln} rows: the unchunked call)" if whole else str(c))
        pieces = 1 if whole else -(-Ln // c)
        lines.append(f"{name} | {pieces} | {med(v):8.2f} [{min(v):8.2f} .. {max(v):8.2f}] | {med(v) - med(ms[0]):+7.2f} ms ({100 * (med(v) / med(ms[0]) - 1):+5.1f} %) | "
                     f"{pk / 2 ** 20:9.1f} | {100 * (pk / peaks[0] - 1):+5.1f} %")
        print(lines[-1], flush=True)
    out_dir = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"prefill_chunk_{model}.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
