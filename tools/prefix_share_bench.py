"""k questions about ONE image: k full request starts against one prefill_prefix + fork + k suffix prefills, at a bench prompt shape.   GPU only.

    python tools/prefix_share_bench.py llava7b|qwen7b [reps] [out_dir]      -> <out_dir = profiles>/prefix_share_<model>.txt (and stdout)

One process, an otherwise idle GPU.  The prompt is a bench request; the prefix is everything up to and including its last image token
(LLaVA-7B: 2192 of 2704 rows), the k questions share it and differ in the text rows behind it.  For k in {1, 2, 4, 8}, after warm-up, the
legs alternate  a, b, a', c  for `reps` repetitions:
  (a) k full request starts as today (SpecModel._start_request per slot: target prefill of all L rows, first token, draft prefill);
  (b) prefill_prefix once + ONE fork into the k caches + k suffix prefills at past_len = P, then the same last stage per request;
  (c) the same with batch_prefill=True (one walk over the k suffixes).
Leg (a) runs twice per repetition: its two interleaved series a / a' give its own spread, and a difference of (b) or (c) from (a) counts only
where it exceeds that spread ("within spread" otherwise).  Times are stream time between two events around a leg (ms), medians and ranges.
The bench request carries its image features ready in HBM (the vision tower is not inside these legs), so what is compared is the target
prefill work alone; a deployment whose requests run the vision front-end saves k - 1 runs of it on top.  k = 1 is printed as it is: a
single question pays the prefix, a store copy and a fork on top of its rows.
The copy kernel alone: Engine.load_kv_rows of the prefix into n = 1, 2, 4, 8 caches (and Engine.save_kv_rows), as GB/s over bytes read +
written, next to n strided torch copy_ calls of the same bytes in the same process, and as a fraction of the 6.3 TB/s the project treats
as achievable."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from vispec_amd.model.spec_model_ours import _start_requests  # noqa: E402

KS = (1, 2, 4, 8)
ACHIEVABLE_GBS = 6300.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    model = sys.argv[1] if len(sys.argv) > 1 else "llava7b"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    bench.MODEL = model
    dev = torch.device("cuda:0")
    lanes, tcfg, _ = bench.build_models(dev, 0, 0, 1, 1, 8)
    models = lanes[0]
    lead = models[0]
    ids, kw = bench.make_request(tcfg, 70, dev)
    Ln = int(ids.shape[1])
    visual = (ids[0] == tcfg.image_token_index)
    P = int(visual.nonzero().max()) + 1
    g = torch.Generator().manual_seed(7)
    questions = []
    for _ in range(max(KS)):  # the same prefix, other text behind it
        q = ids.clone()
        q[0, P:] = torch.randint(3, 30000, (Ln - P,), generator=g).to(dev)
        questions.append(q)
    gen = dict(temperature=0.0, top_k=0.0, is_llama3=False)
    med = statistics.median
    f = lambda v: f"{med(v):8.2f} [{min(v):8.2f} .. {max(v):8.2f}]"
    lines = [f"# tools/prefix_share_bench.py {model} reps={reps}: prompt rows {Ln}, prefix rows {P}, {torch.cuda.get_device_name(0)}, "
             f"prefill GEMMs: {__import__('vispec_amd.model.target', fromlist=['x']).prefill_gemm_selection()}",
             "# ms per leg (stream time), median [min .. max]; a / a' = the two interleaved series of the k full starts",
             "# k | a | a' | b: prefix + fork + k suffix starts | c: the same, one batched walk | b vs a | c vs a | spread of a | verdict b / c"]

    def prefixed(k, batch):
        pfx = lead.prefill_prefix(ids[:, :P], **kw)
        _start_requests(models[:k], [(q, {}) for q in questions[:k]], [0] * k, [64] * k, gen, prefixes=[pfx] * k, batch_prefill=batch)

    for k in KS:
        leg_a = lambda: [m._start_request(q, None, dict(kw)) for m, q in zip(models[:k], questions)]
        leg_b = lambda: prefixed(k, False)
        leg_c = lambda: prefixed(k, True)
        for _ in range(2):
            leg_a(), leg_b(), leg_c()
        torch.cuda.synchronize()
        a, a2, b, c = [], [], [], []
        for _ in range(reps):
            a.append(timed(leg_a))
            b.append(timed(leg_b))
            a2.append(timed(leg_a))
            c.append(timed(leg_c))
        a_all = a + a2
        spread = max(abs(med(a) - med(a2)), max(a_all) - min(a_all))
        verdict = lambda d: "gain" if d > spread else ("loss" if -d > spread else "within spread")
        db, dc = med(a_all) - med(b), med(a_all) - med(c)
        lines.append(f"{k} | {f(a)} | {f(a2)} | {f(b)} | {f(c)} | {db:+8.2f} ms ({100 * db / med(a_all):+5.1f} %) | {dc:+8.2f} ms ({100 * dc / med(a_all):+5.1f} %) | "
                     f"{spread:.2f} ms | {verdict(db)} / {verdict(dc)}")
        print(lines[-1], flush=True)

    # the copy kernel alone
    pfx = lead.prefill_prefix(ids[:, :P], **kw)
    store = pfx.store
    one = store.numel() * store.element_size()
    lines += [f"# copy: store {one / 1e6:.1f} MB ({P} rows x {store.shape[0] * store.shape[1]} planes); GB/s over bytes read + written, median of {reps}; "
              f"fraction of {ACHIEVABLE_GBS / 1e3:.1f} TB/s",
              "# what | n | kernel ms | kernel GB/s (fraction) | n x torch copy_ ms | torch GB/s | verdict"]
    engines = [m.engine for m in models]

    def row(what, n, fn_kernel, fn_torch, moved):
        for _ in range(2):
            fn_kernel(), fn_torch()
        tk, tt = [], []
        for _ in range(reps):
            tk.append(timed(fn_kernel))
            tt.append(timed(fn_torch))
        gk, gt = moved / med(tk) / 1e6, moved / med(tt) / 1e6
        lines.append(f"{what} | {n} | {f(tk)} | {gk:7.0f} ({gk / ACHIEVABLE_GBS:.2f}) | {f(tt)} | {gt:7.0f} | "
                     f"{'kernel faster' if med(tk) < min(tt) else ('torch faster' if med(tt) < min(tk) else 'within spread')}")
        print(lines[-1], flush=True)

    for n in KS:
        row("fork", n, lambda: lead.engine.load_kv_rows(store, engines[:n]),
            lambda: [e.target_kv[:, 0, :, :P].copy_(store) for e in engines[:n]], one * (1 + n))
    spare = torch.empty_like(store)
    row("save", 1, lambda: lead.engine.save_kv_rows(P), lambda: spare.copy_(lead.engine.target_kv[:, 0, :, :P]), one * 2)

    out_dir = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"prefix_share_{model}.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
