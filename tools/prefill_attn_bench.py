"""The prefill attention's three doors onto one sequence against torch's flash SDPA, on the target prefill's shapes (causal flops =
2 L^2 128 H): vispec_prefill_attention, vispec_prefill_attention_varlen with one segment, vispec_prefill_attention_at with pos0 = 0.
The legs alternate over REPS repetitions (each 50 calls between two device events, after a warm-up of 50 calls of every leg); a leg prints its median
and its minimum..maximum, so two legs are compared against the spread of the same run.   GPU only."""
import ctypes as C, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vispec_amd import lib as L
lib = L.load()
dev = torch.device("cuda:0")
p = lambda t: C.c_void_p(t.data_ptr())
REPS, CALLS = 9, 50
for Ln, H, HK, eager in ((2704, 32, 32, 1), (3488, 32, 32, 1), (2704, 40, 40, 1), (1584, 28, 4, 0), (2124, 28, 4, 0), (643, 32, 32, 1)):
    S = 8192
    qkv = torch.randn(Ln, (H + 2 * HK) * 128, device=dev, dtype=torch.bfloat16)
    kc = torch.randn(HK, S, 128, device=dev, dtype=torch.bfloat16)
    vc = torch.randn(HK, S, 128, device=dev, dtype=torch.bfloat16)
    out = torch.empty(Ln, H * 128, device=dev, dtype=torch.bfloat16)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    seg = (L.PrefillSeg * 1)(L.PrefillSeg(0, Ln, kc.data_ptr(), vc.data_ptr()))
    q4 = qkv[:, : H * 128].view(Ln, H, 128).transpose(0, 1)[None]
    legs = {
        "single": lambda: L.check(lib.vispec_prefill_attention(None, st, p(qkv), qkv.shape[1], p(kc), p(vc), S, H, HK, Ln, p(out), H * 128, eager)),
        "varlen": lambda: L.check(lib.vispec_prefill_attention_varlen(None, st, p(qkv), qkv.shape[1], seg, 1, S, H, HK, p(out), H * 128, eager)),
        "at": lambda: L.check(lib.vispec_prefill_attention_at(None, st, p(qkv), qkv.shape[1], p(kc), p(vc), S, H, HK, 0, Ln, p(out), H * 128, eager)),
        "torch sdpa": lambda: torch.nn.functional.scaled_dot_product_attention(q4, kc[None, :, :Ln], vc[None, :, :Ln], is_causal=True,
                                                                                enable_gqa=(H != HK)),
    }
    us, failed = {name: [] for name in legs}, {}
    for name, fn_ in legs.items():
        try:
            for _ in range(CALLS): fn_()  # a timed window's worth
            torch.cuda.synchronize()
        except Exception as e:
            failed[name] = str(e)[:60]
    for _ in range(REPS):
        for name, fn_ in legs.items():
            if name in failed: continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS): fn_()
            e1.record(); torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1000 / CALLS)
    res = []
    for name in legs:
        if name in failed:
            res.append(f"{name} failed: {failed[name]}")
            continue
        med = statistics.median(us[name])
        res.append(f"{name} {med:7.1f} us ({min(us[name]):.1f}..{max(us[name]):.1f}) {2 * Ln * Ln * 128 * H / med / 1e6:5.0f} TF")
    ref = None
    if H == HK and not {"single", "torch sdpa"} & set(failed):
        legs["single"](); torch.cuda.synchronize()
        ref = legs["torch sdpa"]()
    err = "" if ref is None else f" | max |single - sdpa| {float((out.view(Ln, H, 128).transpose(0, 1).float() - ref[0].float()).abs().max()):.4f}"
    print(f"L={Ln} H={H}/{HK} eager={eager}, {REPS} x {CALLS} calls: " + " | ".join(res) + err, flush=True)
