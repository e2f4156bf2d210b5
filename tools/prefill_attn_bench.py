"""The prefill attention's three doors onto one sequence against torch's flash SDPA, on the target prefill's shapes (causal flops =
2 L^2 128 H): vispec_prefill_attention, vispec_prefill_attention_varlen with one segment, vispec_prefill_attention_at with pos0 = 0; and the
rotary/append's two: vispec_rope_append_varlen against vispec_rope_append_varlen_at with pos0 = 0, one segment, on the same shapes.
The legs of a group alternate over REPS repetitions (each 50 calls between two device events, after a warm-up of 50 calls of every leg); a
leg prints its median and its minimum..maximum, so two legs are compared against the spread of the same run: leg A "costs nothing" against
leg B when A's median lies inside B's own min..max (or below it) — the `A in B` column.  (The order inside a repetition is fixed, and the
first attention leg, which follows the SDPA leg of the repetition before, has read 4–6 % slow on the long MHA shapes: NOTEBOOK.)

--parent-lib PATH loads a second build of the library beside the tree's, in the same process: its legs (P:) alternate with the tree's (T:),
every tree leg is held against the parent's leg of the same entry, and the output BYTES of the two builds are compared per leg — on the
timed shapes and on the single-call shapes CASES x HEADS x eager 0/1 — as `identical` or the number of differing elements.   GPU only."""
import argparse, ctypes as C, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vispec_amd import lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None, help="a second build of libvispec_hip.so to alternate with and compare against")
args = ap.parse_args()
builds = {"T": L.load()}
if args.parent_lib:
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    for name, (res, argtypes) in L.SIGNATURES.items():
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = res, argtypes
    builds = {"P": parent, "T": builds["T"]}
dev = torch.device("cuda:0")
p = lambda t: C.c_void_p(t.data_ptr())
REPS, CALLS = 9, 50
SHAPES = ((2704, 32, 32, 1), (3488, 32, 32, 1), (2704, 40, 40, 1), (1584, 28, 4, 0), (2124, 28, 4, 0), (643, 32, 32, 1))
CASES = ((0, 1), (0, 129), (0, 300), (96, 64), (127, 2))  # (pos0, M) of the single-call byte comparison
HEADS = ((4, 4), (14, 2))


def ok(lib, rc):
    if rc != 0:
        raise RuntimeError((lib.vispec_last_error() or b"?").decode())


class Case:
    """One sequence: M rows at positions [pos0, pos0 + M) over caches of S rows.  The attention legs read qkv / kc / vc and write out; the
    rotary legs rotate rqkv in place and append to rkc / rvc (buffers of their own, so that the attention legs' inputs never change)."""

    def __init__(self, pos0, M, H, HK, eager, S):
        self.pos0, self.M, self.H, self.HK, self.eager, self.S = pos0, M, H, HK, eager, S
        g = torch.Generator(device=dev).manual_seed(1000 * M + pos0 + H)
        rnd = lambda *s: torch.randn(*s, device=dev, dtype=torch.bfloat16, generator=g)
        self.qkv, self.kc, self.vc = rnd(M, (H + 2 * HK) * 128), rnd(HK, S, 128), rnd(HK, S, 128)
        self.out = torch.empty(M, H * 128, device=dev, dtype=torch.bfloat16)
        self.rqkv0 = rnd(M, (H + 2 * HK) * 128)
        self.rqkv, self.rkc, self.rvc = self.rqkv0.clone(), torch.zeros_like(self.kc), torch.zeros_like(self.vc)
        ang = torch.arange(S, device=dev, dtype=torch.float32)[:, None] * (10000.0 ** (-torch.arange(64, device=dev) / 64.0))[None]
        self.cos, self.sin = (f(torch.cat([ang, ang], 1)).to(torch.bfloat16).contiguous() for f in (torch.cos, torch.sin))
        self.seg = (L.PrefillSeg * 1)(L.PrefillSeg(0, M, self.kc.data_ptr(), self.vc.data_ptr()))
        self.rseg = (L.PrefillSeg * 1)(L.PrefillSeg(0, M, self.rkc.data_ptr(), self.rvc.data_ptr()))
        self.rseg_at = (L.PrefillSegAt * 1)(L.PrefillSegAt(0, M, pos0, 0, self.rkc.data_ptr(), self.rvc.data_ptr()))

    def attn_legs(self, lib):
        c, st, ld = self, C.c_void_p(torch.cuda.current_stream().cuda_stream), self.qkv.shape[1]
        legs = {"at": lambda: ok(lib, lib.vispec_prefill_attention_at(None, st, p(c.qkv), ld, p(c.kc), p(c.vc), c.S, c.H, c.HK, c.pos0, c.M, p(c.out),
                                                                     c.H * 128, c.eager))}
        if c.pos0 == 0:
            legs["single"] = lambda: ok(lib, lib.vispec_prefill_attention(None, st, p(c.qkv), ld, p(c.kc), p(c.vc), c.S, c.H, c.HK, c.M, p(c.out),
                                                                          c.H * 128, c.eager))
            legs["varlen"] = lambda: ok(lib, lib.vispec_prefill_attention_varlen(None, st, p(c.qkv), ld, c.seg, 1, c.S, c.H, c.HK, p(c.out), c.H * 128,
                                                                                 c.eager))
        return {k: legs[k] for k in ("single", "varlen", "at") if k in legs}

    def rope_legs(self, lib):
        c, st = self, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        legs = {}
        if c.pos0 == 0:
            legs["rope varlen"] = lambda: ok(lib, lib.vispec_rope_append_varlen(None, st, p(c.rqkv), c.H, c.HK, 128, p(c.cos), p(c.sin), 0, c.rseg, 1, c.S))
        legs["rope at"] = lambda: ok(lib, lib.vispec_rope_append_varlen_at(None, st, p(c.rqkv), c.H, c.HK, 128, p(c.cos), p(c.sin), 0, c.rseg_at, 1, c.S))
        return legs

    def result(self, name, fn_):
        """The bytes one call of a leg leaves behind, from the same inputs whichever build runs it."""
        if name.startswith("rope"):
            self.rqkv.copy_(self.rqkv0); self.rkc.zero_(); self.rvc.zero_()
            fn_(); torch.cuda.synchronize()
            return torch.cat([t.reshape(-1).view(torch.int16) for t in (self.rqkv, self.rkc, self.rvc)])
        self.out.zero_()
        fn_(); torch.cuda.synchronize()
        return self.out.reshape(-1).view(torch.int16).clone()

    def compare(self):
        """Parent against tree, per leg: `identical` or the number of differing elements."""
        res = []
        for name in list(self.attn_legs(builds["T"])) + list(self.rope_legs(builds["T"])):
            got = [self.result(name, {**self.attn_legs(b), **self.rope_legs(b)}[name]) for b in (builds["P"], builds["T"])]
            n = int((got[0] != got[1]).sum())
            res.append(f"{name} " + ("identical" if n == 0 else f"{n} of {got[0].numel()} elements differ"))
        return " | ".join(res)


def timed(legs):
    """{name: fn} -> ({name: [us per call] * REPS}, {name: error}); the legs alternate inside every repetition."""
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
    return us, failed


def report(us, failed, pairs, tf=None):
    for name in us:
        if name in failed:
            print(f"  {name:<14} failed: {failed[name]}")
            continue
        med = statistics.median(us[name])
        print(f"  {name:<14} {med:7.1f} us ({min(us[name]):.1f}..{max(us[name]):.1f})" + (f" {tf / med / 1e6:5.0f} TF" if tf else ""))
    for a, b in pairs:
        if a in us and b in us and not {a, b} & set(failed):
            med = statistics.median(us[a])
            print(f"  {a} in {b}: " + ("yes" if med <= max(us[b]) else f"NO ({med:.1f} us > {max(us[b]):.1f} us)"))


for Ln, H, HK, eager in SHAPES:
    c = Case(0, Ln, H, HK, eager, 8192)
    q4 = c.qkv[:, : H * 128].view(Ln, H, 128).transpose(0, 1)[None]
    sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(q4, c.kc[None, :, :Ln], c.vc[None, :, :Ln], is_causal=True, enable_gqa=(H != HK))
    tag = (lambda b: b + ":") if args.parent_lib else (lambda b: "")
    attn = {tag(b) + n: f for b, lib in builds.items() for n, f in c.attn_legs(lib).items()}
    rope = {tag(b) + n: f for b, lib in builds.items() for n, f in c.rope_legs(lib).items()}
    if args.parent_lib:
        pairs_a, pairs_r = [("T:" + n, "P:" + n) for n in ("single", "varlen", "at")], [("T:" + n, "P:" + n) for n in ("rope varlen", "rope at")]
    else:
        pairs_a, pairs_r = [("at", "varlen"), ("at", "single")], [("rope at", "rope varlen")]
    print(f"L={Ln} H={H}/{HK} eager={eager}, {REPS} x {CALLS} calls", flush=True)
    us, failed = timed({**attn, "torch sdpa": sdpa})
    report(us, failed, pairs_a, tf=2 * Ln * Ln * 128 * H)
    if H == HK and not {tag("T") + "single", "torch sdpa"} & set(failed):
        attn[tag("T") + "single"](); torch.cuda.synchronize()
        print(f"  max |single - sdpa| {float((c.out.view(Ln, H, 128).transpose(0, 1).float() - sdpa()[0].float()).abs().max()):.4f}")
    us, failed = timed(rope)
    report(us, failed, pairs_r)
    if args.parent_lib:
        print("  parent against tree: " + c.compare(), flush=True)
if args.parent_lib:
    for H, HK in HEADS:
        for eager in (0, 1):
            for pos0, M in CASES:
                print(f"pos0={pos0} M={M} H={H}/{HK} eager={eager}, parent against tree: " + Case(pos0, M, H, HK, eager, 512).compare(), flush=True)
