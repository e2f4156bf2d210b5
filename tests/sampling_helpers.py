"""Shared pieces of the sampling-kernel tests (tests/test_sampling_ref_cpu.py, tests/test_sampling_kernels_gpu.py): a float64 reference of
csrc/tree_kernels.h's temperature > 0 path (vs_topk_threshold, vs_row_stats, vs_multinomial, verify_accept_sample_body), the two derived
bars, and the inputs both files use.  Plain numpy; nothing is imported from vispec_amd.csrc.  The reference is built so that the kernel's
only freedom against it is fp32 expf and the order of its sums."""
import math

import numpy as np

from helpers import vo
from logprob_helpers import U, bf16_round

THREADS = 1024  # the one block size of sample_row_kernel / verify_accept_sample_kernel
SEEDS = range(256)
FIRST_TOKEN_COUNTER = (0xFFFF, 0, 0)  # sample_row_kernel: vs_uniform(seed, 0xFFFF, 0, 0)


# ------------------------------------------------------------------------------------------------------------------ the reference
def ref_threshold(row_bf16, top_k):
    """TopKLogitsWarper's threshold: the top_k-th largest value of the row, -inf when the warper is off (top_k <= 0 or top_k >= V).  A token
    survives iff row >= threshold, so every tie with the k-th value survives (and +0.0 / -0.0 are one value)."""
    row = np.asarray(row_bf16, np.float32)
    if top_k <= 0 or top_k >= row.shape[0]:
        return np.float32(-np.inf)
    return np.partition(row, row.shape[0] - top_k)[row.shape[0] - top_k]


def ref_weights(row, T, top_k, removed=()):
    """float64 weights of the draw: exp of the fp32 argument  float32(float32(row) / float32(T)) - m  with m the fp32 max of row / T over the
    WHOLE row (vs_row_stats takes it before the top-k filter); 0 for filtered (row < threshold) and removed tokens.  Division, max and
    subtraction are correctly rounded fp32 operations here and in the kernel (the library is built without fast-math: vispec_amd/build.py),
    so the arguments are the kernel's bit for bit and only the exp differs: float64 here, fp32 expf there."""
    row = np.asarray(row, np.float32)
    x = row / np.float32(T)
    arg = x - x.max()
    assert arg.dtype == np.float32
    w = np.exp(arg.astype(np.float64))
    w[row < ref_threshold(row, top_k)] = 0.0
    if len(removed):
        w[np.asarray(removed, np.int64)] = 0.0
    return w


def uniforms(seeds=SEEDS, counter=FIRST_TOKEN_COUNTER):
    """The fp32 uniforms vs_uniform(seed, *counter) of the seeds, as float64 (k / 2^24: exact in both)."""
    return np.array([vo.uniform_hash(int(s), *counter) for s in seeds], np.float64)


class Cdf:
    """The inclusive float64 prefix sums of a configuration's weights, taken ONCE, and the draws / gaps / admissible draws of many uniforms."""

    def __init__(self, weights):
        self.w = np.asarray(weights, np.float64)
        self.cum = np.cumsum(self.w)
        self.total = float(self.cum[-1])
        self.support = np.nonzero(self.w > 0)[0]
        self.scum = self.cum[self.support]  # strictly increasing: one step per surviving token

    def draw(self, u):
        """(tokens, gaps) of uniforms u.  token = the first index whose inclusive prefix is > float64(u) * total; gap = the distance from
        u * total to the nearest prefix step (0 and the total included), divided by the total."""
        t = np.atleast_1d(np.asarray(u, np.float64)) * self.total
        k = np.minimum(np.searchsorted(self.scum, t, side="right"), len(self.support) - 1)
        lo = np.where(k > 0, self.scum[np.maximum(k - 1, 0)], 0.0)
        gap = np.minimum(t - lo, self.scum[k] - t) / self.total
        return self.support[k], gap

    def admissible(self, u, bar):
        """The tokens a correct kernel may draw with uniform u.  Unambiguous (gap >= bar): the reference's draw alone.  Ambiguous: that
        token or the adjacent surviving token on the side of the near step.  A neighbour whose own weight is below bar * total cannot be
        resolved by either side, so the walk goes on past such tokens to the first one that can: every admitted token's own interval
        comes within bar * total of u * total, which is what an error of bar * total in a prefix can move."""
        t = float(u) * self.total
        k = int(min(np.searchsorted(self.scum, t, side="right"), len(self.support) - 1))
        lo = self.scum[k - 1] if k > 0 else 0.0
        d_lo, d_hi = t - lo, self.scum[k] - t
        out = {int(self.support[k])}
        if min(d_lo, d_hi) >= bar * self.total:
            return out
        if d_lo <= d_hi:  # the near step is the lower one: tokens below whose interval ends within the bar of t
            j = k - 1
            while j >= 0 and t - self.scum[j] < bar * self.total:
                out.add(int(self.support[j]))
                j -= 1
        else:  # tokens above whose interval starts within the bar of t
            j = k + 1
            while j < len(self.support) and self.scum[j - 1] - t < bar * self.total:
                out.add(int(self.support[j]))
                j += 1
        return out


def ref_draw(weights, u):
    """(token, gap) of ONE inverse-CDF draw: the first index whose inclusive float64 prefix is > float64(u) * total."""
    tok, gap = Cdf(weights).draw(u)
    return int(tok[0]), float(gap[0])


def draw_bar():
    """The gap below which a draw counts as ambiguous: 2^-22 of the total.

    Kernel and reference exponentiate the SAME fp32 argument (ref_weights) and both accumulate in double, whose own error (~V * 2^-53) is
    five orders below what follows.  HIP documents expf with a maximum error of 1 ulp (HIP documentation, "HIP math API", table
    "Single precision mathematical functions": expf — maximum ULP error 1); one fp32 ulp is at most 2^-23 of the value, so each kernel
    weight is its reference weight times (1 + d), |d| <= 2^-23.  The weights are positive, so every kernel prefix P'_k is within
    2^-23 * P_k of the reference's, and the kernel's target u * total' within 2^-23 * u * total.  The sign of  P_k - u * total  — all the
    draw depends on — can therefore differ only where |P_k - u * total| <= 2^-23 * (P_k + u * total) <= 2^-22 * total.  (A weight so
    small that expf returns a subnormal, or flushes it, is off by at most 2^-126 in absolute terms against a total >= 1 — the arg-max
    contributes exp(0): nothing at this scale.)"""
    return 2.0 ** -22


def ref_posterior(logits, cand, T, top_k, uni):
    """oracle.evaluate_posterior_sampling (utils.py:453-493: sequential rejection over the tree's children) restated on ref_weights.
    logits [n_leaf, m, V] (bf16 values), cand [n_leaf, m] (-1 padded), uni(j, i) the uniform of path j at level i.
    -> (best, accept_len, removed tokens of the final draw, (path, depth) of the logits row of the final draw, comparisons) with one
    (j, i, u, px_ref, rm_ref) per comparison made.  p = w[x] / total, px = p / (1 - rm), rm = the sum of the p of the level's rejected
    tokens — all float64; dividing by (1 - rm) is the oracle's renormalisation after zeroing the rejected entries."""
    n_leaf, m = cand.shape
    acc = [int(cand[0, 0])]
    best, adjust, removed, last = 0, False, [], None
    comps = []
    for i in range(1, m):
        if i != len(acc):
            break
        adjust, removed = False, []
        eq = [j for j in range(n_leaf) if list(cand[j, :i]) == acc]
        fi = eq[0]
        last = (fi, i - 1)
        w = ref_weights(logits[fi, i - 1], T, top_k)
        total = w.sum()
        rm, seen = 0.0, set()
        for j in eq:
            x = int(cand[j, i])
            if x == -1 or x in seen:
                continue
            seen.add(x)
            p = w[x] / total
            px = p / (1.0 - rm) if rm < 1.0 else math.inf
            u = float(uni(j, i))
            comps.append((j, i, u, px, rm))
            if u <= px:
                acc.append(x)
                best = j
                break
            rm += p
            removed.append(x)
            adjust = True
    a = len(acc) - 1
    if adjust and len(acc) != m:
        return best, a, removed, last, comps
    return best, a, [], (best, a), comps


def accept_bar(V, px, rm, nrem=64):
    """Absolute error bound of the kernel's fp32  px = p / (1 - rm)  against ref_posterior's px, from the kernel's shape (u = 2^-24, first
    order in u; not tuned):
      Z     every term is an expf (1 ulp <= 2u, on the reference's own argument); a thread adds its n = ceil(V / 1024) terms in one fp32
            chain (n roundings at most), six shuffle steps add the wave's 64 chains (6), thread 0 .. 1023 then add the 16 wave sums from
            LDS (16): all terms positive, so relative errors add up to (n + 6 + 16 + 2) u.
      p     = expf(arg) / Z: 2u for the numerator, 1u for the division -> e_p = (n + 27) u.
      rm    the fp32 running sum of at most `nrem` (<= 64 tree nodes) earlier p: each within e_p, one rounding per add -> rm is within
            rm * (e_p + nrem * u).
      px    = p / (1.0f - rm): the subtraction rounds once (1u of 1 - rm) and carries rm's error, which is rm * (e_p + nrem * u) / (1 - rm)
            relative to 1 - rm; the division rounds once.
      => |px' - px| <= px * (e_p + 2u + rm * (e_p + nrem * u) / (1 - rm)).
    A filtered token has p = 0 on both sides (bar 0: only u = 0 is undecided); rm >= 1 leaves nothing to divide by (bar inf)."""
    if rm >= 1.0 or not math.isfinite(px):
        return math.inf
    e_p = (math.ceil(V / THREADS) + 27) * U
    return px * (e_p + 2 * U + rm * (e_p + nrem * U) / (1.0 - rm))


# ------------------------------------------------------------------------------------------------------------------ inputs of 2a
DRAW_V = [7, 1000, 1024, 1025, 32064, 152064]
DRAW_T = [0.7, 1.0, 6.0]
DRAW_TOPK = [0, 1, 8, 50]
MAX_AMBIGUOUS = 0.15  # condition on the inputs, not a measurement: at most this share of a configuration's 256 draws may be ambiguous


def draw_rows(V):
    """The three rows of 2a as exact bf16 values: N(0, 4^2) with ONE strict maximum, near-flat N(0, 0.05^2), all-equal."""
    rng = np.random.default_rng(1000 + V)
    wide = bf16_round(rng.standard_normal(V).astype(np.float32) * 4.0)
    top = int(np.argmax(wide))
    if (wide == wide[top]).sum() > 1:
        wide[top] = bf16_round(np.float32([wide[top] + 1.0]))[0]
    assert (wide == wide.max()).sum() == 1
    flat = bf16_round(rng.standard_normal(V).astype(np.float32) * 0.05)
    return {"wide": wide, "flat": flat, "equal": np.full(V, 1.5, np.float32)}


def draw_configs(V):
    """Every (row name, row, T, top_k) of 2a at this V."""
    rows = draw_rows(V)
    return [(name, row, T, k) for name, row in rows.items() for T in DRAW_T for k in DRAW_TOPK]


# ------------------------------------------------------------------------------------------------------------------ inputs of 2b
EDGE_V = [1025, 32064, 152064]  # chunk = 2 / 32 / 149 tokens per thread; 1025 and 152064 end in a partial chunk


def edge_rows(V):
    """Threshold edges: (name, row, top_k) at temperature 1.  The background is N(-40, 1) (no mass: exp(-30) of a survivor), survivors sit
    near +5 in steps of 1/16 — exact in bf16, weights within a factor e^(15/16) of each other."""
    rng = np.random.default_rng(2000 + V)
    chunk = -(-V // THREADS)
    bg = lambda: bf16_round(-40.0 + rng.standard_normal(V).astype(np.float32))
    hi = lambda n: np.float32(5.0) + np.arange(n, dtype=np.float32) / np.float32(16.0)
    out = []

    def put(name, idx, vals=None, top_k=None):
        row = bg()
        idx = np.asarray(idx, np.int64)
        assert len(set(idx.tolist())) == len(idx) and idx.min() >= 0 and idx.max() < V
        row[idx] = hi(len(idx)) if vals is None else np.asarray(vals, np.float32)
        assert np.array_equal(bf16_round(row), row)
        out.append((name, row, len(idx) if top_k is None else top_k))

    n_one = min(8, chunk)
    put("one_chunk", 500 * chunk + np.arange(n_one))
    waves = [(w * 64 + 5) * chunk + chunk - 1 for w in range(16)]
    put("one_per_wave", [i for i in waves if i < V])
    put("ends", [0, V - 1])
    last_lo = ((V - 1) // chunk) * chunk  # first token of the last non-empty chunk (partial at V = 1025, 152064)
    put("last_chunk", np.arange(last_lo, V)[-min(8, V - last_lo):])
    for ties in (1, 3, 200):  # top_k = 8: seven values above the k-th, which occurs `ties` times — 7 + ties tokens survive
        idx = rng.choice(V, 7 + ties, replace=False)
        put(f"tied_{ties}", idx, np.concatenate([hi(8)[1:], np.full(ties, 5.0, np.float32)]), top_k=8)
    row = bf16_round(-np.abs(rng.standard_normal(V).astype(np.float32)) * 4.0 - 1.0)
    out.append(("all_negative", row, 8))
    # +0.0 and -0.0 around the k-th value: 3 values above, then 3 x +0.0 and 3 x -0.0 (one value: all six survive top_k = 5), the rest below
    idx = rng.choice(V, 9, replace=False)
    put("signed_zeros", idx, [1.0, 0.5, 0.25, 0.0, -0.0, 0.0, -0.0, -0.0, 0.0], top_k=5)
    assert np.signbit(out[-1][1][idx]).sum() == 3
    few = rng.choice(V, 12, replace=False)
    put("top_k_is_V", few, top_k=V)  # the threshold is off: the whole row is the support
    put("top_k_is_V_plus_1", few, top_k=V + 1)
    return out


# ------------------------------------------------------------------------------------------------------------------ inputs of 2c
ACCEPT_V = [32064, 152064]
ACCEPT_T = [0.7, 1.3]
ACCEPT_TOPK = [0, 12]
ACCEPT_CASES = 24
U_LAST = 1.0 - 2.0 ** -24  # the generator's largest value


def accept_tree(V, rng, n_leaf, m):
    """A candidate table like G7's: one root, shared prefixes, duplicate children, one -1 padded path; the tokens of a level lie in
    chunks far apart (multiples of ~V/9 plus a small offset)."""
    far = lambda: int(rng.integers(0, 9)) * (V // 9) + int(rng.integers(0, V // 9))
    cand = np.full((n_leaf, m), -1, np.int64)
    cand[:, 0] = far()
    for j in range(n_leaf):
        for i in range(1, m):
            if j > 0 and (cand[j - 1, :i] == cand[j, :i]).all() and rng.random() < 0.45:
                cand[j, i] = cand[j - 1, i]  # a shared prefix (or, one level further, a duplicate child)
            else:
                cand[j, i] = far()
    cand[n_leaf - 1, m - 1] = -1  # a padded path
    return cand


def accept_case(V, c):
    """Case c of V: (cand, logits [n_leaf, m, V] bf16 values, T, top_k, u [n_leaf, m] fp32, u_final, redrawn count).  N(0, 4^2) rows; in
    the odd cases the candidates along path 0 are boosted (accepts happen), and in every case the children of the root are lifted so
    that rejected tokens carry mass.  The override uniforms come from a seeded generator; any u[j, i] that ref_posterior compares within
    accept_bar of its px is drawn again — until every comparison made is decided."""
    rng = np.random.default_rng(3000 + 101 * c + V)
    n_leaf, m = int(rng.integers(3, 7)), int(rng.integers(3, 6))
    T, top_k = ACCEPT_T[c % 2], ACCEPT_TOPK[(c // 2) % 2]
    cand = accept_tree(V, rng, n_leaf, m)
    logits = bf16_round(rng.standard_normal((n_leaf, m, V)).astype(np.float32) * 4.0)
    for j in range(n_leaf):
        for i in range(1, m):
            if cand[j, i] >= 0:  # every row that can judge this child (all paths sharing the prefix) gives it some mass
                for jj in range(n_leaf):
                    if (cand[jj, :i] == cand[j, :i]).all():
                        logits[jj, i - 1, cand[j, i]] = bf16_round(np.float32([14.0 + 2.0 * rng.random()]))[0]
    if c % 4 >= 2:
        for i in range(1, m):
            if cand[0, i] >= 0:
                for jj in range(n_leaf):
                    if (cand[jj, :i] == cand[0, :i]).all():
                        logits[jj, i - 1, cand[0, i]] = np.float32(22.0)
    u = (rng.integers(0, 1 << 24, size=(n_leaf, m)) / float(1 << 24)).astype(np.float32)
    u_final = float(np.float32(rng.integers(0, 1 << 24) / float(1 << 24)))
    redrawn = 0
    for _ in range(1000):
        comps = ref_posterior(logits, cand, T, top_k, lambda j, i: u[j, i])[4]
        close = [(j, i) for j, i, uu, px, rm in comps if abs(uu - px) <= accept_bar(V, px, rm)]
        if not close:
            break
        for j, i in close:
            u[j, i] = np.float32(rng.integers(0, 1 << 24) / float(1 << 24))
            redrawn += 1
    else:
        raise AssertionError("the redraw loop did not end")
    return cand, logits, T, top_k, u, u_final, redrawn


def scripted_case(V, u_final):
    """Every child of the root is rejected (u = 2 is never accepted), the residual draw runs with u_final at T = 1.3, top_k = 12."""
    for c in range(ACCEPT_CASES):  # the first case whose root has three or more distinct children
        cand, logits, _, _, u, _, _ = accept_case(V, c)
        if len(set(cand[:, 1].tolist()) - {-1}) >= 3:
            break
    else:
        raise AssertionError("no case with three children of the root")
    return cand, logits, 1.3, 12, np.full_like(u, 2.0), u_final
