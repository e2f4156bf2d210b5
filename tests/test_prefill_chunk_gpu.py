"""Chunked prompt prefill: the offset HIP kernels (vispec_prefill_attention_at / _varlen_at, vispec_rope_append_varlen_at) against the
unchunked entries bit for bit, TargetLM.prefill(chunk_rows=, past_len=) and prefill_batch(chunk_rows=) against the oracle's bf16 forward,
and the prefill_chunk_rows option of specgenerate / specgenerate_cohort / specgenerate_stream on the tiny models.

Arithmetic class that these tests pin down: a row at position p runs the same key tiles with the same mask whatever the offset of its
chunk, so both offset kernels are bit-identical to the unchunked kernels row for row; the library GEMMs run at M = the piece's rows and
may sum in another fp32 order, so a chunked prefill is held to the oracle within the bar of the single-request prefill comparisons
(test_stage_fixtures_gpu.close: 2^-6 of the tensor's largest magnitude), and to itself exactly where the pieces coincide."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from helpers import T, synth, vo  # noqa: E402
from test_loop_gpu import IMG_TOK, build, build_qwen  # noqa: E402
from test_prefill_batch_gpu import (CANARY, embeds_of, llava_prompt, p, packed_row0, qwen_prompt, rand_bf16, same_tuples, stream,  # noqa: E402
                                    t_bf16, tiny_requests)
from test_stage_fixtures_gpu import close  # noqa: E402  (the bar of the single-request prefill comparisons)
from vispec_amd import lib as L  # noqa: E402
from vispec_amd.model.spec_model_ours import specgenerate_cohort, specgenerate_stream  # noqa: E402

i16 = lambda t: t.view(torch.int16)
err = lambda lib: (lib.vispec_last_error() or b"").decode()
# (pos0, M): one row, rows inside / filling / leaving a 32-key tile, waves that straddle two diagonal tiles (96, 64), the 128-key chunk
# edges, more than one row block at an unaligned offset, one row / two blocks deep in a long cache
EDGES = [(1, 1), (31, 1), (32, 32), (33, 31), (96, 64), (127, 2), (128, 128), (129, 127), (200, 300), (2047, 1), (1920, 256)]
HEADS = [(4, 4), (14, 2)]


def segs_at(row0, lens, pos0, ks, vs):
    segs = (L.PrefillSegAt * len(lens))()
    for i in range(len(lens)):
        segs[i] = L.PrefillSegAt(row0[i], lens[i], pos0[i], 0, ks[i].data_ptr(), vs[i].data_ptr())
    return segs


@functools.lru_cache(maxsize=None)
def attention_case(Ln, H, Hkv, eager):
    """Random q [Ln, ldq], K/V [Hkv, S, 128] and the full kernel's output for them: computed once per shape, shared, never modified."""
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(4242 + Ln + 7 * H + eager)
    S = (Ln + 127) // 128 * 128 + 64
    ldq, ldo = (H + 2 * Hkv) * 128, H * 128
    q, k, v = rand_bf16(gen, Ln, ldq), rand_bf16(gen, Hkv, S, 128), rand_bf16(gen, Hkv, S, 128)
    want = torch.full((Ln, ldo), CANARY, dtype=torch.bfloat16, device="cuda")
    L.check(lib.vispec_prefill_attention(None, stream(), p(q), ldq, p(k), p(v), S, H, Hkv, Ln, p(want), ldo, eager))
    torch.cuda.synchronize()
    assert not (want == CANARY).all(dim=1).any()
    return q, k, v, S, want


def attention_at(lib, case, H, Hkv, eager, pos0, M, out):
    """rows [pos0, pos0 + M) of `out` <- vispec_prefill_attention_at on q rows [pos0, pos0 + M)"""
    q, k, v, S, _ = case
    ldq, ldo = (H + 2 * Hkv) * 128, H * 128
    L.check(lib.vispec_prefill_attention_at(None, stream(), p(q[pos0:]), ldq, p(k), p(v), S, H, Hkv, pos0, M, p(out[pos0:]), ldo, eager))


# ------------------------------------------------------------------------------------------------------------ 1. attention at an offset
@pytest.mark.parametrize("eager", [1, 0])
@pytest.mark.parametrize("pos0,M,H,Hkv", [(a, b, h, k) for a, b in EDGES for h, k in HEADS] + [(1000, 2000, 32, 32)])
def test_offset_attention_is_the_full_kernel_bit_for_bit(pos0, M, H, Hkv, eager):
    """Rows [pos0, pos0 + M) of a prefill of pos0 + M rows, computed from their q rows alone over the same cache == the rows
    vispec_prefill_attention computes for them (array equality on the bit patterns); no other row of the out buffer is written.
    (32 heads, pos0 = 1000, M = 2000: 16 row blocks of 32 heads, the paired long + short launch.)"""
    lib = L.load()
    Ln = pos0 + M
    case = attention_case(Ln, H, Hkv, eager)
    out = torch.full((Ln + 3, H * 128), CANARY, dtype=torch.bfloat16, device="cuda")
    attention_at(lib, case, H, Hkv, eager, pos0, M, out)
    torch.cuda.synchronize()
    assert torch.equal(i16(out[pos0:Ln]), i16(case[4][pos0:]))
    assert (out[:pos0] == CANARY).all() and (out[Ln:] == CANARY).all()


# -------------------------------------------------------------------------------------------------------------------- 2. splitting composes
@pytest.mark.parametrize("eager", [1, 0])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_two_offset_calls_compose_to_the_single_call(H, Hkv, eager):
    """L = 300 cut at c into rows [0, c) (pos0 = 0) and [c, 300) (pos0 = c): together the single call, bit for bit."""
    lib = L.load()
    Ln = 300
    case = attention_case(Ln, H, Hkv, eager)
    for c in (1, 31, 32, 33, 127, 128, 129, 299):
        out = torch.full((Ln, H * 128), CANARY, dtype=torch.bfloat16, device="cuda")
        attention_at(lib, case, H, Hkv, eager, 0, c, out)
        attention_at(lib, case, H, Hkv, eager, c, Ln - c, out)
        torch.cuda.synchronize()
        assert torch.equal(i16(out), i16(case[4])), f"cut at {c}"


# ----------------------------------------------------------------------------------------------------------- 3. varlen at an offset
# [(pos0, len) per segment], pad rows between segments
VARLEN_SETS = [([(0, 129), (77, 200)], 0), ([(96, 64), (0, 1), (200, 300)], 5), ([(31, 1), (0, 300), (128, 128), (5, 33)], 131),
               ([(0, 257), (100, 129), (1, 1), (640, 64), (0, 1), (33, 31), (127, 2), (300, 260)], 0)]


@pytest.mark.parametrize("eager", [1, 0])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_varlen_offset_attention_is_the_single_offset_entry_bit_for_bit(H, Hkv, eager):
    """Every output row of a varlen-at launch == the row vispec_prefill_attention_at computes for that segment alone; rows between the
    segments (padded row0) keep their canary.  Segments at pos0 = 0 and pos0 > 0 mixed, eight segments, and two consecutive pieces whose
    second continues a cache of the first."""
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(99 + H + eager)
    ldq, ldo = (H + 2 * Hkv) * 128, H * 128
    S = 1024
    caches = [(rand_bf16(gen, Hkv, S, 128), rand_bf16(gen, Hkv, S, 128)) for _ in range(8)]
    pieces = [(s, pad, list(range(len(s)))) for s, pad in VARLEN_SETS]
    pieces.append(([(0, 100), (0, 28)], 0, [0, 1]))         # piece A: cache 0 rows [0, 100), cache 1 rows [0, 28)
    pieces.append(([(100, 80), (28, 48)], 0, [0, 1]))       # piece B: the same two caches, continued
    for seg_list, pad, cache_ix in pieces:
        pos0, lens = [s[0] for s in seg_list], [s[1] for s in seg_list]
        n = len(lens)
        row0, total = packed_row0(lens, pad)
        q = rand_bf16(gen, total, ldq)
        ks, vs = [caches[c][0] for c in cache_ix], [caches[c][1] for c in cache_ix]
        out = torch.full((total, ldo), CANARY, dtype=torch.bfloat16, device="cuda")
        L.check(lib.vispec_prefill_attention_varlen_at(None, stream(), p(q), ldq, segs_at(row0, lens, pos0, ks, vs), n, S, H, Hkv, p(out), ldo, eager))
        owned = torch.zeros(total, dtype=torch.bool, device="cuda")
        for i in range(n):
            want = torch.full((lens[i], ldo), CANARY, dtype=torch.bfloat16, device="cuda")
            L.check(lib.vispec_prefill_attention_at(None, stream(), p(q[row0[i]:]), ldq, p(ks[i]), p(vs[i]), S, H, Hkv, pos0[i], lens[i], p(want), ldo,
                                                    eager))
            torch.cuda.synchronize()
            assert not (want == CANARY).all(dim=1).any()
            assert torch.equal(i16(out[row0[i]:row0[i] + lens[i]]), i16(want)), f"segment {i} of {seg_list}"
            owned[row0[i]:row0[i] + lens[i]] = True
        assert (out[~owned] == CANARY).all()


# ------------------------------------------------------------------------------------------------------ 4. rotary + KV append at an offset
@pytest.mark.parametrize("source", ["shared", "per_request"])
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_offset_rope_append_is_the_single_entry_on_the_whole_sequence(H, Hkv, source):
    """For every (pos0, M) edge: rotated q rows and cache rows [pos0, pos0 + M) == what vispec_rope_append writes for those rows of the
    whole sequence, bit for bit; cache rows outside keep their canary.  Both rotary sources: one shared table indexed by the position, and a
    table of the call's own rows (M-RoPE style: distinct contents per row, table row = global row of the call).  Then the same through one
    call with three segments of three sequences and a padded row0."""
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(31 + H)
    NH = H + 2 * Hkv
    Lmax = max(a + b for a, b in EDGES)
    S = Lmax + 70
    qkv0 = rand_bf16(gen, Lmax, NH * 128)
    cos, sin = rand_bf16(gen, S, 128), rand_bf16(gen, S, 128)  # row m = the rotary of position m (either source)
    want_q = qkv0.clone()
    want_k = torch.full((Hkv, S, 128), CANARY, dtype=torch.bfloat16, device="cuda")
    want_v = torch.full((Hkv, S, 128), CANARY, dtype=torch.bfloat16, device="cuda")
    L.check(lib.vispec_rope_append(None, stream(), p(want_q), Lmax, H, Hkv, 128, p(cos), p(sin), None, None, p(want_k), p(want_v), S, None))
    torch.cuda.synchronize()
    assert not (want_k[:, :Lmax] == CANARY).all(dim=2).any()

    def run(segments, pad):
        """segments = [(pos0, M)], each on a cache of its own: rows [pos0, pos0 + M) of the sequence, packed with `pad` rows between"""
        pos0, lens = [s[0] for s in segments], [s[1] for s in segments]
        n = len(lens)
        row0, total = packed_row0(lens, pad)
        qkv = rand_bf16(gen, total, NH * 128)
        for i in range(n):
            qkv[row0[i]:row0[i] + lens[i]] = qkv0[pos0[i]:pos0[i] + lens[i]]
        before = qkv.clone()
        ks = [torch.full((Hkv, S, 128), CANARY, dtype=torch.bfloat16, device="cuda") for _ in range(n)]
        vs = [torch.full((Hkv, S, 128), CANARY, dtype=torch.bfloat16, device="cuda") for _ in range(n)]
        if source == "shared":
            tc, ts, table_global = cos, sin, 0
        else:  # a table that covers exactly the call's rows
            tc, ts = rand_bf16(gen, total, 128), rand_bf16(gen, total, 128)
            for i in range(n):
                tc[row0[i]:row0[i] + lens[i]] = cos[pos0[i]:pos0[i] + lens[i]]
                ts[row0[i]:row0[i] + lens[i]] = sin[pos0[i]:pos0[i] + lens[i]]
            table_global = 1
        L.check(lib.vispec_rope_append_varlen_at(None, stream(), p(qkv), H, Hkv, 128, p(tc), p(ts), table_global, segs_at(row0, lens, pos0, ks, vs), n, S))
        torch.cuda.synchronize()
        owned = torch.zeros(total, dtype=torch.bool, device="cuda")
        for i in range(n):
            lo, hi = pos0[i], pos0[i] + lens[i]
            assert torch.equal(i16(qkv[row0[i]:row0[i] + lens[i]]), i16(want_q[lo:hi])), f"q|k|v rows of {segments[i]}"
            assert torch.equal(i16(ks[i][:, lo:hi]), i16(want_k[:, lo:hi])) and torch.equal(i16(vs[i][:, lo:hi]), i16(want_v[:, lo:hi])), segments[i]
            for cache in (ks[i], vs[i]):
                assert (cache[:, :lo] == CANARY).all() and (cache[:, hi:] == CANARY).all()
            owned[row0[i]:row0[i] + lens[i]] = True
        assert torch.equal(i16(qkv[~owned]), i16(before[~owned]))

    for edge in EDGES:
        run([edge], 0)
    run([(96, 64), (0, 129), (200, 300)], 3)


# --------------------------------------------------------------------------------------------------------------------------- 5. refusals
def test_offset_entries_refuse_bad_arguments():
    """pos0 < 0, pos0 + len > s_max, n_seq outside 1..8, null pointers, overlapping or descending row0, more than 1536 row blocks: non-zero,
    the message names the entry, and nothing is launched (q|k|v rows, caches and the out buffer keep their content)."""
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(6)
    S, H = 256, 2
    ldq, ldo = 3 * H * 128, H * 128
    q = rand_bf16(gen, 64, ldq)
    q0 = q.clone()
    out = torch.full((64, ldo), CANARY, dtype=torch.bfloat16, device="cuda")
    kc, vc = rand_bf16(gen, H, S, 128), rand_bf16(gen, H, S, 128)
    kc0, vc0 = kc.clone(), vc.clone()
    cos, sin = rand_bf16(gen, S, 128), rand_bf16(gen, S, 128)

    def att_v(segs, n, s_max=S, q_=q, out_=out):
        return lib.vispec_prefill_attention_varlen_at(None, stream(), None if q_ is None else p(q_), ldq, segs, n, s_max, H, H, None if out_ is None else p(out_),
                                                      ldo, 1), "prefill_attention_varlen_at"

    def rope_v(segs, n, s_max=S, q_=q, cos_=cos):
        return lib.vispec_rope_append_varlen_at(None, stream(), None if q_ is None else p(q_), H, H, 128, None if cos_ is None else p(cos_), p(sin), 0, segs, n,
                                                s_max), "rope_append_varlen_at"

    def att_1(pos0, M, k_=kc, q_=q, out_=out):
        return lib.vispec_prefill_attention_at(None, stream(), None if q_ is None else p(q_), ldq, None if k_ is None else p(k_), p(vc), S, H, H, pos0, M,
                                               None if out_ is None else p(out_), ldo, 1), "prefill_attention_at"

    def refused(call, word=None):
        rc, name = call
        assert rc != 0, name
        assert name + ":" in err(lib) and (word is None or word in err(lib)), err(lib)

    one = lambda row0, ln, pos0: segs_at([row0], [ln], [pos0], [kc], [vc])
    nine = segs_at([4 * i for i in range(9)], [4] * 9, [0] * 9, [kc] * 9, [vc] * 9)
    null_cache = (L.PrefillSegAt * 1)(L.PrefillSegAt(0, 4, 0, 0, None, vc.data_ptr()))
    for fn in (att_v, rope_v):
        refused(fn(one(0, 4, -1), 1), "pos0")
        refused(fn(one(0, 4, S - 3), 1), "pos0 + len")
        refused(fn(one(0, S + 1, 0), 1))
        refused(fn(one(0, 0, 0), 1))
        for n_seq in (0, 9):
            refused(fn(nine, n_seq), "n_seq")
        refused(fn(None, 1), "null")
        refused(fn(null_cache, 1), "null")
        refused(fn(one(0, 4, 0), 1, q_=None))
        refused(fn(segs_at([0, 8], [16, 16], [0, 0], [kc] * 2, [vc] * 2), 2), "ascending")   # overlapping
        refused(fn(segs_at([32, 0], [16, 16], [0, 0], [kc] * 2, [vc] * 2), 2), "ascending")  # descending
    refused(att_v(one(0, 4, 0), 1, out_=None), "null")
    refused(rope_v(one(0, 4, 0), 1, cos_=None))
    # 8 x 24 704 rows = 1544 row blocks of 128 (refused before anything is read: the buffers need not hold that many rows)
    big = 193 * 128
    refused(att_v(segs_at([big * i for i in range(8)], [big] * 8, [0] * 8, [kc] * 8, [vc] * 8), 8, s_max=1 << 20), "1536")
    refused(att_1(-1, 4), "pos0")
    refused(att_1(S - 3, 4), "pos0 + len")
    refused(att_1(0, 0))
    refused(att_1(0, 4, k_=None), "null")
    refused(att_1(0, 4, q_=None), "null")
    refused(att_1(0, 4, out_=None), "null")
    torch.cuda.synchronize()
    assert (out == CANARY).all() and torch.equal(q, q0) and torch.equal(kc, kc0) and torch.equal(vc, vc0)


# ------------------------------------------------------------------------------------------------------------------------ 6. model level
def oracle_prefill(ot, emb, pos3, NL, Hkv, max_pos, hd):
    pkv, pkv_data, cur = vo.initialize_past_key_values(NL, Hkv, max_pos, hd)
    lg, hid = ot.forward(pkv, inputs_embeds=emb, position_ids=pos3) if pos3 is not None else ot.forward(pkv, inputs_embeds=emb)
    return lg[-1], hid, pkv_data[0][:, 0, :, :emb.shape[0]].copy()


def check_prefill(eng, logits, hidden, ref):
    lg, hid, kv = ref
    Ln = hid.shape[0]
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (1, lg.shape[-1])
    assert hidden.dtype == torch.bfloat16 and tuple(hidden.shape) == tuple(hid.shape) and hidden.is_contiguous()
    close(hidden.float().cpu().numpy(), hid)
    close(eng.target_kv.float().cpu().numpy()[:, 0, :, :Ln], kv)
    close(logits.float().cpu().numpy()[0], lg)
    assert (eng.target_kv[:, :, :, Ln:] == CANARY).all()  # no row past the prompt was written


@pytest.fixture(scope="module")
def llava_model():
    """Tiny LLaVA with a 300-row prompt (an image run of 200 rows) and the oracle's prefill of it."""
    sm, ot, od = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    emb = embeds_of(ot, *llava_prompt(np.random.default_rng(700), 40, 200, 60), IMG_TOK)
    return sm, ot, emb, None, oracle_prefill(ot, emb, None, T["NL"], T["H"], T["max_pos"], T["D"] // T["H"])


@pytest.fixture(scope="module")
def qwen_model():
    """Tiny Qwen2.5-VL (GQA 4/2, q/k/v bias, SDPA-class scores, M-RoPE) with a 291-row prompt of two image runs."""
    sm, ot, od, IMG = build_qwen()
    Q = synth.QWEN_TINY
    ids, feats, grids = qwen_prompt(np.random.default_rng(701), IMG, Q["D"], [(60, (1, 20, 24)), (70, (1, 12, 12))])
    emb, pos3 = embeds_of(ot, ids, feats, IMG), synth.qwen_rope_index(ids, IMG, grids)[0]
    return sm, ot, emb, pos3, oracle_prefill(ot, emb, pos3, Q["NL"], Q["Hkv"], Q["max_pos"], Q["D"] // Q["H"])


@pytest.mark.parametrize("which", ["llava", "qwen"])
def test_chunked_prefill_matches_the_oracle(which, request):
    """chunk_rows in {37, 128, 129}: K/V rows of every layer, hidden rows and the last row's logits within the bar of the single-request
    comparisons; chunk_rows >= L is the unchunked call, byte for byte; and a chunked prefill equals, as an array, the same pieces issued by
    hand: prefill(first C rows) followed by prefill(next rows, past_len=...) (same kernels, same GEMM shapes)."""
    sm, ot, emb, pos3, ref = request.getfixturevalue(which + "_model")
    eng, base = sm.engine, sm.base_model
    x = t_bf16(emb)
    Ln = x.shape[0]
    pz = None if pos3 is None else torch.from_numpy(pos3)
    eng.target_kv.fill_(CANARY)
    lg0, hid0 = base.prefill(x, position_ids=pz)
    kv0 = eng.target_kv.clone()
    for big in (Ln, Ln + 1, 4096):
        eng.target_kv.fill_(CANARY)
        lg, hid = base.prefill(x, position_ids=pz, chunk_rows=big)
        assert torch.equal(lg, lg0) and torch.equal(hid, hid0) and torch.equal(eng.target_kv, kv0)
    for chunk in (37, 128, 129):
        eng.target_kv.fill_(CANARY)
        lg, hid = base.prefill(x, position_ids=pz, chunk_rows=chunk)
        torch.cuda.synchronize()
        check_prefill(eng, lg, hid, ref)
        kv = eng.target_kv.clone()
        lg_all, hid_all = base.prefill(x, all_logits=True, position_ids=pz, chunk_rows=chunk)
        assert tuple(lg_all.shape) == (Ln, ref[0].shape[-1]) and lg_all.dtype == torch.float32 and torch.equal(hid_all, hid)
        close(lg_all[-1].cpu().numpy(), lg[0].cpu().numpy())  # (the lm_head GEMM at M = the last piece's rows against M = 1)
        eng.target_kv.fill_(CANARY)
        hs = []
        for lo in range(0, Ln, chunk):  # the same pieces by hand; the first one is the unchunked call on `chunk` rows
            hi = min(Ln, lo + chunk)
            lg_p, h_p = base.prefill(x[lo:hi], position_ids=None if pz is None else pz[:, lo:hi], past_len=lo)
            assert tuple(h_p.shape) == (hi - lo, x.shape[1]) and tuple(lg_p.shape) == (1, ref[0].shape[-1])
            hs.append(h_p)
        assert torch.equal(torch.cat(hs), hid) and torch.equal(lg_p, lg) and torch.equal(eng.target_kv, kv)


def test_chunked_prefill_refusals(llava_model, monkeypatch):
    sm, ot, emb, _, _ = llava_model
    eng, base = sm.engine, sm.base_model
    x = t_bf16(emb)
    eng.target_kv.fill_(CANARY)
    with pytest.raises(L.VispecError, match="does not fit"):  # past_len + L rows against the cache, before any row is written
        base.prefill(x, past_len=T["max_pos"] - x.shape[0])
    for bad in (dict(chunk_rows=0), dict(chunk_rows=-3), dict(past_len=-1)):
        with pytest.raises(ValueError):
            base.prefill(x, **bad)
    with pytest.raises(ValueError):
        base.prefill_batch([eng], [x], chunk_rows=0)
    torch.cuda.synchronize()
    assert (eng.target_kv == CANARY).all()
    with monkeypatch.context() as mp:  # other head sizes are served by the unchunked SDPA path only
        mp.setattr(type(base.cfg), "head_dim", property(lambda self: 64))
        with pytest.raises(L.VispecError, match="head_dim"):
            base.prefill(x, chunk_rows=64)
    assert (eng.target_kv == CANARY).all()


@pytest.mark.parametrize("chunk", [37, 128, 129])
def test_chunked_prefill_batch_matches_the_oracle_qwen(qwen_model, chunk):
    """Three prompts on one chunked walk — M-RoPE prompts and a text-only one among them (its rows use the plain table) — cut at chunk
    boundaries that fall inside prompts: every request within the oracle's bar."""
    sm, ot, emb_a, pos_a, ref_a = qwen_model
    Q = synth.QWEN_TINY
    IMG = Q["V"] - 1
    models = [sm] + [sm.make_cohort_member() for _ in range(2)]
    engines = [m.engine for m in models]
    rng = np.random.default_rng(702)
    ids_b = rng.integers(3, IMG, 61).astype(np.int64)  # text only
    emb_b = embeds_of(ot, ids_b, np.zeros((0, Q["D"]), np.float32), IMG)
    ids_c, feats_c, grids_c = qwen_prompt(rng, IMG, Q["D"], [(9, (1, 8, 12)), (30, (1, 4, 4))])
    emb_c, pos_c = embeds_of(ot, ids_c, feats_c, IMG), synth.qwen_rope_index(ids_c, IMG, grids_c)[0]
    args = (Q["NL"], Q["Hkv"], Q["max_pos"], Q["D"] // Q["H"])
    refs = [oracle_prefill(ot, emb_b, None, *args), ref_a, oracle_prefill(ot, emb_c, pos_c, *args)]
    for e in engines:
        e.target_kv.fill_(CANARY)
    res = sm.base_model.prefill_batch(engines, [t_bf16(emb_b), t_bf16(emb_a), t_bf16(emb_c)], [None, torch.from_numpy(pos_a), torch.from_numpy(pos_c)],
                                      chunk_rows=chunk)
    torch.cuda.synchronize()
    for e, (lg, hid), ref in zip(engines, res, refs):
        check_prefill(e, lg, hid, ref)


def test_a_request_does_not_depend_on_what_shares_its_pieces():
    """The same prompt in two chunked batches of the same total row count but other companions (other lengths, other contents): identical
    K/V rows, hidden rows and logits, bit for bit — and the oracle's within the bar, with the shared table (LLaVA)."""
    sm, ot, od = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    models = [sm] + [sm.make_cohort_member() for _ in range(2)]
    engines = [m.engine for m in models]
    rng = np.random.default_rng(556)
    a = embeds_of(ot, *llava_prompt(rng, 7, 90, 20), IMG_TOK)                 # 117 rows
    b1, c1 = embeds_of(ot, *llava_prompt(rng, 3, 50, 7), IMG_TOK), embeds_of(ot, *llava_prompt(rng, 10, 100, 30), IMG_TOK)  # 60 + 140
    b2, c2 = embeds_of(ot, *llava_prompt(rng, 30, 99, 4), IMG_TOK), embeds_of(ot, *llava_prompt(rng, 1, 60, 6), IMG_TOK)    # 133 + 67
    args = (T["NL"], T["H"], T["max_pos"], T["D"] // T["H"])
    for e in engines:
        e.target_kv.fill_(CANARY)
    r1 = sm.base_model.prefill_batch(engines, [t_bf16(a), t_bf16(b1), t_bf16(c1)], chunk_rows=100)
    kv1 = engines[0].target_kv[:, :, :, :a.shape[0]].clone()
    for e, (lg, hid), emb in zip(engines, r1, (a, b1, c1)):
        check_prefill(e, lg, hid, oracle_prefill(ot, emb, None, *args))
    r2 = sm.base_model.prefill_batch(engines, [t_bf16(a), t_bf16(b2), t_bf16(c2)], chunk_rows=100)
    kv2 = engines[0].target_kv[:, :, :, :a.shape[0]].clone()
    assert torch.equal(kv1, kv2) and torch.equal(r1[0][1], r2[0][1]) and torch.equal(r1[0][0], r2[0][0])


# ------------------------------------------------------------------------------------------------------------------------ 7. peak memory
def test_chunking_bounds_the_prefill_workspace(llava_model):
    """The longest prompt the tiny model's cache takes: the peak of allocated memory above the resident baseline is strictly lower with
    chunk_rows = L / 8 than unchunked (no ratio is fixed here: the full-size figures come from tools/prefill_chunk_bench.py)."""
    sm = llava_model[0]
    eng, base = sm.engine, sm.base_model
    Ln = (eng.kv_max_pos - eng.total_token - 8) // 8 * 8
    x = (torch.randn(Ln, T["D"], generator=torch.Generator(device="cuda").manual_seed(8), device="cuda") * 0.05).to(torch.bfloat16)

    def peak(**kw):
        base.prefill(x, **kw)  # (allocator and library warm-up of this shape)
        torch.cuda.synchronize()
        gc.collect()  # cyclic garbage of earlier tests (closed models and their caches) freed DURING the measured call would lower its peak
        torch.cuda.reset_peak_memory_stats()
        floor = torch.cuda.memory_allocated()
        out = base.prefill(x, **kw)
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated() - floor

    whole, chunked = peak(), peak(chunk_rows=Ln // 8)
    print(f"prefill of {Ln} rows: peak above baseline {whole} B unchunked, {chunked} B with chunk_rows = {Ln // 8}")
    assert chunked < whole


# -------------------------------------------------------------------------------------------------------------------------- 8. loop level
@pytest.fixture(scope="module")
def tiny_cohort8():
    sm, ot, od = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    return [sm] + [sm.make_cohort_member() for _ in range(7)]


def equals_greedy_ar(model, reqs, budgets, got):
    for t, ((ids, kw), (toks, new_token, idx, acc)) in enumerate(zip(reqs, got)):
        ar = model.baseline_generate(ids, max_new_tokens=budgets[t], max_steps=budgets[t] + 1, **kw)
        m = min(ar.shape[1], toks.shape[1])
        assert m >= min(ids.shape[1] + budgets[t], toks.shape[1])
        np.testing.assert_array_equal(ar[0, :m].cpu().numpy(), toks[0, :m].cpu().numpy(), err_msg=f"request {t} vs greedy AR")


def test_loops_with_a_chunked_prefill_return_the_unchunked_tuples(tiny_cohort8):
    """specgenerate, specgenerate_cohort (batched start, 2 and 8 requests) and specgenerate_stream (more requests than slots) with
    prefill_chunk_rows: the tuples of the unchunked call and the tokens of greedy AR; one sampling case with equal seeds.
    These equalities rest on the logit margins of the synthetic structured weights, as in the existing cohort tests (a chunked prefill may
    sum its GEMMs in another fp32 order): the invariant is the oracle bar of test_chunked_prefill_matches_the_oracle."""
    models = tiny_cohort8
    sm = models[0]
    reqs = tiny_requests(np.random.default_rng(95), 8)  # 37 .. 257 rows
    budgets = [20, 14, 17, 12, 20, 15, 19, 16]
    ids, kw = reqs[7]  # 257 rows, an image run of 200
    want = sm.specgenerate(ids, max_new_tokens=20, log=True, return_acceptance_len=True, **kw)
    got = sm.specgenerate(ids, max_new_tokens=20, log=True, return_acceptance_len=True, prefill_chunk_rows=64, **kw)
    same_tuples([got], [want])
    equals_greedy_ar(sm, [reqs[7]], [20], [got])
    for n in (2, 8):
        sub = reqs[8 - n:]
        want = specgenerate_cohort(models[:n], sub, max_new_tokens=budgets[:n])
        got = specgenerate_cohort(models[:n], sub, max_new_tokens=budgets[:n], batch_prefill=True, prefill_chunk_rows=100)
        same_tuples(got, want)
        equals_greedy_ar(sm, sub, budgets[:n], got)
    got = specgenerate_cohort(models[:2], reqs[6:], max_new_tokens=budgets[:2], prefill_chunk_rows=100)  # per-request starts, chunked
    same_tuples(got, specgenerate_cohort(models[:2], reqs[6:], max_new_tokens=budgets[:2]))
    slots = models[:3]
    want = specgenerate_stream(slots, reqs[1:], max_new_tokens=budgets[1:])
    for bp in (False, True):
        got = specgenerate_stream(slots, reqs[1:], max_new_tokens=budgets[1:], batch_prefill=bp, prefill_chunk_rows=100)
        same_tuples(got, want)
    equals_greedy_ar(sm, reqs[1:], budgets[1:], got)
    gen = dict(temperature=1.0, top_k=4, seeds=[3, 4, 5], max_new_tokens=16)
    same_tuples(specgenerate_cohort(slots, reqs[5:], batch_prefill=True, prefill_chunk_rows=100, **gen), specgenerate_cohort(slots, reqs[5:], **gen))
