"""A shared prompt prefix: the K/V row copy kernel (vispec_kv_copy_rows) against torch slicing bit for bit, SpecModel.prefill_prefix and
requests on a PromptPrefix (specgenerate / specgenerate_cohort / specgenerate_stream with prefix=) on the tiny models.

Arithmetic class that these tests pin down: the prefix rows of every cache are the donor prefill's bytes; the new rows run the offset
kernels and library GEMMs at M = the new rows.  A request on a prefix therefore equals, bit for bit, the two-piece chunked prefill
specgenerate(prefill_chunk_rows=P) when P >= L / 2 (the same pieces, GEMM shapes and kernels), and is held to the oracle's bf16 forward
within the bar of the single-request prefill comparisons (2^-6 of the tensor's largest magnitude, as tests/test_prefill_chunk_gpu.py)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from helpers import T, synth, vo  # noqa: E402
from test_loop_gpu import IMG_TOK, build, build_qwen  # noqa: E402  (the tiny-model builders)
from vispec_amd import lib as L  # noqa: E402
from vispec_amd.model import PromptPrefix  # noqa: E402
from vispec_amd.model.spec_model_ours import specgenerate_cohort, specgenerate_stream  # noqa: E402

CANARY = -1536.0  # exact in bf16
i16 = lambda t: t.view(torch.int16)
p = lambda t: C.c_void_p(t.data_ptr())
err = lambda lib: (lib.vispec_last_error() or b"").decode()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def close(got, want, frac=2.0 ** -6):
    """The bar of the single-request prefill comparisons: 2^-6 of the reference tensor's largest magnitude."""
    np.testing.assert_allclose(np.asarray(got, np.float32), want, rtol=0, atol=frac * float(np.abs(want).max()))


def t_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).cuda()


def rand_bf16(gen, *shape):
    return torch.randn(*shape, generator=gen, device="cuda").to(torch.bfloat16)


def same_tuples(got, want):
    for t, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[0], w[0]) and (g[1], g[2], g[3]) == (w[1], w[2], w[3]), f"request {t}"


def ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


# ---------------------------------------------------------------------------------------------------------------------- 1. the copy kernel
HD = 128
ROWS = (1, 2, 127, 128, 129, 300)


def copy_rows(lib, src, dsts, rows):
    planes, src_smax = src.shape[0], src.shape[1]
    return lib.vispec_kv_copy_rows(None, stream(), p(src), src_smax, ptrs(dsts), len(dsts), dsts[0].shape[1], planes, rows, HD)


@pytest.mark.parametrize("n_dst", [1, 2, 8])
@pytest.mark.parametrize("planes", [8, 64])
def test_copy_rows_equals_torch_slicing_bit_for_bit(planes, n_dst):
    """rows in {1, 2, 127, 128, 129, 300} x src_smax in {rows, 512} x dst_smax in {rows, 384, 512}: rows [0, rows) of every plane of every
    destination are the source's bit patterns, rows >= `rows` keep their sentinel, the source is unchanged."""
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(planes + n_dst)
    for rows in ROWS:
        for src_smax in (rows, 512):
            src = rand_bf16(gen, planes, src_smax, HD)
            src0 = src.clone()
            for dst_smax in (rows, 384, 512):
                dsts = [torch.full((planes, dst_smax, HD), CANARY - d, dtype=torch.bfloat16, device="cuda") for d in range(n_dst)]
                L.check(copy_rows(lib, src, dsts, rows))
                torch.cuda.synchronize()
                for d, dst in enumerate(dsts):
                    assert torch.equal(i16(dst[:, :rows]), i16(src0[:, :rows])), (rows, src_smax, dst_smax, d)
                    assert (dst[:, rows:] == CANARY - d).all(), (rows, src_smax, dst_smax, d)
                assert torch.equal(i16(src), i16(src0))


def test_copy_rows_round_trip_cache_store_cache():
    """cache -> compact store -> another cache (both directions of Engine.save_kv_rows / load_kv_rows): the rows arrive unchanged."""
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(3)
    planes, S, rows = 8, 512, 211
    cache_a = rand_bf16(gen, planes, S, HD)
    store = torch.full((planes, rows, HD), CANARY, dtype=torch.bfloat16, device="cuda")
    cache_b = torch.full((planes, S, HD), CANARY, dtype=torch.bfloat16, device="cuda")
    L.check(copy_rows(lib, cache_a, [store], rows))
    L.check(copy_rows(lib, store, [cache_b], rows))
    torch.cuda.synchronize()
    assert torch.equal(i16(store), i16(cache_a[:, :rows])) and torch.equal(i16(cache_b[:, :rows]), i16(cache_a[:, :rows]))
    assert (cache_b[:, rows:] == CANARY).all()


def test_copy_rows_refusals_write_nothing():
    """n_dst outside 1..8, rows < 1 / > src_smax / > dst_smax, planes < 1, head_dim * 2 bytes not a multiple of 16, a null pointer, a
    destination equal to the source: non-zero, the message names the entry, nothing is enqueued."""
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(4)
    planes, S = 8, 64
    src = rand_bf16(gen, planes, S, HD)
    src0 = src.clone()
    dsts = [torch.full((planes, S, HD), CANARY, dtype=torch.bfloat16, device="cuda") for _ in range(9)]
    st, P_ = stream(), ptrs

    def call(src_=src, src_smax=S, dp=None, n_dst=1, dst_smax=S, planes_=planes, rows=4, hd=HD):
        return lib.vispec_kv_copy_rows(None, st, None if src_ is None else p(src_), src_smax, P_(dsts) if dp is None else dp, n_dst, dst_smax, planes_, rows, hd)

    null_dst = (C.c_void_p * 2)(dsts[0].data_ptr(), None)
    self_dst = (C.c_void_p * 2)(dsts[0].data_ptr(), src.data_ptr())
    bad = [dict(n_dst=0), dict(n_dst=9), dict(n_dst=-1), dict(rows=0), dict(rows=-5), dict(rows=S + 1), dict(rows=40, dst_smax=39), dict(rows=40, src_smax=39),
           dict(planes_=0), dict(planes_=-2), dict(hd=4), dict(hd=12), dict(src_=None), dict(dp=null_dst, n_dst=2), dict(dp=self_dst, n_dst=2)]
    for kw in bad:
        assert call(**kw) != 0, kw
        assert "kv_copy_rows:" in err(lib), (kw, err(lib))
    assert lib.vispec_kv_copy_rows(None, st, p(src), S, None, 1, S, planes, 4, HD) != 0 and "null" in err(lib)
    torch.cuda.synchronize()
    assert torch.equal(i16(src), i16(src0)) and all((d == CANARY).all() for d in dsts)
    assert call(n_dst=8) == 0  # (and the same table is served once its arguments are in range)
    torch.cuda.synchronize()
    assert all(torch.equal(i16(d[:, :4]), i16(src0[:, :4])) and (d[:, 4:] == CANARY).all() for d in dsts[:8]) and (dsts[8] == CANARY).all()
    assert lib.vispec_version() == 4


# ------------------------------------------------------------------------------------------------------------------- 2. tiny LLaVA, one request
P_ROWS, N_PRE, N_IMG = 200, 40, 150  # the prefix: 40 text rows, an image run of 150, 10 text rows
SUFFIX = (100, 1, 5, 33, 2, 17, 64, 77)  # new rows per request (all distinct); request 0: L = 300, P >= L / 2


def oracle_prefill(ot, emb, pos3, NL, Hkv, max_pos, hd):
    pkv, pkv_data, cur = vo.initialize_past_key_values(NL, Hkv, max_pos, hd)
    lg, hid = ot.forward(pkv, inputs_embeds=emb, position_ids=pos3) if pos3 is not None else ot.forward(pkv, inputs_embeds=emb)
    return lg[-1], hid, pkv_data[0][:, 0, :, :emb.shape[0]].copy()


@pytest.fixture(scope="module")
def llava():
    """Tiny LLaVA cohort of eight, one prefix of 200 rows (image run inside) and eight prompts that begin with it."""
    sm, ot, od = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    models = [sm] + [sm.make_cohort_member() for _ in range(7)]
    rng = np.random.default_rng(811)
    pre = np.concatenate([rng.integers(3, IMG_TOK, N_PRE), np.full(N_IMG, IMG_TOK), rng.integers(3, IMG_TOK, P_ROWS - N_PRE - N_IMG)]).astype(np.int64)
    feats = t_bf16(synth.bf16_grid(rng.standard_normal((N_IMG, T["D"]), dtype=np.float32) * 0.05))
    ids = [torch.from_numpy(np.concatenate([pre, rng.integers(3, IMG_TOK, n)]).astype(np.int64))[None] for n in SUFFIX]
    pfx = sm.prefill_prefix(ids[0][:, :P_ROWS], pixel_values=feats)
    return SimpleNamespace(models=models, ot=ot, od=od, ids=ids, feats=feats, pfx=pfx, budgets=[16, 12, 14, 20, 13, 18, 15, 17], solo={})


def solo(env, i):
    """Request i alone on the leader: specgenerate(prefix=) — computed once, shared, never modified."""
    if i not in env.solo:
        env.solo[i] = env.models[0].specgenerate(env.ids[i], max_new_tokens=env.budgets[i], log=True, return_acceptance_len=True, prefix=env.pfx)
    return env.solo[i]


def started(model, ids, kw, **how):
    """One request start on a sentinel-filled cache: -> (hidden, draft embeddings, mask, first token, K/V cache) as the draft prefill saw them."""
    model.engine.target_kv.fill_(CANARY)
    hidden, demb, mask, first = model._start_request(ids, None, dict(kw), max_new_tokens=16, **how)
    torch.cuda.synchronize()
    return hidden.clone(), demb.clone(), mask, first.clone(), model.engine.target_kv.clone()


def same_start(a, b, Ln):
    assert torch.equal(i16(a[4]), i16(b[4])), "K/V rows of every layer (and the sentinel behind them)"
    assert not (a[4][:, :, :, :Ln] == CANARY).all(dim=-1).any() and (a[4][:, :, :, Ln:] == CANARY).all()
    assert tuple(a[0].shape) == tuple(b[0].shape) and torch.equal(i16(a[0]), i16(b[0])), "the hidden handed to the draft prefill"
    assert torch.equal(i16(a[1]), i16(b[1])) and np.array_equal(a[2], b[2]) and torch.equal(a[3], b[3]), "draft embeddings, mask, first token"


def test_prefix_object(llava):
    pfx, sm = llava.pfx, llava.models[0]
    NL2, Hk, hd = 2 * T["NL"], T["H"], T["D"] // T["H"]
    assert isinstance(pfx, PromptPrefix) and pfx.rows == P_ROWS and pfx.weights is sm.base_model.w
    assert tuple(pfx.store.shape) == (NL2, Hk, P_ROWS, hd) and tuple(pfx.hidden.shape) == tuple(pfx.emb.shape) == (P_ROWS, T["D"])
    assert pfx.nbytes >= pfx.store.numel() * 2 + 2 * P_ROWS * T["D"] * 2
    assert int(pfx.image_mask.sum()) == N_IMG and torch.equal(pfx.ids, llava.ids[0][:, :P_ROWS])
    kv = sm.engine.target_kv
    lo, hi = pfx.store.data_ptr(), pfx.store.data_ptr() + pfx.store.numel() * 2
    assert hi <= kv.data_ptr() or lo >= kv.data_ptr() + kv.numel() * 2, "the store aliases no cache"
    # save / load are each other's inverse on the engine's own cache shape
    sm.engine.target_kv.fill_(CANARY)
    sm.engine.load_kv_rows(pfx.store, [sm.engine])
    again = sm.engine.save_kv_rows(P_ROWS)
    torch.cuda.synchronize()
    assert torch.equal(i16(again), i16(pfx.store)) and (sm.engine.target_kv[:, :, :, P_ROWS:] == CANARY).all()
    with pytest.raises(ValueError):
        sm.engine.load_kv_rows(pfx.store, [])
    with pytest.raises(ValueError):
        sm.engine.load_kv_rows(pfx.store[:, :1], [sm.engine])
    with pytest.raises(L.VispecError):
        sm.engine.save_kv_rows(T["max_pos"] + 1)


def test_request_on_a_prefix_equals_the_two_piece_chunked_start(llava):
    """specgenerate(ids, prefix=pfx) against specgenerate(ids, prefill_chunk_rows=P): K/V rows, the hidden handed to the draft prefill, the
    first token, then the whole token stream and acceptance lengths — bit-equal; on the slot that computed the prefix, on a cohort
    member's cache, and after the computing slot has served an unrelated request in between (the store aliases no cache)."""
    sm, member = llava.models[0], llava.models[3]
    ids, kw = llava.ids[0], dict(pixel_values=llava.feats)
    Ln = ids.shape[1]
    assert Ln == 300 and P_ROWS >= Ln / 2
    want = started(sm, ids, kw, prefill_chunk_rows=P_ROWS)
    store0 = llava.pfx.store.clone()
    same_start(started(sm, ids, {}, prefix=llava.pfx), want, Ln)
    same_start(started(member, ids, {}, prefix=llava.pfx), want, Ln)
    gen = dict(max_new_tokens=20, log=True, return_acceptance_len=True)
    want_run = sm.specgenerate(ids, prefill_chunk_rows=P_ROWS, **gen, **kw)
    same_tuples([sm.specgenerate(ids, prefix=llava.pfx, **gen)], [want_run])
    same_tuples([member.specgenerate(ids, prefix=llava.pfx, **gen)], [want_run])
    other = torch.from_numpy(np.random.default_rng(5).integers(3, IMG_TOK, 260))[None]  # an unrelated request overwrites the slot's rows
    sm.specgenerate(other, max_new_tokens=8)
    assert torch.equal(i16(llava.pfx.store), i16(store0))
    same_start(started(sm, ids, {}, prefix=llava.pfx), want, Ln)
    same_tuples([sm.specgenerate(ids, prefix=llava.pfx, **gen)], [want_run])
    same_tuples([solo(llava, 0)], [sm.specgenerate(ids, prefill_chunk_rows=P_ROWS, max_new_tokens=llava.budgets[0], log=True, return_acceptance_len=True, **kw)])


def test_request_on_a_prefix_against_the_oracle(llava):
    """Fork + prefill(new rows, past_len=P): hidden rows, K/V rows and the last row's logits within the oracle bars; and bit-identical to
    prefill(x[:P]) followed by prefill(x[P:], past_len=P) on one cache.  prefill_prefix(prefill_chunk_rows=) keeps the same class."""
    sm, pfx = llava.models[0], llava.pfx
    eng, base = sm.engine, sm.base_model
    for i in (0, 3):
        ids = llava.ids[i]
        Ln = ids.shape[1]
        full = sm._embed_prompt(ids, None, dict(pixel_values=llava.feats))[1]
        ref = oracle_prefill(llava.ot, full.float().cpu().numpy(), None, T["NL"], T["H"], T["max_pos"], T["D"] // T["H"])
        emb = sm._embed_on_prefix(ids, pfx)[1]
        assert torch.equal(i16(emb), i16(full))
        eng.target_kv.fill_(CANARY)
        eng.load_kv_rows(pfx.store, [eng])
        lg, hid_new = base.prefill(emb[P_ROWS:], past_len=P_ROWS)
        torch.cuda.synchronize()
        hidden, kv = torch.cat([pfx.hidden, hid_new]), eng.target_kv.clone()
        close(hidden.float().cpu().numpy(), ref[1])
        close(kv.float().cpu().numpy()[:, 0, :, :Ln], ref[2])
        close(lg.float().cpu().numpy()[0], ref[0])
        assert (kv[:, :, :, Ln:] == CANARY).all()
        eng.target_kv.fill_(CANARY)
        _, h0 = base.prefill(emb[:P_ROWS])
        lg1, h1 = base.prefill(emb[P_ROWS:], past_len=P_ROWS)
        assert torch.equal(i16(torch.cat([h0, h1])), i16(hidden)) and torch.equal(lg1, lg) and torch.equal(i16(eng.target_kv), i16(kv))
    chunked = sm.prefill_prefix(llava.ids[0][:, :P_ROWS], prefill_chunk_rows=64, pixel_values=llava.feats)
    close(chunked.hidden.float().cpu().numpy(), ref[1][:P_ROWS])
    close(chunked.store.float().cpu().numpy(), ref[2][:, :, :P_ROWS])


def test_the_vision_front_end_does_not_run_on_a_prefixed_request(llava):
    sm, member = llava.models[0], llava.models[1]
    vision, calls = sm.base_model.vision, []
    assert member.base_model.vision is vision
    inner = vision.features
    vision.features = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    try:
        ids = llava.ids[2]
        pfx = sm.prefill_prefix(ids[:, :P_ROWS], pixel_values=(N_IMG, 7))
        assert len(calls) == 1
        a = sm.specgenerate(ids, max_new_tokens=10, log=True, return_acceptance_len=True, prefix=pfx)
        b = member.specgenerate(ids, max_new_tokens=10, log=True, return_acceptance_len=True, prefix=pfx, pixel_values=(N_IMG, 7))  # not read
        assert len(calls) == 1
        same_tuples([b], [a])
        sm.specgenerate(ids, max_new_tokens=10, pixel_values=(N_IMG, 7))
        assert len(calls) == 2
    finally:
        del vision.features


# ----------------------------------------------------------------------------------------------------------------------- 3. tiny Qwen, M-RoPE
def test_qwen_mrope_request_on_a_prefix():
    """GQA 4/2, q/k/v bias, M-RoPE tables: the same equalities against the two-piece chunked start, rope_delta of the full prompt, and the
    oracle bars on the new rows' positions [3, L - P]."""
    sm, ot, od, IMG = build_qwen()
    Q = synth.QWEN_TINY
    rng = np.random.default_rng(812)
    grids = [(1, 20, 24), (1, 8, 8)]
    pre = np.concatenate([rng.integers(3, IMG, 60), np.full(120, IMG), rng.integers(3, IMG, 20), np.full(16, IMG), rng.integers(3, IMG, 5)])
    P = len(pre)
    ids_np = np.concatenate([pre, rng.integers(3, IMG, 79)]).astype(np.int64)
    ids, Ln = torch.from_numpy(ids_np)[None], len(ids_np)
    assert Ln == 300 and P >= Ln / 2
    feats = t_bf16(synth.bf16_grid(rng.standard_normal((136, Q["D"]), dtype=np.float32) * 0.05))
    kw = dict(pixel_values=feats, image_grid_thw=torch.tensor(grids))
    pos3, delta = synth.qwen_rope_index(ids_np, IMG, grids)
    assert delta < 0
    pfx = sm.prefill_prefix(ids[:, :P], **kw)
    assert tuple(pfx.pos3.shape) == (3, P) and np.array_equal(pfx.pos3.numpy(), pos3[:, :P])
    member = sm.make_cohort_member()
    want = started(sm, ids, kw, prefill_chunk_rows=P)
    assert sm._rope_delta == delta
    sm._rope_delta = None
    same_start(started(sm, ids, {}, prefix=pfx), want, Ln)
    assert sm._rope_delta == delta
    same_start(started(member, ids, {}, prefix=pfx), want, Ln)
    assert member._rope_delta == delta
    gen = dict(max_new_tokens=20, log=True, return_acceptance_len=True)
    want_run = sm.specgenerate(ids, prefill_chunk_rows=P, **gen, **kw)
    same_tuples([sm.specgenerate(ids, prefix=pfx, **gen), member.specgenerate(ids, prefix=pfx, **gen)], [want_run, want_run])
    # the oracle bars
    full = sm._embed_prompt(ids, None, dict(kw))[1]
    ref = oracle_prefill(ot, full.float().cpu().numpy(), pos3, Q["NL"], Q["Hkv"], Q["max_pos"], Q["D"] // Q["H"])
    eng = sm.engine
    eng.target_kv.fill_(CANARY)
    eng.load_kv_rows(pfx.store, [eng])
    lg, hid_new = sm.base_model.prefill(full[P:], position_ids=torch.from_numpy(pos3[:, P:]), past_len=P)
    torch.cuda.synchronize()
    close(torch.cat([pfx.hidden, hid_new]).float().cpu().numpy(), ref[1])
    close(eng.target_kv.float().cpu().numpy()[:, 0, :, :Ln], ref[2])
    close(lg.float().cpu().numpy()[0], ref[0])
    # one walk with a text-only whole prompt next to it (past_lens = [P, 0], M-RoPE rows and plain-table rows): both within the bars
    text = t_bf16(ot.w["model.embed_tokens.weight"][rng.integers(3, IMG, 41)])
    for e in (eng, member.engine):
        e.target_kv.fill_(CANARY)
    eng.load_kv_rows(pfx.store, [eng])
    res = sm.base_model.prefill_batch([eng, member.engine], [full[P:], text], [torch.from_numpy(pos3[:, P:]), None], past_lens=[P, 0])
    torch.cuda.synchronize()
    close(torch.cat([pfx.hidden, res[0][1]]).float().cpu().numpy(), ref[1])
    close(res[0][0].float().cpu().numpy()[0], ref[0])
    ref_t = oracle_prefill(ot, text.float().cpu().numpy(), None, Q["NL"], Q["Hkv"], Q["max_pos"], Q["D"] // Q["H"])
    close(res[1][1].float().cpu().numpy(), ref_t[1])
    close(res[1][0].float().cpu().numpy()[0], ref_t[0])


# ------------------------------------------------------------------------------------------------------------------------------ 4. cohorts
@pytest.mark.parametrize("n", [4, 8])
def test_cohort_on_one_prefix(llava, n, monkeypatch):
    """n requests on one prefix, per-request suffix prefills: every tuple equals the request's solo specgenerate(prefix=) — bit-equal for
    n <= 4; for n = 8 the c8 class criteria of the existing cohort tests (the composition does not matter; on these confident models the
    c8 rounding changes no decision) — and exactly one copy launch serves the fork."""
    models, reqs = llava.models[:n], [(ids, {}) for ids in llava.ids[:n]]
    want = [solo(llava, i) for i in range(n)]
    lib, launches = models[0].engine.lib, []
    inner = lib.vispec_kv_copy_rows
    monkeypatch.setattr(lib, "vispec_kv_copy_rows", lambda *a: (launches.append(a[5]), inner(*a))[1])
    st = {}
    got = specgenerate_cohort(models, reqs, max_new_tokens=llava.budgets[:n], prefix=llava.pfx, stats=st)
    assert st["prefix_forks"] == [n] and launches == [n]
    monkeypatch.undo()
    same_tuples(got, want)
    if n > 4:
        rev = specgenerate_cohort(models, reqs[::-1], max_new_tokens=llava.budgets[:n][::-1], prefix=[llava.pfx] * n)[::-1]
        same_tuples(rev, got)
    st = {}
    specgenerate_cohort(models[:2], reqs[:2], max_new_tokens=4, stats=st)
    assert "prefix_forks" not in st


def test_cohort_batched_suffixes(llava):
    """batch_prefill=True: prefix rows of every cache equal the store bit for bit; new rows' hidden, K/V and logits within the oracle
    bars; a request's rows do not depend on its company in the batch; a list mixing a prefix with None."""
    models, pfx, sm = llava.models[:4], llava.pfx, llava.models[0]
    engines = [m.engine for m in models]
    base = sm.base_model
    args = (T["NL"], T["H"], T["max_pos"], T["D"] // T["H"])
    embs = [sm._embed_on_prefix(ids, pfx)[1] for ids in llava.ids]

    def batched(which):
        for e in engines[:len(which)]:
            e.target_kv.fill_(CANARY)
        sm.engine.load_kv_rows(pfx.store, engines[:len(which)])
        res = base.prefill_batch(engines[:len(which)], [embs[i][P_ROWS:] for i in which], None, past_lens=[P_ROWS] * len(which))
        torch.cuda.synchronize()
        return res

    which = [0, 1, 2, 3]
    res = batched(which)
    for e, i, (lg, hid) in zip(engines, which, res):
        Ln = embs[i].shape[0]
        ref = oracle_prefill(llava.ot, embs[i].float().cpu().numpy(), None, *args)
        assert torch.equal(i16(e.target_kv[:, 0, :, :P_ROWS]), i16(pfx.store)), "prefix rows are the store's bytes"
        assert tuple(hid.shape) == (Ln - P_ROWS, T["D"]) and tuple(lg.shape) == (1, T["V"])
        close(hid.float().cpu().numpy(), ref[1][P_ROWS:])
        close(e.target_kv.float().cpu().numpy()[:, 0, :, :Ln], ref[2])
        close(lg.float().cpu().numpy()[0], ref[0])
        assert (e.target_kv[:, :, :, Ln:] == CANARY).all()
    # request 3 (33 new rows) next to two companions of 100 + 1 new rows, then next to four of 5 + 2 + 17 + 77: the same total row count
    # (one piece of 134 rows either way), other neighbours, other segment counts
    assert SUFFIX[0] + SUFFIX[1] == SUFFIX[2] + SUFFIX[4] + SUFFIX[5] + SUFFIX[7] == 101
    engines = [m.engine for m in llava.models[:5]]
    a = batched([3, 0, 1])
    kv_a = engines[0].target_kv.clone()
    b = batched([3, 2, 4, 5, 7])
    assert torch.equal(i16(a[0][1]), i16(b[0][1])) and torch.equal(a[0][0], b[0][0]) and torch.equal(i16(kv_a), i16(engines[0].target_kv))
    # a list mixing a prefix with None, through the cohort entry: the tuples of the requests alone
    reqs = [(llava.ids[1], {}), (llava.ids[5], dict(pixel_values=llava.feats)), (llava.ids[3], {}), (llava.ids[2], dict(pixel_values=llava.feats))]
    budgets = [llava.budgets[i] for i in (1, 5, 3, 2)]
    want = [solo(llava, 1), sm.specgenerate(llava.ids[5], max_new_tokens=budgets[1], log=True, return_acceptance_len=True, pixel_values=llava.feats),
            solo(llava, 3), sm.specgenerate(llava.ids[2], max_new_tokens=budgets[3], log=True, return_acceptance_len=True, pixel_values=llava.feats)]
    st = {}
    got = specgenerate_cohort(models, reqs, max_new_tokens=budgets, prefix=[pfx, None, pfx, None], batch_prefill=True, stats=st)
    assert st["prefix_forks"] == [2]
    same_tuples(got, want)
    got = specgenerate_cohort(models, [(llava.ids[i], {}) for i in range(4)], max_new_tokens=llava.budgets[:4], prefix=pfx, batch_prefill=True,
                              prefill_chunk_rows=50)
    same_tuples(got, [solo(llava, i) for i in range(4)])


def test_stream_on_one_prefix(llava):
    """2 slots, 5 requests, one prefix: the results in request order equal the solo prefixed runs; prefix_forks accounts for all five."""
    slots = llava.models[:2]
    reqs = [(llava.ids[i], {}) for i in range(5)]
    want = [solo(llava, i) for i in range(5)]
    for bp in (False, True):
        st = {}
        got = specgenerate_stream(slots, reqs, max_new_tokens=llava.budgets[:5], prefix=llava.pfx, stats=st, batch_prefill=bp)
        same_tuples(got, want)
        forks = st["prefix_forks"]
        print("prefix_forks", forks)
        assert forks[0] == 2 and sum(forks) == 5 and all(1 <= f <= 2 for f in forks)
    st = {}
    got = specgenerate_stream(slots, reqs[:2], max_new_tokens=llava.budgets[:2], prefix=[llava.pfx, llava.pfx], stats=st)  # requests <= slots
    same_tuples(got, want[:2])
    assert st["prefix_forks"] == [2]
    st = {}
    specgenerate_stream(slots, [(llava.ids[1], dict(pixel_values=llava.feats))] * 3, max_new_tokens=4, stats=st)
    assert "prefix_forks" not in st


# ---------------------------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_every_cache_unchanged(llava):
    sm, m1, pfx = llava.models[0], llava.models[1], llava.pfx
    good = llava.ids[2]
    other, _, _ = build(51, 61, True, arch="LlavaNextForConditionalGeneration")
    foreign = other.prefill_prefix(good[:, :P_ROWS], pixel_values=llava.feats)
    wrong = good.clone()
    wrong[0, 7] = 3 + (int(wrong[0, 7]) - 2) % (IMG_TOK - 3)
    visual = good.clone()
    visual[0, -1] = IMG_TOK
    too_long = torch.cat([good[:, :P_ROWS], torch.full((1, T["max_pos"] - P_ROWS - 20), 5, dtype=torch.int64)], dim=1)
    cases = [(wrong, pfx, ValueError, "does not begin"), (visual, pfx, ValueError, "placeholder"), (good[:, :P_ROWS], pfx, ValueError, "new row"),
             (good, foreign, ValueError, "other target weights"), (too_long, pfx, L.VispecError, "does not fit")]
    for m in (sm, m1):
        m.engine.target_kv.fill_(CANARY)
        m.engine.target_kv[:, :, :, ::7] = 1.0
    snap = [m.engine.target_kv.clone() for m in (sm, m1)]
    for ids, pf, exc, word in cases:
        with pytest.raises(exc, match=word):
            sm.specgenerate(ids, max_new_tokens=4, prefix=pf)
        with pytest.raises(exc, match=word):  # the second request of a cohort: the first one's cache is not written either
            specgenerate_cohort([sm, m1], [(good, {}), (ids, {})], max_new_tokens=4, prefix=[pfx, pf])
        with pytest.raises(exc, match=word):
            specgenerate_cohort([sm, m1], [(good, {}), (ids, {})], max_new_tokens=4, prefix=[pfx, pf], batch_prefill=True)
        with pytest.raises(exc, match=word):
            specgenerate_stream([sm, m1], [(good, {}), (ids, {}), (good, {})], max_new_tokens=4, prefix=[pfx, pf, pfx])
        torch.cuda.synchronize()
        for m, s in zip((sm, m1), snap):
            assert torch.equal(i16(m.engine.target_kv), i16(s)), word
    with pytest.raises(ValueError):
        sm.specgenerate(None, inputs_embeds=torch.zeros(1, 210, T["D"]), prefix=pfx)
    with pytest.raises(ValueError):
        specgenerate_cohort([sm, m1], [(good, {}), (good, {})], max_new_tokens=4, prefix=[pfx])
    with pytest.raises(L.VispecError, match="does not fit"):
        sm.base_model.prefill_batch([sm.engine, m1.engine], [torch.zeros(100, T["D"], dtype=torch.bfloat16, device="cuda")] * 2, None,
                                    past_lens=[0, T["max_pos"] - 120])
    for m, s in zip((sm, m1), snap):
        assert torch.equal(i16(m.engine.target_kv), i16(s))
    same_tuples([sm.specgenerate(good, max_new_tokens=llava.budgets[2], log=True, return_acceptance_len=True, prefix=pfx)], [solo(llava, 2)])
