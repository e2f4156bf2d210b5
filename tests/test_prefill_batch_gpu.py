"""Batched prompt prefill: the varlen HIP kernels (vispec_prefill_attention_varlen, vispec_rope_append_varlen) against the single-sequence
entries bit for bit, TargetLM.prefill_batch against the oracle's bf16 forward, and the batch_prefill switch of specgenerate_cohort /
specgenerate_stream against the per-request start (tiny models and the full-size bench models).

Arithmetic class that these tests pin down: both varlen kernels and every row-wise kernel are bit-identical to the per-request path; the
library GEMMs run at M = sum L and may sum in another fp32 order, so prefill_batch is held to the oracle within the bars of the
single-request prefill comparisons (test_stage_fixtures_gpu.close: 2^-6 of the tensor's largest magnitude), and to itself exactly when
only the company of a prompt changes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from helpers import T, synth, vo  # noqa: E402
from test_loop_gpu import IMG_TOK, build, build_qwen  # noqa: E402
from test_stage_fixtures_gpu import close  # noqa: E402  (the bar of the single-request prefill comparisons)
from vispec_amd import lib as L  # noqa: E402
from vispec_amd.model.spec_model_ours import specgenerate_cohort, specgenerate_stream  # noqa: E402

CANARY = -1536.0  # exact in bf16
p = lambda t: C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rand_bf16(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen, device="cuda") * scale).to(torch.bfloat16)


def segs_of(row0, lens, ks, vs):
    segs = (L.PrefillSeg * len(lens))()
    for i in range(len(lens)):
        segs[i] = L.PrefillSeg(row0[i], lens[i], ks[i].data_ptr(), vs[i].data_ptr())
    return segs


def packed_row0(lens, pad=0):
    r, out = 0, []
    for ln in lens:
        out.append(r)
        r += ln + pad
    return out, r


EIGHT = (2704, 1584, 911, 640, 257, 129, 64, 1)
LENGTH_SETS = [((n,), 0) for n in (1, 127, 128, 129, 257, 2704)] + [
    ((1, 2704), 0), ((129, 128, 127), 0), ((2704, 2144, 600, 33), 0), (EIGHT, 0), ((129, 128, 127), 5), ((300, 2, 1000), 131)]


# ------------------------------------------------------------------------------------------------------------------ 1. varlen attention
@pytest.mark.parametrize("eager", [1, 0])
@pytest.mark.parametrize("H,Hkv", [(32, 32), (28, 4)])
@pytest.mark.parametrize("lens,pad", LENGTH_SETS)
def test_varlen_attention_is_the_single_entry_bit_for_bit(lens, pad, H, Hkv, eager):
    """Every output row of the varlen launch == the row vispec_prefill_attention computes for that sequence alone (array equality); rows
    of the out buffer that belong to no sequence (padded row0) keep their canary."""
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(1234 + sum(lens) + H)
    n = len(lens)
    S = (max(lens) + 127) // 128 * 128 + 64
    ldq, ldo = (H + 2 * Hkv) * 128, H * 128
    row0, total = packed_row0(lens, pad)
    q = rand_bf16(gen, total, ldq)
    ks = [rand_bf16(gen, Hkv, S, 128) for _ in range(n)]
    vs = [rand_bf16(gen, Hkv, S, 128) for _ in range(n)]
    want = []
    for i in range(n):
        o = torch.full((lens[i], ldo), CANARY, dtype=torch.bfloat16, device="cuda")
        qi = q[row0[i]:row0[i] + lens[i]]
        L.check(lib.vispec_prefill_attention(None, stream(), p(qi), ldq, p(ks[i]), p(vs[i]), S, H, Hkv, lens[i], p(o), ldo, eager))
        want.append(o)
    out = torch.full((total, ldo), CANARY, dtype=torch.bfloat16, device="cuda")
    segs = segs_of(row0, lens, ks, vs)
    L.check(lib.vispec_prefill_attention_varlen(None, stream(), p(q), ldq, segs, n, S, H, Hkv, p(out), ldo, eager))
    torch.cuda.synchronize()
    owned = torch.zeros(total, dtype=torch.bool, device="cuda")
    for i in range(n):
        got = out[row0[i]:row0[i] + lens[i]]
        assert not (want[i] == CANARY).all(dim=1).any()  # the single entry wrote every row
        assert torch.equal(got.view(torch.int16), want[i].view(torch.int16)), f"sequence {i} of {lens}"
        owned[row0[i]:row0[i] + lens[i]] = True
    assert (out[~owned] == CANARY).all()


# ---------------------------------------------------------------------------------------------------------------- 2. varlen rope + append
@pytest.mark.parametrize("source", ["shared", "per_request"])
@pytest.mark.parametrize("H,Hkv", [(32, 32), (28, 4)])
@pytest.mark.parametrize("lens,pad", [((1,), 0), ((129,), 0), ((1, 300), 0), ((129, 128, 127), 0), ((257, 33, 600, 64), 3), (EIGHT, 0)])
def test_varlen_rope_append_is_the_single_entry_bit_for_bit(lens, pad, H, Hkv, source):
    """Rotated q rows and K/V rows [0, L_s) of every cache == vispec_rope_append on that sequence alone; cache rows >= L_s and padding rows
    of the q|k|v buffer keep their content.  Both rotary sources: one shared table indexed by the position inside the sequence, and
    per-request tables with distinct contents (M-RoPE style) concatenated like the rows."""
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(77 + sum(lens) + Hkv)
    n = len(lens)
    S = max(lens) + 70
    NH = H + 2 * Hkv
    row0, total = packed_row0(lens, pad)
    qkv0 = rand_bf16(gen, total, NH * 128)
    if source == "shared":
        cos, sin = rand_bf16(gen, S, 128), rand_bf16(gen, S, 128)
        tabs = [(cos, sin)] * n
        table_global = 0
    else:
        cos, sin = rand_bf16(gen, total, 128), rand_bf16(gen, total, 128)  # every request's own rows: distinct contents
        tabs = [(cos[row0[i]:row0[i] + lens[i]].contiguous(), sin[row0[i]:row0[i] + lens[i]].contiguous()) for i in range(n)]
        table_global = 1
    want_q, want_k, want_v = [], [], []
    for i in range(n):
        x = qkv0[row0[i]:row0[i] + lens[i]].clone()
        kc = torch.full((Hkv, S, 128), CANARY, dtype=torch.bfloat16, device="cuda")
        vc = torch.full((Hkv, S, 128), CANARY, dtype=torch.bfloat16, device="cuda")
        L.check(lib.vispec_rope_append(None, stream(), p(x), lens[i], H, Hkv, 128, p(tabs[i][0]), p(tabs[i][1]), None, None, p(kc), p(vc), S, None))
        want_q.append(x)
        want_k.append(kc)
        want_v.append(vc)
    qkv = qkv0.clone()
    ks = [torch.full((Hkv, S, 128), CANARY, dtype=torch.bfloat16, device="cuda") for _ in range(n)]
    vs = [torch.full((Hkv, S, 128), CANARY, dtype=torch.bfloat16, device="cuda") for _ in range(n)]
    segs = segs_of(row0, lens, ks, vs)
    L.check(lib.vispec_rope_append_varlen(None, stream(), p(qkv), H, Hkv, 128, p(cos), p(sin), table_global, segs, n, S))
    torch.cuda.synchronize()
    owned = torch.zeros(total, dtype=torch.bool, device="cuda")
    i16 = lambda t: t.view(torch.int16)
    for i in range(n):
        assert torch.equal(i16(qkv[row0[i]:row0[i] + lens[i]]), i16(want_q[i])), f"q|k|v rows of sequence {i}"
        assert torch.equal(i16(ks[i]), i16(want_k[i])) and torch.equal(i16(vs[i]), i16(want_v[i])), f"cache of sequence {i}"
        assert (ks[i][:, lens[i]:] == CANARY).all() and (vs[i][:, lens[i]:] == CANARY).all()
        assert not (ks[i][:, :lens[i]] == CANARY).all(dim=2).any()
        owned[row0[i]:row0[i] + lens[i]] = True
    assert torch.equal(i16(qkv[~owned]), i16(qkv0[~owned]))


def test_c_entries_refuse_bad_segment_tables():
    lib = L.load()
    gen = torch.Generator(device="cuda").manual_seed(5)
    S, H = 256, 2
    q = rand_bf16(gen, 64, 3 * H * 128)
    out = torch.zeros(64, H * 128, dtype=torch.bfloat16, device="cuda")
    kc, vc = rand_bf16(gen, H, S, 128), rand_bf16(gen, H, S, 128)
    cos, sin = rand_bf16(gen, S, 128), rand_bf16(gen, S, 128)
    nine = segs_of([4 * i for i in range(9)], [4] * 9, [kc] * 9, [vc] * 9)
    err = lambda: (lib.vispec_last_error() or b"").decode()
    for n_seq in (0, 9):
        assert lib.vispec_prefill_attention_varlen(None, stream(), p(q), 3 * H * 128, nine, n_seq, S, H, H, p(out), H * 128, 1) != 0
        assert "n_seq" in err() and "prefill_attention_varlen" in err()
        assert lib.vispec_rope_append_varlen(None, stream(), p(q), H, H, 128, p(cos), p(sin), 0, nine, n_seq, S) != 0
        assert "n_seq" in err() and "rope_append_varlen" in err()
    overlap = segs_of([0, 8], [16, 16], [kc] * 2, [vc] * 2)
    assert lib.vispec_prefill_attention_varlen(None, stream(), p(q), 3 * H * 128, overlap, 2, S, H, H, p(out), H * 128, 1) != 0
    too_long = segs_of([0], [S + 1], [kc], [vc])
    assert lib.vispec_rope_append_varlen(None, stream(), p(q), H, H, 128, p(cos), p(sin), 0, too_long, 1, S) != 0
    torch.cuda.synchronize()
    assert (out == 0).all()
    assert lib.vispec_version() == 4


# ------------------------------------------------------------------------------------------------------- 3. prefill_batch against the oracle
def llava_prompt(rng, n_pre, n_img, n_post):
    ids = np.concatenate([rng.integers(3, IMG_TOK, n_pre), np.full(n_img, IMG_TOK), rng.integers(3, IMG_TOK, n_post)]).astype(np.int64)
    feats = synth.bf16_grid(rng.standard_normal((n_img, T["D"]), dtype=np.float32) * 0.05)
    return ids, feats


def qwen_prompt(rng, IMG, D, runs):
    """runs = [(n_text_before, (t, h, w)), ...] + trailing text; -> ids, feats, grids"""
    parts, grids = [], []
    for n_text, g in runs:
        parts += [rng.integers(3, IMG, n_text), np.full(g[0] * (g[1] // 2) * (g[2] // 2), IMG)]
        grids.append(g)
    parts.append(rng.integers(3, IMG, 5))
    ids = np.concatenate(parts).astype(np.int64)
    feats = synth.bf16_grid(rng.standard_normal((int((ids == IMG).sum()), D), dtype=np.float32) * 0.05)
    return ids, feats, grids


def embeds_of(ot, ids, feats, img):
    emb = ot.w["model.embed_tokens.weight"][ids].copy()
    emb[ids == img] = feats
    return emb


def t_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).cuda()


def check_against_oracle(ot, engines, res, embs, poss, NL, Hkv, max_pos, hd):
    for e, (logits, hidden), emb, pos3 in zip(engines, res, embs, poss):
        pkv, pkv_data, cur = vo.initialize_past_key_values(NL, Hkv, max_pos, hd)
        lg, hid = ot.forward(pkv, inputs_embeds=emb, position_ids=pos3) if pos3 is not None else ot.forward(pkv, inputs_embeds=emb)
        Ln = emb.shape[0]
        assert logits.dtype == torch.float32 and tuple(logits.shape) == (1, lg.shape[-1])
        assert hidden.dtype == torch.bfloat16 and tuple(hidden.shape) == (Ln, emb.shape[1]) and hidden.is_contiguous()
        close(hidden.float().cpu().numpy(), hid)
        kvd = e.target_kv.float().cpu().numpy()
        close(kvd[:, 0, :, :Ln], pkv_data[0][:, 0, :, :Ln])
        close(logits.float().cpu().numpy()[0], lg[-1])


LLAVA_SHAPES = [(5, 23, 9), (2, 70, 31), (40, 0, 1), (1, 130, 3), (9, 17, 4), (3, 64, 60), (12, 1, 12), (0, 200, 57)]


@pytest.mark.parametrize("n", [2, 3, 8])
def test_prefill_batch_matches_the_oracle_llava(n):
    sm, ot, od = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    models = [sm] + [sm.make_cohort_member() for _ in range(n - 1)]
    engines = [m.engine for m in models]
    rng = np.random.default_rng(300 + n)
    embs = [embeds_of(ot, *llava_prompt(rng, *LLAVA_SHAPES[i]), IMG_TOK) for i in range(n)]
    for e in engines:
        e.target_kv.fill_(CANARY)
    res = sm.base_model.prefill_batch(engines, [t_bf16(e_) for e_ in embs])
    torch.cuda.synchronize()
    check_against_oracle(ot, engines, res, embs, [None] * n, T["NL"], T["H"], T["max_pos"], T["D"] // T["H"])
    for e, emb in zip(engines, embs):  # no row past a request's prompt was written
        assert (e.target_kv[:, :, :, emb.shape[0]:] == CANARY).all()
    # all_logits: prefill()'s shape
    res_all = sm.base_model.prefill_batch(engines, [t_bf16(e_) for e_ in embs], all_logits=True)
    for (lg_all, _), (lg_last, _), emb in zip(res_all, res, embs):
        assert tuple(lg_all.shape) == (emb.shape[0], T["V"]) and lg_all.dtype == torch.float32
        close(lg_all[-1].cpu().numpy(), lg_last[0].cpu().numpy())  # (the lm_head GEMM at M = L_i against M = 1)
    # max_rows splits the batch into consecutive sub-batches: still the oracle's arithmetic
    res_split = sm.base_model.prefill_batch(engines, [t_bf16(e_) for e_ in embs], max_rows=embs[0].shape[0] + embs[1].shape[0])
    check_against_oracle(ot, engines, res_split, embs, [None] * n, T["NL"], T["H"], T["max_pos"], T["D"] // T["H"])


@pytest.mark.parametrize("n", [2, 3, 8])
def test_prefill_batch_matches_the_oracle_qwen(n):
    """GQA 4/2, q/k/v bias, SDPA-class scores, per-request M-RoPE tables (a text-only prompt among them: its rows use the plain table)."""
    sm, ot, od, IMG = build_qwen()
    Q = synth.QWEN_TINY
    models = [sm] + [sm.make_cohort_member() for _ in range(n - 1)]
    engines = [m.engine for m in models]
    rng = np.random.default_rng(400 + n)
    layouts = [[(4, (1, 6, 8)), (3, (1, 4, 4))], [(9, (1, 4, 4))], [(30, (1, 2, 2))], [(1, (1, 8, 12)), (2, (1, 2, 4)), (7, (1, 4, 6))],
               [(6, (1, 10, 10))], [(2, (1, 4, 8)), (40, (1, 2, 2))], [(17, (1, 6, 6))], [(3, (1, 12, 12))]]
    embs, poss = [], []
    for i in range(n):
        ids, feats, grids = qwen_prompt(rng, IMG, Q["D"], layouts[i])
        embs.append(embeds_of(ot, ids, feats, IMG))
        poss.append(synth.qwen_rope_index(ids, IMG, grids)[0])
    res = sm.base_model.prefill_batch(engines, [t_bf16(e_) for e_ in embs], [torch.from_numpy(p3) for p3 in poss])
    torch.cuda.synchronize()
    check_against_oracle(ot, engines, res, embs, poss, Q["NL"], Q["Hkv"], Q["max_pos"], Q["D"] // Q["H"])


def test_a_request_does_not_depend_on_what_shares_its_batch():
    """The same prompt in two batches of the same total row count but other companions (other lengths, other contents): identical K/V rows,
    hidden rows and logits, bit for bit."""
    sm, ot, od = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    models = [sm] + [sm.make_cohort_member() for _ in range(2)]
    engines = [m.engine for m in models]
    rng = np.random.default_rng(555)
    a = embeds_of(ot, *llava_prompt(rng, 7, 90, 20), IMG_TOK)                 # 117 rows
    b1, c1 = embeds_of(ot, *llava_prompt(rng, 3, 50, 7), IMG_TOK), embeds_of(ot, *llava_prompt(rng, 10, 100, 30), IMG_TOK)  # 60 + 140
    b2, c2 = embeds_of(ot, *llava_prompt(rng, 30, 99, 4), IMG_TOK), embeds_of(ot, *llava_prompt(rng, 1, 60, 6), IMG_TOK)    # 133 + 67
    assert b1.shape[0] + c1.shape[0] == b2.shape[0] + c2.shape[0]
    r1 = sm.base_model.prefill_batch(engines, [t_bf16(a), t_bf16(b1), t_bf16(c1)])
    kv1 = engines[0].target_kv[:, :, :, :a.shape[0]].clone()
    r2 = sm.base_model.prefill_batch(engines, [t_bf16(a), t_bf16(b2), t_bf16(c2)])
    kv2 = engines[0].target_kv[:, :, :, :a.shape[0]].clone()
    assert torch.equal(kv1, kv2) and torch.equal(r1[0][1], r2[0][1]) and torch.equal(r1[0][0], r2[0][0])


# ----------------------------------------------------------------------------------------------------------- 5-8. tiny-model request starts
def tiny_requests(rng, n):
    reqs = []
    for i in range(n):
        ids, feats = llava_prompt(rng, *LLAVA_SHAPES[i % len(LLAVA_SHAPES)])
        kw = dict(pixel_values=t_bf16(feats)) if len(feats) else {}
        reqs.append((torch.from_numpy(ids)[None], kw))
    return reqs


def same_tuples(got, want):
    for t, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g[0], w[0]) and (g[1], g[2], g[3]) == (w[1], w[2], w[3]), f"request {t}"


@pytest.fixture(scope="module")
def tiny_cohort():
    sm, ot, od = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    return [sm] + [sm.make_cohort_member() for _ in range(3)], ot, od


def test_batched_start_equals_the_unbatched_start_and_the_default_is_unchanged(tiny_cohort):
    """Greedy: a cohort started through one batched prefill returns the tuples of the per-request start, which are the oracle's; and a run
    with default arguments after a batched run is bit-identical to the one before it (no state leaks between the two kinds of start)."""
    models, ot, od = tiny_cohort
    reqs = tiny_requests(np.random.default_rng(91), 4)
    before = specgenerate_cohort(models, reqs, max_new_tokens=30)
    kv_before = [m.engine.target_kv.clone() for m in models]
    batched = specgenerate_cohort(models, reqs, max_new_tokens=30, batch_prefill=True)
    after = specgenerate_cohort(models, reqs, max_new_tokens=30)
    same_tuples(after, before)
    for m, kv in zip(models, kv_before):
        assert torch.equal(m.engine.target_kv, kv)
    same_tuples(batched, before)
    ids0, kw0 = reqs[0]
    mask = (ids0[0] == IMG_TOK).numpy()
    emb = embeds_of(ot, ids0[0].numpy(), kw0["pixel_values"].float().cpu().numpy(), IMG_TOK)
    o_out, o_new, o_idx, o_acc = vo.specgenerate(ot, od, ids0[0].numpy(), inputs_embeds=emb, image_mask=mask, max_new_tokens=30, max_pos=T["max_pos"])
    np.testing.assert_array_equal(batched[0][0][0].cpu().numpy(), o_out)
    assert batched[0][3] == o_acc


@pytest.mark.parametrize("temperature,top_k", [(1.0, 4), (5.0, 6)])
def test_batched_start_with_sampling(tiny_cohort, temperature, top_k):
    """temperature > 0 with top_k: the first token of a batched start comes from each engine's own sample_row and seed."""
    models, _, _ = tiny_cohort
    reqs = tiny_requests(np.random.default_rng(92), 3)
    kw = dict(temperature=temperature, top_k=top_k, seeds=[3, 4, 5], max_new_tokens=24)
    want = specgenerate_cohort(models[:3], reqs, **kw)
    got = specgenerate_cohort(models[:3], reqs, batch_prefill=True, **kw)
    same_tuples(got, want)


def test_stream_with_batched_fills(tiny_cohort):
    """More requests than slots, unequal budgets: the same outputs in request order; the first batch fills every slot, and the batch
    sizes account for every request that did not start through the per-request path."""
    models, _, _ = tiny_cohort
    slots = models[:3]
    reqs = tiny_requests(np.random.default_rng(93), 9)
    budgets = [12, 12, 12, 30, 7, 7, 18, 5, 9]  # equal first budgets: slots that finish in the same round are refilled as one batch
    st0, st1 = {}, {}
    want = specgenerate_stream(slots, reqs, max_new_tokens=budgets, stats=st0)
    singles = []
    for m in slots:  # count the starts that go through the per-request path
        m._start_request = (lambda f: lambda *a, **k: (singles.append(1), f(*a, **k))[1])(m._start_request)
    try:
        got = specgenerate_stream(slots, reqs, max_new_tokens=budgets, stats=st1, batch_prefill=True)
    finally:
        for m in slots:
            del m._start_request
    same_tuples(got, want)
    assert "prefill_batches" not in st0
    pb = st1["prefill_batches"]
    print("prefill_batches", pb, "single refills", len(singles))
    assert pb[0] == len(slots) and all(2 <= b <= len(slots) for b in pb) and sum(pb) + len(singles) == len(reqs)
    assert (st1["rounds"], st1["request_rounds"]) == (st0["rounds"], st0["request_rounds"])
    # requests <= slots: the plain cohort, started as one batch
    st2 = {}
    got2 = specgenerate_stream(slots, reqs[:3], max_new_tokens=budgets[:3], stats=st2, batch_prefill=True)
    same_tuples(got2, want[:3])
    assert st2["prefill_batches"] == [3]


def test_refusals(tiny_cohort):
    models, ot, _ = tiny_cohort
    engines = [m.engine for m in models]
    rng = np.random.default_rng(94)
    ok = t_bf16(embeds_of(ot, *llava_prompt(rng, 5, 23, 9), IMG_TOK))
    too_long = torch.zeros(T["max_pos"] - 8, T["D"], dtype=torch.bfloat16, device="cuda")
    for e in engines:
        e.target_kv.fill_(CANARY)
    with pytest.raises(L.VispecError, match="does not fit"):
        models[0].base_model.prefill_batch(engines[:3], [ok, ok, too_long])
    torch.cuda.synchronize()
    for e in engines:
        assert (e.target_kv == CANARY).all()
    other, _, _ = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    with pytest.raises(ValueError, match="leader group"):
        models[0].base_model.prefill_batch([engines[0], other.engine], [ok, ok])
    with pytest.raises(ValueError, match="cohort_leader"):
        specgenerate_cohort([models[0], other], tiny_requests(rng, 2), max_new_tokens=4, batch_prefill=True)
    for e in engines:
        assert (e.target_kv == CANARY).all()
    with pytest.raises(TypeError):
        specgenerate_cohort(models[:2], tiny_requests(rng, 2), max_new_tokens=4, batch_prefil=True)


# ------------------------------------------------------------------------------------------------------------------------ 4. full size
@pytest.fixture(scope="module", params=["llava7b", "qwen7b", "qwen7b-fp8a8"])
def cohort_full(request):
    import gc
    import bench
    bench.MODEL = request.param
    lanes, tcfg, _ = bench.build_models(torch.device("cuda:0"), 0, 0, 1, 1, 8)
    yield lanes[0], tcfg, request.param
    bench.MODEL = "llava7b"
    del lanes
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n", [2, 4, 8])
def test_batched_cohort_start_at_full_size(cohort_full, n):
    """Cohorts of 2, 4 and 8 at the bench prompt shapes (LLaVA-7B: 2704 rows; Qwen2.5-VL-7B: 1584 rows, four image runs, M-RoPE; the W8A8
    Qwen variant: 2124 rows): a cohort started through ONE batched prefill equals greedy AR token for token — the assertion that must
    hold — and returns the tuples of the per-request start (an observation on these wide-margin synthetic weights, like the existing
    cohort-of-8 comparisons: the GEMMs at M = sum L may sum in another fp32 order)."""
    import bench
    models, tcfg, name = cohort_full
    bench.MODEL = name
    dev = torch.device("cuda:0")
    NEW = 40
    reqs = [bench.make_request(tcfg, 40 + i, dev) for i in range(n)]
    budgets = [NEW, 33, 36, 29, 40, 31, 38, 35][:n]
    want = specgenerate_cohort(models[:n], reqs, max_new_tokens=budgets)
    got = specgenerate_cohort(models[:n], reqs, max_new_tokens=budgets, batch_prefill=True)
    for t, ((ids, pix), (toks, new_token, idx, acc)) in enumerate(zip(reqs, got)):
        assert new_token > budgets[t] and toks.shape[1] == ids.shape[1] + new_token
        ar = models[0].baseline_generate(ids, max_new_tokens=budgets[t], max_steps=budgets[t] + 1, **pix)
        m = min(ar.shape[1], toks.shape[1])
        assert m >= ids.shape[1] + budgets[t]
        np.testing.assert_array_equal(ar[0, :m].cpu().numpy(), toks[0, :m].cpu().numpy(), err_msg=f"{name}: request {t} vs greedy AR")
    same_tuples(got, want)
