"""The draft prefill (vispec_draft_prefill: fc(cat(emb, img_fc(cat(h, g)))) over the text segments, the ImgAdaptor over every image run,
then k|v with rotary at the ORIGINAL positions into the compressed draft KV cache) against the oracle's DraftModel.forward_prefill, at
the row counts where its forms switch and at the real draft widths.

Every later draft round attends over the cache this writes, so it sets the acceptance length; it does not set the output tokens
(speculative output equals greedy AR whatever the draft proposes), so the full-size token tests cannot see a wrong prefill.  The forms:

 * text segments of >= 64 rows: two BIG_PLAIN prefill GEMMs (csrc/gemm_prefill.h) with the rows gathered through idx0 and cat(h, g) /
   cat(emb, img_fc(...)) formed at k_split, g a broadcast row (bcast1); shorter segments: 32-row passes of the skinny kernel;
 * image runs of >= 64 rows: one BIG_KV GEMM scattering k|v into the adaptor's [H][cap][128] scratch; shorter runs: skinny passes;
 * the compressed sequence (Lc rows) when Lc >= 64 and the q|k|v weight is rope-ordered (3D = 4608 and up): one BIG_ROPE_KV GEMM (bias in
   natural order, rotary at pos[m], append), then the last 32-row chunk again through the skinny q|k|v (o_first) for the last row's q.

Asserted for every prompt: draft_len == the oracle's Lc; the whole compressed K and V within 2^-6 of each (head, row)'s largest magnitude
(the statistical tail rule of test_full_size_gpu.assert_close_with_tail); g and the last hidden row; the first tree (exact on the device's
own candidate lists, root top-k == the oracle's wherever it is unambiguous); no draft-KV row written past the first round's capacity
bound; and, re-running a prompt after another one, bit-identical results."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from helpers import synth, vo  # noqa: E402
from test_full_size_gpu import assert_close_with_tail  # noqa: E402
from test_loop_gpu import IMG_TOK, check_tree_exact, dev_tree_inputs  # noqa: E402
from vispec_amd.engine import DraftConfig, TargetConfig  # noqa: E402
from vispec_amd.model import SpecModel  # noqa: E402

BIG_MIN_ROWS, CHUNK = 64, 32  # PREFILL_BIG_MIN_ROWS and CHUNK of vispec_hip.hip
SENTINEL = -1536.0            # exact in bf16; what every draft-KV row past the first round's rows must still hold


def token_mask(parts):
    """[("t", n_text_tokens) | ("i", n_image_tokens), ...] -> (L, image mask over the tokens, or None without an image token)."""
    m = np.concatenate([np.full(n, k == "i") for k, n in parts])
    return len(m), (m if m.any() else None)


def prefill_plan(mask, L, num_q):
    """(text segment rows, image run rows, Lc) of a prompt, segmented the way vispec_draft_prefill's host plan does: row r is an image row
    when token r + 1 is one (the embeddings are shifted by one, cnets_ours.py:880), a run is a maximal block of image rows, the text rows
    before each run form one segment (none when empty), each run becomes num_q - 1 compressed rows, and the rows after the last run (at
    least row L - 1, which pairs with the sampled token) form the last segment."""
    m1 = np.zeros(L - 1, bool) if mask is None else np.asarray(mask, bool)[1:]
    texts, runs, t, n = [], [], 0, 0
    for r in range(L - 1):
        if m1[r]:
            n += 1
            continue
        if n:
            texts += [t] if t else []
            runs.append(n)
            t = n = 0
        t += 1
    if n:
        texts += [t] if t else []
        runs.append(n)
        t = 0
    texts.append(t + 1)
    return texts, runs, sum(texts) + len(runs) * (num_q - 1)


def gemm_rows(texts, runs, Lc):
    """M of every prefill-GEMM launch of a plan, per form, and the first row of the skinny q|k|v pass (a width whose q|k|v is fused)."""
    big = dict(plain=[n for n in texts if n >= BIG_MIN_ROWS], kv=[n for n in runs if n >= BIG_MIN_ROWS],
               rope_kv=[Lc] if Lc >= BIG_MIN_ROWS else [])
    return big, ((Lc - 1) // CHUNK) * CHUNK if big["rope_kv"] else 0


# ---------------------------------------------------------------------------------------------------------------------------- A. D = 1536
W = dict(D=1536, H=12, I=1024, V=1008, P=2048, DP=512)  # DP: draft cache rows (the sentinel region behind every compressed prompt)
DRAFTS = {  # draft variant -> (num_q, q|k|v bias, rope_theta, rms_norm_eps)
    "q2": (2, False, 1e4, 1e-5),
    "q3_bias": (3, True, 1e6, 1e-6),  # Qwen-style: q|k|v (and adaptor k|v) bias, theta 1e6, eps 1e-6
    "q5": (5, False, 1e4, 1e-5),
}
# prompt -> (draft variant, mask layout in tokens).  Row r pairs with token r + 1: a leading text segment has one row fewer than its
# tokens, the trailing one a row more (row L - 1 pairs with the sampled token), so a prompt that ends on an image token keeps one text
# row.  test_row_edge_table_covers_every_switch checks what the comments say.  (Grouped by variant: one engine per group.)
ROW_EDGE = {
    "text64": ("q2", [("t", 64)]),                                             # no image: g = 0 through bcast1; Lc 64
    "img1000_last": ("q2", [("t", 64), ("i", 1000)]),                          # text 63 (skinny), run 1000, image to the end, Lc 65
    "lc63": ("q2", [("t", 31), ("i", 70), ("t", 31)]),                         # Lc 63: q|k|v stays skinny
    "two_runs_q5": ("q5", [("t", 66), ("i", 63), ("t", 1), ("i", 65), ("t", 22)]),  # runs 63 / 65 split by one text row, Lc 97
    "lc96_q5": ("q5", [("t", 5), ("i", 128), ("t", 87)]),                      # Lc 96
    "long_text_q5": ("q5", [("t", 129), ("i", 129), ("t", 256)]),              # text 128 / 257
    "text129_bias": ("q3_bias", [("t", 129)]),                                 # Lc 129
    "lc128_bias": ("q3_bias", [("t", 64), ("i", 200), ("t", 62)]),             # Lc 128
    "four_runs_bias": ("q3_bias", [("t", 128), ("i", 128), ("t", 1), ("i", 129), ("t", 64), ("i", 64), ("t", 1), ("i", 65), ("t", 3)]),
}
WANT = dict(  # every M value of every prefill-GEMM form (and of the skinny stay / handoff) that the table must reach
    text=[63, 64, 65, 127, 128, 129], text_ge=257, runs=[63, 64, 65, 128, 129], runs_ge=1000, Lc=[63, 64, 65, 96, 97, 128, 129])


def make_pair(D, H, I, V, P, DP, num_q, bias, theta, eps, seed, target_I=None):
    """(SpecModel, bf16 oracle, fp32 oracle, lm_head) of a synthetic draft at (D, H, I) over a ONE-layer target.  Only the target's
    lm_head (the draft's head) and the draft's own weights enter the draft prefill, so the target's intermediate size may be reduced."""
    tI = target_I or I
    tw = synth.make_target_weights(D, H, tI, V, 1, seed=seed)
    dw = synth.make_draft_weights(D, H, I, V, num_q=num_q, seed=seed + 1, qkv_bias=bias)
    tcfg = TargetConfig(hidden_size=D, num_heads=H, num_kv_heads=H, intermediate_size=tI, vocab_size=V, num_layers=1, max_position_embeddings=P,
                        image_token_index=IMG_TOK)
    dcfg = DraftConfig(hidden_size=D, num_heads=H, intermediate_size=I, vocab_size=V, max_position_embeddings=DP, rms_norm_eps=eps,
                       rope_theta=theta, qkv_bias=bias)
    sm = SpecModel.from_weights(tcfg, dcfg, tw, dw, num_q=num_q)
    ocfg = vo.DraftConfig(D, H, I, V, P, rms_norm_eps=eps, rope_theta=theta, num_q=num_q)  # (oracle rotary tables cover every position)
    return sm, vo.DraftModel(ocfg, dw, bf16=True), vo.DraftModel(ocfg, dw, bf16=False), np.asarray(tw["lm_head.weight"], np.float32)


def make_inputs(D, parts, seed):
    L, mask = token_mask(parts)
    rng = np.random.default_rng(seed)
    hidden = synth.bf16_grid(rng.standard_normal((L, D), dtype=np.float32))
    embeds = synth.bf16_grid(rng.standard_normal((L, D), dtype=np.float32) * 0.05)
    ids = rng.integers(3, IMG_TOK, size=L + 1)  # ids[L]: the sampled first token
    return hidden, embeds, mask, ids


def run_prefill(eng, hidden, embeds, mask, ids):
    """begin_request + draft_prefill on a sentinel-filled draft cache; -> snapshot of what the prefill left (device tensors)."""
    L, D = hidden.shape
    eng.begin_request(ids[:L], 64)
    eng.draft_kv.fill_(SENTINEL)
    first = torch.tensor([ids[L]], dtype=torch.int32, device="cuda")
    eng.draft_prefill(torch.from_numpy(hidden).to(torch.bfloat16).cuda(), torch.from_numpy(embeds).to(torch.bfloat16).cuda(), mask, first)
    Lc = eng.state()["draft_len"]
    return dict(Lc=Lc, kv=eng.draft_kv[:, :, :Lc].clone(), g=eng.buffer("draft_g", (1, D)).clone(),
                last=eng.buffer("draft_last", (16, D))[:1].clone())


def oracle_prefill(od, hidden, embeds, mask, first):
    """forward_prefill on the reference's inputs: embeddings shifted by one, last row = the draft's embedding of the sampled token."""
    e_shift = np.concatenate([embeds[1:], od.ops.rd(od.w["embed_tokens.weight"][[first]])], 0)
    od.reset_kv()
    out_c, kv, pos = od.forward_prefill(hidden, e_shift, mask)
    return out_c, kv, pos, od.last_img_hidden.copy()


def assert_rows_close(got, want, what):
    """[H, Lc, 128]: |got - want| <= 2^-6 * max|want[h, row, :]| (each head-row against its own scale, so that one wrong row of small
    values cannot hide under the largest row's bar), tail rule of assert_close_with_tail.  -> the worst error in units of its bar.
    (Measured: up to 0.96 for K, whose rotary rounds twice more, and 0.50 for V, over every prompt here: 2^-6 is the tightest power of two.)"""
    bar = 2.0 ** -6 * np.abs(want).max(axis=-1, keepdims=True)
    rel = np.abs(got - want) / bar
    worst = np.unravel_index(np.argmax(rel), want.shape)
    try:
        assert_close_with_tail(got, want, bar)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e} (worst at head {worst[0]}, row {worst[1]})") from None
    return float(rel.max())


def check_prefill(sm, od, head_w, hidden, embeds, mask, ids, od32=None):
    """Run one prompt through the device and the oracle and assert everything listed in the module docstring.  -> the device snapshot."""
    eng = sm.engine
    L, D = hidden.shape
    k, depth = eng.top_k, eng.depth
    got = run_prefill(eng, hidden, embeds, mask, ids)
    out_c, (want_k, want_v, _), pos, g_want = oracle_prefill(od, hidden, embeds, mask, int(ids[L]))
    Lc = out_c.shape[0]
    texts, runs, plan_Lc = prefill_plan(mask, L, eng.num_q)
    assert got["Lc"] == Lc == plan_Lc == len(pos)
    # nothing written past the rows the prefill and the first tree own (the capacity check of vispec_draft_prefill)
    bound = Lc + k * depth + depth + 2
    assert bound < eng.draft_max_pos
    tail = eng.draft_kv[:, :, bound:]
    n_bad = int((tail != SENTINEL).sum())
    assert n_bad == 0, f"{n_bad} draft-KV elements at rows >= {bound} overwritten (Lc = {Lc})"
    kv = got["kv"].float().cpu().numpy()
    rk, rv = assert_rows_close(kv[0], want_k, "K"), assert_rows_close(kv[1], want_v, "V")
    print(f"L {L} Lc {Lc} text segments {texts} image runs {runs}: worst K / V error {rk:.3f} / {rv:.3f} of the row bar")
    if od32 is not None:  # triangulation: no further from the fp32 evaluation than the reference's own bf16 graph is (test_full_size_gpu)
        _, (k32, v32, _), _, _ = oracle_prefill(od32, hidden, embeds, mask, int(ids[L]))
        for name, g_, w_, t_ in (("K", kv[0], want_k, k32), ("V", kv[1], want_v, v32)):
            e_hip, e_ora = np.abs(g_ - t_), np.abs(w_ - t_)
            print(f"{name} vs fp32: HIP mean {e_hip.mean():.3g} max {e_hip.max():.3g} | bf16 oracle mean {e_ora.mean():.3g} max {e_ora.max():.3g}")
            assert e_hip.mean() <= 1.25 * e_ora.mean() and e_hip.max() <= 1.25 * e_ora.max(), \
                f"{name}: HIP further from fp32 than the bf16 oracle (mean {e_hip.mean():.3g} vs {e_ora.mean():.3g}, max {e_hip.max():.3g} vs {e_ora.max():.3g})"
    g = got["g"].float().cpu().numpy()
    np.testing.assert_allclose(g, g_want, rtol=0, atol=2.0 ** -6 * np.abs(g_want).max())  # (no image: exactly 0)
    last = got["last"].float().cpu().numpy()
    np.testing.assert_allclose(last[0], out_c[-1], rtol=0, atol=2.0 ** -6 * np.abs(out_c[-1]).max())
    # first tree: exact integer logic on the device's candidate lists; root top-k == the oracle's where the log-probs leave no doubt
    tok, _, _, _ = check_tree_exact(eng)
    assert tok[0] == ids[L]
    _, dev_tok, _ = dev_tree_inputs(eng)
    z = od.ops.linear(out_c[-1:], head_w)
    vals, want_tok = vo.topk_desc(od.ops.log_softmax(z)[0], k + 1)
    tol = 2.0 ** -6 * (np.abs(z).max() + np.abs(vals))  # the first-token guard of test_full_size_gpu + 2 bf16 ulps of the log-prob
    gap = vals[:-1] - vals[1:]
    for i in range(k):
        if gap[i] > tol[i] and (i == 0 or gap[i - 1] > tol[i]):
            assert dev_tok[i] == want_tok[i], f"root top-{k}: rank {i} token {dev_tok[i]} != {want_tok[i]}"
    return got


def build_pair(name):
    """The engine and oracles of one draft variant at D = 1536 (DRAFTS) or of one real width (REAL).  At the real widths the draft (D, H,
    I, bias, theta, eps) is the real one; the target is ONE layer with a reduced intermediate size and the vocabulary is reduced to 1008:
    V enters only the first tree's head GEMM, not the K/V, g and last hidden row compared here, and the target's layers not at all."""
    if name in DRAFTS:
        num_q, bias, theta, eps = DRAFTS[name]
        pair = make_pair(W["D"], W["H"], W["I"], W["V"], W["P"], W["DP"], num_q, bias, theta, eps, seed=400 + num_q)
        assert pair[0].engine.lib.vispec_qkv_rope_fused(3 * W["D"])  # the one-launch BIG_ROPE_KV form is live at this width
        return pair
    D, H, I, bias, theta, eps = REAL[name]
    return make_pair(D, H, I, 1008, 4096, 1024, 2, bias, theta, eps, seed=500, target_I=1024)


@pytest.fixture(scope="module")
def pairs():
    """name -> build_pair(name), one configuration alive at a time (the tests below are ordered so that each is built once)."""
    import gc
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()
            gc.collect()
            torch.cuda.empty_cache()
            cache[name] = build_pair(name)
        return cache[name]
    yield get
    cache.clear()
    gc.collect()
    torch.cuda.empty_cache()


def test_row_edge_table_covers_every_switch():
    """ROW_EDGE reaches every M value in WANT for every prefill-GEMM form, the skinny stays just below them and every prompt layout and draft
    variant listed above, all derived from the masks the way the host plan derives them."""
    from vispec_amd import lib
    assert lib.load().vispec_qkv_rope_fused(3 * W["D"])
    got = dict(text=set(), runs=set(), Lc=set(), plain=set(), kv=set(), rope_kv=set(), o_first=set(), num_q=set(), runs_per_prompt=set(),
               sep=set())
    layouts = set()
    for name, (var, parts) in ROW_EDGE.items():
        L, mask = token_mask(parts)
        num_q = DRAFTS[var][0]
        texts, runs, Lc = prefill_plan(mask, L, num_q)
        big, o_first = gemm_rows(texts, runs, Lc)
        got["text"] |= set(texts)
        got["runs"] |= set(runs)
        got["Lc"].add(Lc)
        for f in ("plain", "kv", "rope_kv"):
            got[f] |= set(big[f])
        got["o_first"].add(o_first)
        got["num_q"].add(num_q)
        got["runs_per_prompt"].add(len(runs))
        if len(runs) > 1:
            got["sep"] |= set(texts[1:len(runs)])  # the text segments BETWEEN image runs
        if mask is None and L >= BIG_MIN_ROWS:
            layouts.add("no_image")
        elif mask is not None and mask[-1]:
            layouts.add("image_last")
        if DRAFTS[var][1]:
            layouts.add("bias")
        else:
            layouts.add("no_bias")
        if DRAFTS[var][2] == 1e6 and DRAFTS[var][3] == 1e-6:
            layouts.add("theta1e6_eps1e-6")
    assert set(WANT["text"]) <= got["text"] and max(got["text"]) >= WANT["text_ge"]
    assert set(WANT["runs"]) <= got["runs"] and max(got["runs"]) >= WANT["runs_ge"]
    assert set(WANT["Lc"]) <= got["Lc"]
    # per form: BIG_PLAIN takes the text segments of >= 64 rows (63 stays skinny), BIG_KV the runs of >= 64, BIG_ROPE_KV Lc >= 64
    assert 63 in got["text"] and 63 not in got["plain"] and {64, 65, 127, 128, 129} <= got["plain"] and max(got["plain"]) >= WANT["text_ge"]
    assert 63 in got["runs"] and 63 not in got["kv"] and {64, 65, 128, 129} <= got["kv"] and max(got["kv"]) >= WANT["runs_ge"]
    assert 63 in got["Lc"] and 63 not in got["rope_kv"] and {64, 65, 96, 97, 128, 129} <= got["rope_kv"]
    # the skinny q|k|v's last chunk starts at 32 (Lc 64), 64 (Lc 65 / 96), 96 (Lc 97 / 128) and 128 (Lc 129): a full and a 1-row chunk
    assert {32, 64, 96, 128} <= got["o_first"]
    assert got["num_q"] >= {2, 3, 5} and {1, 2, 4} <= got["runs_per_prompt"]
    assert 1 in got["sep"] and max(got["sep"]) >= BIG_MIN_ROWS  # runs split by one text row and by a BIG_PLAIN segment
    assert {"no_image", "image_last", "bias", "no_bias", "theta1e6_eps1e-6"} <= layouts


@pytest.mark.parametrize("prompt", list(ROW_EDGE))
def test_row_edges_against_the_oracle(pairs, prompt):
    var, parts = ROW_EDGE[prompt]
    sm, od, _, head_w = pairs(var)
    hidden, embeds, mask, ids = make_inputs(W["D"], parts, seed=len(prompt) * 31 + sum(n for _, n in parts))
    check_prefill(sm, od, head_w, hidden, embeds, mask, ids)


def assert_rerun_bit_identical(eng, first, other):
    """Prompt A, prompt B, prompt A again on one engine: the second A leaves exactly what the first did (no state or scratch leaks)."""
    a1 = run_prefill(eng, *first)
    run_prefill(eng, *other)
    a2 = run_prefill(eng, *first)
    assert a1["Lc"] == a2["Lc"]
    for key in ("kv", "g", "last"):
        assert torch.equal(a1[key], a2[key]), key


def test_row_edge_rerun_is_bit_identical(pairs):
    a = make_inputs(W["D"], ROW_EDGE["four_runs_bias"][1], seed=11)
    b = make_inputs(W["D"], ROW_EDGE["lc128_bias"][1], seed=12)
    assert_rerun_bit_identical(pairs("q3_bias")[0].engine, a, b)


# ------------------------------------------------------------------------------------------------------------------- B. cohort member
def test_cohort_member_prefill(pairs):
    """A cohort member has its own prefill scratch but shares xq / gemm_part and 32-row tiles of the leader's activation workspaces: the
    same prompt leaves bit-identical K/V, g and last hidden row on both, and the member's prefill changes nothing the leader's left."""
    sm = pairs("q3_bias")[0]
    lead_eng = sm.engine
    x = make_inputs(W["D"], ROW_EDGE["four_runs_bias"][1], seed=31)
    lead = run_prefill(lead_eng, *x)
    kv_before = lead_eng.draft_kv.clone()
    mb = sm.make_cohort_member()
    try:
        got = run_prefill(mb.engine, *x)
        assert got["Lc"] == lead["Lc"]
        for key in ("kv", "g", "last"):
            assert torch.equal(got[key], lead[key]), key
        assert torch.equal(lead_eng.draft_kv, kv_before)
        assert torch.equal(lead_eng.buffer("draft_g", (1, W["D"])), lead["g"])
        assert torch.equal(lead_eng.buffer("draft_last", (16, W["D"]))[:1], lead["last"])
    finally:
        mb.engine.close()  # hands the activation tile back to the leader


# ---------------------------------------------------------------------------------------------------------------------- C. real widths
REAL = {  # the real draft of every BASELINE model family: (D, H, I, q|k|v bias, rope_theta, rms_norm_eps)
    "llava7b": (4096, 32, 11008, False, 1e4, 1e-5),
    "llava13b": (5120, 40, 13824, False, 1e4, 1e-5),
    "qwen7b": (3584, 28, 18944, True, 1e6, 1e-6),
}
# the prompt shapes of bench._make_request, plus one with a text segment of >= 64 rows before the image
LLAVA = [("t", 48), ("i", 2144), ("t", 512)]                                       # llava7b / llava13b: L = 2704
QWEN = [("t", 48), ("i", 256), ("t", 96), ("i", 256), ("t", 96), ("i", 256), ("t", 96), ("i", 256), ("t", 224)]  # qwen7b: L = 1584
QWEN_FP8 = [("t", 48), ("i", 1564), ("t", 512)]                                    # qwen7b-fp8 (one 68 x 92 grid): L = 2124
LONG_TEXT = [("t", 130), ("i", 200), ("t", 70)]
REAL_PROMPTS = {"llava7b": dict(baseline=LLAVA, long_text=LONG_TEXT), "llava13b": dict(baseline=LLAVA, long_text=LONG_TEXT),
                "qwen7b": dict(baseline=QWEN, fp8_shape=QWEN_FP8, long_text=LONG_TEXT)}


@pytest.mark.parametrize("width,prompt", [(w, p) for w, ps in REAL_PROMPTS.items() for p in ps])
def test_real_width_against_the_oracle(pairs, width, prompt):
    sm, od, od32, head_w = pairs(width)
    parts = REAL_PROMPTS[width][prompt]
    hidden, embeds, mask, ids = make_inputs(sm.engine.dcfg.hidden_size, parts, seed=600 + len(prompt))
    check_prefill(sm, od, head_w, hidden, embeds, mask, ids, od32=od32)


@pytest.mark.parametrize("width", ["qwen7b", "llava7b", "llava13b"])  # (qwen7b first: still built by the last test above)
def test_real_width_rerun_is_bit_identical(pairs, width):
    eng = pairs(width)[0].engine
    D, ps = eng.dcfg.hidden_size, REAL_PROMPTS[width]
    assert_rerun_bit_identical(eng, make_inputs(D, ps["baseline"], seed=21), make_inputs(D, ps["long_text"], seed=22))
