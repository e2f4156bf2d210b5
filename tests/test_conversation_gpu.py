"""Conversation turns: a finished request handed back as a PromptPrefix (return_prefix=True on specgenerate / specgenerate_cohort /
specgenerate_stream), the per-request hidden-row log behind it (Engine.set_hidden_log / hidden_log: one more store in the post_accept launch
of every round) and PromptPrefix.truncated, on the tiny models.

Arithmetic class that these tests pin down: the prompt rows of a returned prefix are the bytes the request started with; the generated
rows' K/V are the cache's bytes at the finish and their hidden rows are, byte for byte, the rows the rounds staged for the draft — all
from the verify kernels, held to the oracle's bf16 forward within the bar of the verify-forward comparisons (2^-6 of the tensor's largest
magnitude).  In cohorts of up to four a request's prefix is bit-equal to its solo run's; in cohorts of five to eight it does not depend on
what shares the weight pass.  Token equality of a turn on a returned prefix with the oracle's run on the full ids is asserted below as an
OBSERVATION on this structured (wide-margin) pair, not as an invariant of the feature."""
import ctypes as C
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from helpers import T, synth, vo  # noqa: E402
from test_loop_gpu import IMG_TOK, build, build_qwen  # noqa: E402  (the tiny-model builders)
from test_prefix_gpu import close, oracle_prefill  # noqa: E402
from vispec_amd import lib as L  # noqa: E402
from vispec_amd.engine import DraftConfig, TargetConfig  # noqa: E402
from vispec_amd.model import PromptPrefix, SpecModel  # noqa: E402
from vispec_amd.model.spec_model_ours import specgenerate_cohort, specgenerate_stream  # noqa: E402
from vispec_amd.model.target import SyntheticVision  # noqa: E402

CANARY = -1536.0  # exact in bf16
i16 = lambda t: t.view(torch.int16)
ID_HI = 600  # prompt ids stay far below the placeholder id: the successor pair then never generates one
GEN = dict(log=True, return_acceptance_len=True, return_prefix=True)


def t_ids(a):
    return torch.from_numpy(np.asarray(a, np.int64))[None]


def image_prompt(rng, n_pre, n_img, n_post, img_tok=IMG_TOK):
    return np.concatenate([rng.integers(3, ID_HI, n_pre), np.full(n_img, img_tok), rng.integers(3, ID_HI, n_post)]).astype(np.int64)


def same_prefix(a, b, what=""):
    assert isinstance(a, PromptPrefix) and isinstance(b, PromptPrefix), what
    assert a.rows == b.rows and torch.equal(a.ids, b.ids), what
    assert torch.equal(i16(a.store), i16(b.store)), f"{what}: K/V store"
    assert torch.equal(i16(a.hidden), i16(b.hidden)), f"{what}: hidden rows"
    assert torch.equal(i16(a.emb), i16(b.emb)), f"{what}: embeddings"
    assert (a.image_mask is None) == (b.image_mask is None) and (a.image_mask is None or torch.equal(a.image_mask.cpu(), b.image_mask.cpu())), what
    assert (a.pos3 is None) == (b.pos3 is None) and (a.pos3 is None or torch.equal(a.pos3.cpu(), b.pos3.cpu())), what


def same_results(got, want, what=""):
    assert len(got) == len(want) == 5, what
    assert torch.equal(got[0], want[0]) and (got[1], got[2], got[3]) == (want[1], want[2], want[3]), what
    assert got[4].rows == got[0].shape[1], what
    same_prefix(got[4], want[4], what)


@pytest.fixture(scope="module")
def tiny():
    """Tiny LLaVA leader with five cohort members, six prompts of 12..30 rows (two with an image run) and their ragged budgets."""
    sm, ot, od = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    models = [sm] + [sm.make_cohort_member() for _ in range(5)]
    rng = np.random.default_rng(2024)
    reqs = [(t_ids(image_prompt(rng, 5, 9, 6)), dict(pixel_values=(9, 7))), (t_ids(rng.integers(3, ID_HI, 12)), {}),
            (t_ids(rng.integers(3, ID_HI, 30)), {}), (t_ids(image_prompt(rng, 4, 11, 8)), dict(pixel_values=(11, 8))),
            (t_ids(rng.integers(3, ID_HI, 17)), {}), (t_ids(rng.integers(3, ID_HI, 25)), {})]
    return SimpleNamespace(models=models, ot=ot, od=od, reqs=reqs, budgets=[12, 5, 20, 9, 16, 7], solo={})


def solo(env, i):
    """Request i alone on the leader with return_prefix: computed once, shared, never modified."""
    if i not in env.solo:
        ids, kw = env.reqs[i]
        env.solo[i] = env.models[0].specgenerate(ids, max_new_tokens=env.budgets[i], **GEN, **kw)
        assert len(env.solo[i]) == 5
    return env.solo[i]


def oracle_embeddings(ot, ids, feats_of_runs, img_tok=IMG_TOK):
    """The merged embeddings [L, D] of ids for the oracle: the target's table, the image rows replaced by the features."""
    emb = ot.w["model.embed_tokens.weight"][ids].copy()
    mask = ids == img_tok
    if mask.any():
        emb[mask] = feats_of_runs
    return emb, mask


def synthetic_features(D, n, seed):
    return SyntheticVision(D).features(n, seed, "cpu", torch.bfloat16).float().numpy()


# ------------------------------------------------------------------------------------------------------------ 1. the log = the staged rows
def drive_rounds(sm, ids, rounds, forced=(), **gen):
    """A request start with return_prefix on, then rounds by hand; after each one the log's rows [n, n + a] against accept_hidden[:a + 1]
    (the rows the same launch staged for the draft), bit for bit.  n = n_ctx - a - 1 of the state read-back (the round's n_prev).
    forced: accept lengths scripted for extra rounds behind the free ones.  -> the accept lengths."""
    eng = sm.engine
    D = eng.tcfg.hidden_size
    sm._start_request(ids, None, {}, max_new_tokens=200, return_prefix=True, **gen)
    L0, accs = ids.shape[1], []
    pos = L0
    for fa in [-1] * rounds + list(forced):
        eng.verify_accept(fa)
        eng.draft_round()
        st = eng.state()
        a = st["accept_len"]
        n = st["n_ctx"] - a - 1
        assert n == pos and not st["done"] and (fa < 0 or a == fa)
        got = eng.hidden_log(n, a + 1)
        want = eng.buffer("accept_hidden", (16, D))[:a + 1]
        assert tuple(got.shape) == (a + 1, D) and got.dtype == torch.bfloat16
        assert torch.equal(i16(got), i16(want)), (len(accs), n, a)
        assert got.float().abs().max() > 0
        pos = st["n_ctx"]
        accs.append(a)
    # every generated position was written exactly by the round that committed it: the log of [L, n_ctx) is still the rounds' rows
    assert tuple(eng.hidden_log(L0, pos - L0).shape) == (pos - L0, D)
    print("accept lengths", accs)
    return accs


@pytest.mark.parametrize("gen", [dict(), dict(temperature=1.0, seed=3)], ids=["greedy", "t1"])
def test_log_rows_are_the_staged_rows_bit_for_bit(tiny, gen):
    accs = drive_rounds(tiny.models[0], tiny.reqs[2][0], 6, forced=(0, 2) if not gen else (), **gen)
    free = accs[:6]
    assert min(free) == 0 and max(free) >= 2, free


def test_log_rows_with_a_40_node_tree():
    sm, _, _ = build(50, 60, True, total_token=40)
    assert sm.engine.total_token == 40
    ids = t_ids(np.random.default_rng(40).integers(3, ID_HI, 19))
    accs = drive_rounds(sm, ids, 6)
    assert min(accs) == 0 and max(accs) >= 2, accs


def test_log_rows_wider_than_one_pass_of_the_copy_loop():
    """D = 2560 (20 heads x 128): 256 threads x 8 elements cover 2048 per pass, so the last 512 elements of a row go through a second
    pass of the loop that also stores the log row.  A 2-layer structured pair made for this test alone."""
    D, H, I, V, NL, P = 2560, 20, 1024, 1008, 2, 256
    tw = synth.make_target_weights(D, H, I, V, NL, seed=52, structured=True)
    dw = synth.make_draft_weights(D, H, I, V, num_q=2, seed=62, structured=True, target_embed=tw["model.embed_tokens.weight"], rho=0.25)
    tcfg = TargetConfig(hidden_size=D, num_heads=H, num_kv_heads=H, intermediate_size=I, vocab_size=V, num_layers=NL,
                        max_position_embeddings=P, architectures=("LlamaForCausalLM",))
    dcfg = DraftConfig(hidden_size=D, num_heads=H, intermediate_size=I, vocab_size=V, max_position_embeddings=P)
    sm = SpecModel.from_weights(tcfg, dcfg, tw, dw, num_q=2)
    ids = t_ids(np.random.default_rng(41).integers(3, ID_HI, 14))
    accs = drive_rounds(sm, ids, 6)
    assert min(accs) == 0 and max(accs) >= 2, accs
    n = sm.engine.state()["n_ctx"]
    rows = sm.engine.hidden_log(14, n - 14).float()
    assert (rows[:, 2048:].abs().amax(dim=1) > 0).all(), "the second pass of every row was stored"


# ----------------------------------------------------------------------------------------------------- 2. the returned prefix vs the oracle
def test_returned_prefix_against_the_oracle(tiny):
    sm, ot = tiny.models[0], tiny.ot
    ids, kw = tiny.reqs[0]
    Ln = ids.shape[1]
    out, _, _, _, pfx = solo(tiny, 0)
    P = out.shape[1]
    assert isinstance(pfx, PromptPrefix) and pfx.rows == P > Ln + 8 and torch.equal(pfx.ids, out.cpu()) and pfx.weights is sm.base_model.w
    NL2, Hk, hd = 2 * T["NL"], T["H"], T["D"] // T["H"]
    assert tuple(pfx.store.shape) == (NL2, Hk, P, hd) and pfx.store.is_contiguous() and tuple(pfx.hidden.shape) == tuple(pfx.emb.shape) == (P, T["D"])
    assert int(pfx.image_mask.sum()) == 9 and not pfx.image_mask[:, Ln:].any() and pfx.pos3 is None and pfx.draft_emb
    kv = sm.engine.target_kv
    lo, hi = pfx.store.data_ptr(), pfx.store.data_ptr() + pfx.store.numel() * 2
    assert hi <= kv.data_ptr() or lo >= kv.data_ptr() + kv.numel() * 2, "the store aliases no cache"
    # generated rows: the oracle's target forward over the returned ids, the bar of the verify-forward rows
    toks = out[0].cpu().numpy()
    emb, _ = oracle_embeddings(ot, toks, synthetic_features(T["D"], 9, 7))
    _, hid, okv = oracle_prefill(ot, emb, None, T["NL"], T["H"], T["max_pos"], hd)
    close(pfx.hidden[Ln:].float().cpu().numpy(), hid[Ln:])
    close(pfx.store[:, :, Ln:].float().cpu().numpy(), okv[:, :, Ln:])
    assert torch.equal(i16(pfx.emb[Ln:]), i16(sm.base_model.get_input_embeddings()(out[0, Ln:]).to(torch.bfloat16)))
    # prompt rows: bit-equal to what an identical request start produces
    hidden, _, _, _ = sm._start_request(ids, None, dict(kw), max_new_tokens=16)
    torch.cuda.synchronize()
    assert torch.equal(i16(pfx.hidden[:Ln]), i16(hidden))
    assert torch.equal(i16(pfx.store[:, :, :Ln]), i16(sm.engine.target_kv[:, 0, :, :Ln]))
    assert torch.equal(i16(pfx.emb[:Ln]), i16(sm._embed_prompt(ids, None, dict(kw))[1]))


# ------------------------------------------------------------------------------------------------------------- 3. a three-turn conversation
def test_three_turns_on_returned_prefixes(tiny):
    """Turn k + 1 = the previous turn's ids + 6 new ids on the previous turn's returned prefix.  Tokens and accept lengths equal the
    oracle's run on the full ids of each turn — an equality that holds on THIS structured pair (wide margins), not an invariant: the prefix
    rows come from the verify kernels, the oracle prefills them.  The vision front-end runs for turn 1 only."""
    sm, ot, od = tiny.models[0], tiny.ot, tiny.od
    vision, calls = sm.base_model.vision, []
    inner = vision.features
    vision.features = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    feats = synthetic_features(T["D"], 9, 7)
    rng = np.random.default_rng(77)
    try:
        ids, pfx, prev = tiny.reqs[0][0], None, None
        for turn in range(3):
            if turn:
                ids = torch.cat([prev[0].cpu(), t_ids(rng.integers(3, ID_HI, 6))], dim=1)
            kw = dict(pixel_values=(9, 7)) if pfx is None else dict(prefix=pfx)
            got = sm.specgenerate(ids, max_new_tokens=8, **GEN, **kw)
            assert len(calls) == 1, f"turn {turn + 1}"
            ids_np = ids[0].numpy()
            emb, mask = oracle_embeddings(ot, ids_np, feats)
            o_out, o_new, o_idx, o_acc = vo.specgenerate(ot, od, ids_np, inputs_embeds=emb, image_mask=mask, max_new_tokens=8, max_pos=T["max_pos"])
            np.testing.assert_array_equal(got[0][0].cpu().numpy(), o_out)  # (on this pair only)
            assert got[3] == o_acc and got[1] == o_new
            new = got[4]
            assert new.rows == got[0].shape[1] and torch.equal(new.ids, got[0].cpu()) and int(new.image_mask.sum()) == 9
            if pfx is not None:
                assert torch.equal(i16(new.hidden[:pfx.rows]), i16(pfx.hidden)) and torch.equal(i16(new.emb[:pfx.rows]), i16(pfx.emb))
                assert torch.equal(i16(new.store[:, :, :pfx.rows]), i16(pfx.store)), "the prefix rows are the donor's bytes"
            pfx, prev = new, got
        assert pfx.rows >= tiny.reqs[0][0].shape[1] + 3 * 8 + 12
    finally:
        del vision.features


# --------------------------------------------------------------------------------------------------------------- 4. cutting at a boundary
def test_a_turn_on_a_truncated_prefix(tiny):
    sm = tiny.models[0]
    out, _, _, _, pfx1 = solo(tiny, 0)
    Ln = tiny.reqs[0][0].shape[1]
    r = Ln + 5
    assert Ln < r < pfx1.rows
    cut = pfx1.truncated(r)
    assert cut.rows == r and cut.store.is_contiguous() and cut.store.data_ptr() != pfx1.store.data_ptr()
    hand = PromptPrefix(pfx1.store[:, :, :r].contiguous(), pfx1.hidden[:r].contiguous(), pfx1.emb[:r].contiguous(), pfx1.draft_emb,
                        pfx1.image_mask[:, :r].contiguous(), pfx1.ids[:, :r].contiguous(), weights=pfx1.weights)
    ids = torch.cat([pfx1.ids[:, :r], t_ids(np.random.default_rng(5).integers(3, ID_HI, 6))], dim=1)
    a = sm.specgenerate(ids, max_new_tokens=10, prefix=cut, **GEN)
    b = sm.specgenerate(ids, max_new_tokens=10, prefix=hand, **GEN)
    same_results(a, b, "truncated() against a hand-made prefix of the same rows")
    with pytest.raises(ValueError):
        pfx1.truncated(8)  # inside the image run (rows 5..13)
    with pytest.raises(ValueError):
        pfx1.truncated(pfx1.rows + 1)


# -------------------------------------------------------------------------------------------------------------------- 5. Qwen2.5-VL M-RoPE
def test_qwen_mrope_turn_on_a_returned_prefix():
    sm, ot, od, IMG = build_qwen()
    Q = synth.QWEN_TINY
    rng = np.random.default_rng(17)
    grids = [(1, 6, 8)]  # -> 12 merged image tokens
    ids_np = image_prompt(rng, 4, 12, 6, IMG)
    Ln = len(ids_np)
    feats = synth.bf16_grid(rng.standard_normal((12, Q["D"]), dtype=np.float32) * 0.05)
    kw = dict(pixel_values=torch.from_numpy(feats).to(torch.bfloat16).cuda(), image_grid_thw=torch.tensor(grids))
    out1, _, _, _, pfx = sm.specgenerate(t_ids(ids_np), max_new_tokens=10, **GEN, **kw)
    pos3, delta = synth.qwen_rope_index(ids_np, IMG, grids)
    assert delta < 0 and sm._rope_delta == delta
    P = pfx.rows
    assert P == out1.shape[1] > Ln and tuple(pfx.pos3.shape) == (3, P) and np.array_equal(pfx.pos3[:, :Ln].numpy(), pos3)
    for c in range(3):
        assert torch.equal(pfx.pos3[c, Ln:].long(), torch.arange(Ln, P) + delta)
    assert set(pfx.grids) == {"image_grid_thw"}
    # turn 2 passes PromptPrefix.extend's position assert (it would raise) and equals the oracle's stream for the full ids (on this pair)
    ids2 = torch.cat([out1.cpu(), t_ids(rng.integers(3, ID_HI, 6))], dim=1)
    got = sm.specgenerate(ids2, max_new_tokens=8, prefix=pfx, **GEN)
    ids2_np = ids2[0].numpy()
    pos3_2, delta2 = synth.qwen_rope_index(ids2_np, IMG, grids)
    assert delta2 == delta and np.array_equal(pos3_2[:, :P], pfx.pos3.numpy())
    emb, mask = oracle_embeddings(ot, ids2_np, feats, IMG)
    o_out, o_new, _, o_acc = vo.specgenerate(ot, od, ids2_np, inputs_embeds=emb, image_mask=mask, max_new_tokens=8, max_pos=Q["max_pos"],
                                             position_ids=pos3_2, rope_delta=delta2)
    np.testing.assert_array_equal(got[0][0].cpu().numpy(), o_out)
    assert got[3] == o_acc and got[1] == o_new
    pfx2 = got[4]
    assert pfx2.rows == got[0].shape[1] and torch.equal(pfx2.pos3[:, :P], pfx.pos3)
    assert torch.equal(pfx2.pos3[0, P:].long(), torch.arange(P, pfx2.rows) + delta)


# ------------------------------------------------------------------------------------------------------------------------------ 6. cohorts
@pytest.mark.parametrize("n", [2, 4])
def test_cohort_prefixes_equal_the_solo_runs(tiny, n):
    got = specgenerate_cohort(tiny.models[:n], tiny.reqs[:n], max_new_tokens=tiny.budgets[:n], return_prefix=True)
    for t in range(n):
        same_results(got[t], solo(tiny, t), f"request {t} of a cohort of {n}")


def test_cohort_of_five_prefix_does_not_depend_on_company_or_slot(tiny):
    """The c8 class: requests 0, 2, 3 and 4 next to request 1 in slots 0, 2, 3, 4, then next to request 5 in slots 4, 1, 0, 2."""
    m = tiny.models
    a = specgenerate_cohort(m[:5], [tiny.reqs[i] for i in (0, 1, 2, 3, 4)], max_new_tokens=[tiny.budgets[i] for i in (0, 1, 2, 3, 4)], return_prefix=True)
    order = (3, 2, 4, 5, 0)
    b = specgenerate_cohort(m[:5], [tiny.reqs[i] for i in order], max_new_tokens=[tiny.budgets[i] for i in order], return_prefix=True)
    for i in (0, 2, 3, 4):
        same_results(a[i], b[order.index(i)], f"request {i}")


def test_a_frozen_request_keeps_its_rows_while_its_partners_run_on(tiny):
    m, (r1, r2) = tiny.models[:2], (tiny.reqs[1], tiny.reqs[2])
    first = specgenerate_cohort(m, [r1, r2], max_new_tokens=[5, 24], return_prefix=True)  # request 1 ends rounds before its partner
    last = specgenerate_cohort(m, [r1, r2], max_new_tokens=[5, 1], return_prefix=True)    # ... and here it finishes last
    assert first[0][2] < first[1][2] and last[0][2] >= last[1][2]
    assert first[0][4].rows == first[0][0].shape[1] < first[1][4].rows
    same_results(first[0], last[0], "the request that froze early")
    same_results(first[0], solo(tiny, 1), "against its solo run")


# ------------------------------------------------------------------------------------------------------------------------------- 7. stream
def test_stream_harvests_a_prefix_before_the_slot_is_refilled(tiny):
    order = [2, 0, 4, 1, 5, 3]  # long requests first: the slots are refilled by shorter ones
    got = specgenerate_stream(tiny.models[:3], [tiny.reqs[i] for i in order], max_new_tokens=[tiny.budgets[i] for i in order], return_prefix=True)
    assert len(got) == 6
    for k, i in enumerate(order):
        assert isinstance(got[k][-1], PromptPrefix) and got[k][-1].rows == got[k][0].shape[1]
        same_results(got[k], solo(tiny, i), f"request {i}")
    two = specgenerate_stream(tiny.models[:3], [tiny.reqs[i] for i in (1, 4)], max_new_tokens=[tiny.budgets[i] for i in (1, 4)], return_prefix=True)
    same_results(two[0], solo(tiny, 1), "requests <= slots")  # (the plain-cohort route of the stream entry)
    same_results(two[1], solo(tiny, 4), "requests <= slots")


# --------------------------------------------------------------------------------------------------------------------------- 8. off is off
def test_off_is_off_and_the_flag_is_part_of_the_graph_key(tiny):
    sm, _, _ = build(50, 60, True)
    with pytest.raises(L.VispecError, match="never enabled"):
        sm.engine.hidden_log(0, 1)  # an engine that never switched the log on has none
    ids = tiny.reqs[4][0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        off = sm.specgenerate(ids, max_new_tokens=16, log=True, return_acceptance_len=True)
        s.synchronize()
        c0 = sm.engine.graph_stats()["captures"]
        assert len(off) == 4 and torch.is_tensor(sm.specgenerate(ids, max_new_tokens=16))  # a bare call still returns the ids alone
        s.synchronize()
        assert sm.engine.graph_stats()["captures"] == c0  # same key: replayed
        with pytest.raises(L.VispecError, match="never enabled"):
            sm.engine.hidden_log(0, 1)
        on = sm.specgenerate(ids, max_new_tokens=16, **GEN)
        s.synchronize()
        c1 = sm.engine.graph_stats()["captures"]
        assert len(on) == 5 and c1 > c0  # another key: captured again, never the flag-off graph replayed
        assert torch.equal(on[0], off[0]) and on[1:4] == off[1:4] and on[4].rows == on[0].shape[1]
        again = sm.specgenerate(ids, max_new_tokens=16, log=True, return_acceptance_len=True)
        s.synchronize()
        assert len(again) == 4 and sm.engine.graph_stats()["captures"] == c1  # ... and the flag-off graphs are still cached
        assert torch.equal(again[0], off[0])
        both = sm.specgenerate(ids, max_new_tokens=16, log=True, return_acceptance_len=True, return_logprobs=True, return_prefix=True)
        s.synchronize()
        assert len(both) == 6 and isinstance(both[-1], PromptPrefix) and torch.is_tensor(both[-2]) and both[-2].dtype == torch.float32
        assert both[-2].shape == (1, both[0].shape[1] - ids.shape[1])
        same_prefix(both[-1], on[4], "with the log-probabilities on as well")
        ids_only, pfx = sm.specgenerate(ids, max_new_tokens=16, return_prefix=True)
        same_prefix(pfx, on[4], "a bare call with return_prefix")
        # the AR baseline never carries the log, even right behind a request that did
        ar = sm.baseline_generate(ids, max_new_tokens=8)
        assert torch.is_tensor(ar) and torch.equal(ar[0, :ids.shape[1] + 8], off[0][0, :ids.shape[1] + 8])
    m = tiny.models
    for got in (specgenerate_cohort(m[:2], tiny.reqs[:2], max_new_tokens=4),
                specgenerate_stream(m[:2], tiny.reqs[:3], max_new_tokens=4)):
        assert all(len(g) == 4 and torch.is_tensor(g[0]) for g in got)
    got = specgenerate_cohort(m[:2], tiny.reqs[:2], max_new_tokens=tiny.budgets[:2], return_logprobs=True, return_prefix=True)
    for t in range(2):
        assert len(got[t]) == 6 and isinstance(got[t][5], PromptPrefix) and isinstance(got[t][4], np.ndarray)
        same_prefix(got[t][5], solo(tiny, t)[4], f"request {t}")


# ---------------------------------------------------------------------------------------------------------------------------- 9. refusals
def test_a_generated_placeholder_id_gives_none_and_a_warning(tiny, monkeypatch):
    sm = tiny.models[0]
    ids = tiny.reqs[4][0]
    want = solo(tiny, 4)
    # an id the request is known to generate (and its prompt does not hold) becomes a placeholder id of this model
    tid = next(t for t in want[0][0, ids.shape[1]:].tolist() if t not in ids[0].tolist())
    monkeypatch.setattr(sm, "_visual_token_ids", lambda: (tid,))
    with pytest.warns(RuntimeWarning, match="placeholder"):
        got = sm.specgenerate(ids, max_new_tokens=tiny.budgets[4], **GEN)
    assert got[4] is None and torch.equal(got[0], want[0]) and got[1:4] == want[1:4]  # the other outputs are unaffected
    monkeypatch.undo()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        same_results(sm.specgenerate(ids, max_new_tokens=tiny.budgets[4], **GEN), want)


def test_get_hidden_log_refuses_a_range_that_leaves_the_log(tiny):
    eng = tiny.models[0].engine
    solo(tiny, 0)  # (the log exists)
    lib, D, S = eng.lib, T["D"], T["max_pos"]
    dst = torch.full((8, D), CANARY, dtype=torch.bfloat16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for row0, rows in ((S - 2, 4), (S, 1), (-1, 2), (0, S + 1), (3, -1), (2 ** 31 - 2, 4)):
        assert lib.vispec_get_hidden_log(eng.h, st, C.c_void_p(dst.data_ptr()), row0, rows) != 0, (row0, rows)
        assert "get_hidden_log:" in (lib.vispec_last_error() or b"").decode()
        with pytest.raises(L.VispecError):
            eng.hidden_log(row0, rows)
    assert lib.vispec_get_hidden_log(eng.h, st, None, 0, 2) != 0
    torch.cuda.synchronize()
    assert (dst == CANARY).all(), "a refused call writes nothing"
    L.check(lib.vispec_get_hidden_log(eng.h, st, C.c_void_p(dst.data_ptr()), S - 4, 4))  # the last rows of the log are in range
    torch.cuda.synchronize()
    assert (dst[4:] == CANARY).all()
    assert tuple(eng.hidden_log(5, 0).shape) == (0, D)
