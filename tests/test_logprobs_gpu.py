"""Per-token target log-probabilities (return_logprobs=True) on the tiny pair: the HIP kernel against float64 on the same bf16 logits,
the loops against the oracle target's teacher-forced forward, alignment / truncation, the untouched default, cohorts, streams, the
prefill flavours, determinism and the AR cross-check."""
import math
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from helpers import T, vo  # noqa: E402
from logprob_helpers import bf16_round, kernel_bar, loop_bar, oracle_logprobs, ref_token_logprob  # noqa: E402
from vispec_amd import synth  # noqa: E402
from vispec_amd.engine import DraftConfig, TargetConfig  # noqa: E402
from vispec_amd.model import SpecModel  # noqa: E402
from vispec_amd.model.spec_model_ours import specgenerate_cohort, specgenerate_stream  # noqa: E402


def build(seed_t=50, seed_d=60, eos=None, **kw):
    tw = synth.make_target_weights(T["D"], T["H"], T["I"], T["V"], T["NL"], seed=seed_t, structured=True)
    dw = synth.make_draft_weights(T["D"], T["H"], T["I"], T["V"], num_q=2, seed=seed_d, structured=True,
                                  target_embed=tw["model.embed_tokens.weight"], rho=0.25)
    extra = {} if eos is None else {"eos_token_id": eos}
    tcfg = TargetConfig(hidden_size=T["D"], num_heads=T["H"], num_kv_heads=T["H"], intermediate_size=T["I"], vocab_size=T["V"],
                        num_layers=T["NL"], max_position_embeddings=T["max_pos"], architectures=("LlamaForCausalLM",), **extra)
    dcfg = DraftConfig(hidden_size=T["D"], num_heads=T["H"], intermediate_size=T["I"], vocab_size=T["V"], max_position_embeddings=T["max_pos"])
    sm = SpecModel.from_weights(tcfg, dcfg, tw, dw, num_q=2, **kw)
    ot = vo.TargetLlama(vo.TargetConfig(T["D"], T["H"], T["H"], T["I"], T["V"], T["NL"], T["max_pos"]), tw, bf16=True)
    od = vo.DraftModel(vo.DraftConfig(T["D"], T["H"], T["I"], T["V"], T["max_pos"], num_q=2), dw, bf16=True)
    return sm, ot, od


@pytest.fixture(scope="module")
def pair():
    return build()


@pytest.fixture(scope="module")
def g8(golden_dir):
    return np.load(os.path.join(golden_dir, "g8_loop.npz"))


def prompts(g8, n):
    """n ragged text prompts: the two fixture prompts, then random ones of mixed lengths."""
    rng = np.random.default_rng(91)
    out = [g8["succ0_ids"], g8["succ1_ids"]] + [rng.integers(3, T["V"] - 1, size=ln) for ln in (17, 9, 23, 12, 20, 7)]
    return [np.asarray(p, np.int64) for p in out[:n]]


def solo(sm, ids, **gen):
    """(tokens, accept lengths, logprobs) of one request alone."""
    toks, _, _, acc, lp = sm.specgenerate(torch.from_numpy(ids)[None], log=True, return_acceptance_len=True, return_logprobs=True, **gen)
    assert lp.dtype == torch.float32 and lp.shape == (1, toks.shape[1] - len(ids))
    return toks[0].cpu().numpy(), acc, lp[0].cpu().numpy()


def check_against_oracle(ot, toks, n_prompt, lp):
    want, scale = oracle_logprobs(ot, toks, n_prompt)
    assert len(lp) == len(toks) - n_prompt == len(want)
    assert np.all(np.isfinite(lp)) and np.all(lp <= 0)
    err = np.abs(lp.astype(np.float64) - want)
    print(f"logprobs vs oracle: max err {err.max():.3e}, bar {loop_bar(scale):.3e}, min logprob {want.min():.3f}")
    assert err.max() <= loop_bar(scale), (err.max(), loop_bar(scale))


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
def rows_for(V, rng):
    rows = {"random": bf16_round(rng.standard_normal(V).astype(np.float32) * 4.0)}
    dom = bf16_round(rng.standard_normal(V).astype(np.float32))
    dom[V // 3] = dom.max() + 40.0  # a single dominant logit, gap 40: log Z ~ 0
    rows["dominant"] = bf16_round(dom)
    rows["equal"] = np.full(V, 1.5, np.float32)  # logprob = -ln V
    return rows


@pytest.mark.parametrize("V", [7, 1000, 32000, 152064])
def test_row_kernel_against_float64_on_the_same_bf16_logits(pair, V):
    """token_logprob_row vs numpy float64 log_softmax of the bf16 values, bar = logprob_helpers.kernel_bar (derived from the kernel's one-pass
    running-max summation with 1024 threads: the re-derivation the summation shape asks for is in its docstring)."""
    eng = pair[0].engine
    eng.set_logprobs(True)
    eng.begin_request(np.arange(3, 8), 4)
    rng = np.random.default_rng(V)
    for name, row in rows_for(V, rng).items():
        toks = sorted({0, V - 1, V // 3, int(np.argmax(row)), int(np.argmin(row)), int(rng.integers(0, V))})
        dev = torch.from_numpy(row).cuda().to(torch.bfloat16)
        assert np.array_equal(dev.float().cpu().numpy(), row)  # the test's rows are bf16 values already
        for i, t in enumerate(toks):
            eng.token_logprob_row(dev, torch.tensor([t], dtype=torch.int32, device="cuda"), 10 + i)
        got = eng.logprobs(10 + len(toks))[10:]
        bar = kernel_bar(V, float(np.abs(row).max()))
        for t, v in zip(toks, got):
            want = ref_token_logprob(row, t)
            assert abs(float(v) - want) <= bar, (name, V, t, float(v), want, bar)
        if name == "equal":
            assert abs(float(got[0]) + math.log(V)) <= bar
        if name == "dominant":
            assert abs(float(eng.logprobs(10 + len(toks))[10 + toks.index(V // 3)])) <= bar + 1e-12
    eng.set_logprobs(False)


@pytest.mark.parametrize("forced", [0, "depth"])
def test_round_kernel_on_a_scripted_round_with_random_logits(pair, g8, forced):
    """One accept step with a scripted accept length (0 and depth) over RANDOM bf16 logits written into the verify buffer: the kernel
    behind the accept kernel writes lp[n + j + 1] from row sel[j] at tree_tokens[sel[j + 1]] (j < a) and lp[n + a + 1] from row sel[a] at
    next_token — each against float64 on the same bf16 row, every other entry of the log untouched."""
    sm = pair[0]
    eng = sm.engine
    ids = g8["succ0_ids"]
    sm.specgenerate(torch.from_numpy(ids)[None], max_new_tokens=1, return_logprobs=True)  # leaves a live tree and the flag on
    V, Tn = T["V"], eng.total_token
    fa = eng.depth if forced == "depth" else 0
    rng = np.random.default_rng(7 + fa)
    logits = bf16_round(rng.standard_normal((Tn, V)).astype(np.float32) * 3.0)
    eng.buffer("logits", (64, V))[:Tn].copy_(torch.from_numpy(logits).cuda().to(torch.bfloat16))
    eng.buffer("am", (64,), torch.int32)[:Tn].copy_(torch.from_numpy(np.argmax(logits, axis=1).astype(np.int32)).cuda())
    n = eng.state()["n_ctx"]
    cap = T["max_pos"] + 64
    before = eng.logprobs(cap)
    tree_tok = eng.tree()[0]
    eng.accept(fa)
    st = eng.state()
    a = st["accept_len"]
    assert a == fa and st["n_ctx"] == n + a + 1
    sel = eng.buffer("sel", (16,), torch.int32).cpu().numpy()
    after = eng.logprobs(cap)
    bar = kernel_bar(V, float(np.abs(logits).max()))
    for j in range(a + 1):
        tok = int(tree_tok[sel[j + 1]]) if j < a else st["next_token"]
        want = ref_token_logprob(logits[sel[j]], tok)
        assert abs(float(after[n + j + 1]) - want) <= bar, (j, float(after[n + j + 1]), want, bar)
    keep = np.ones(cap, bool)
    keep[n + 1:n + a + 2] = False
    np.testing.assert_array_equal(after[keep], before[keep])
    eng.set_logprobs(False)


# ---------------------------------------------------------------------------------------------------------------- 2. loop vs oracle
@pytest.mark.parametrize("gen", [dict(temperature=0.0), dict(temperature=1.0, seed=0), dict(temperature=6.0, top_k=4, seed=1)],
                         ids=["greedy", "t1", "t6_topk4"])
def test_loop_logprobs_match_the_oracles_teacher_forced_forward(pair, g8, gen):
    sm, ot, od = pair
    ids = g8["succ0_ids"]
    toks, acc, lp = solo(sm, ids, max_new_tokens=24, **gen)
    o_out, _, _, o_acc = vo.specgenerate(ot, od, ids, max_new_tokens=24, max_pos=T["max_pos"], **gen)
    np.testing.assert_array_equal(toks, o_out)
    assert acc == o_acc
    if gen.get("top_k"):
        assert min(o_acc) == 0  # a round that rejected every draft token: the residual-draw row is exercised
    check_against_oracle(ot, toks, len(ids), lp)


# ---------------------------------------------------------------------------------------------------------------- 3. alignment / truncation
def test_alignment_when_stopped_by_eos_budget_and_full_kv_cache(pair, g8):
    sm, ot, od = pair
    ids = g8["succ0_ids"]
    # budget
    toks, acc, lp = solo(sm, ids, max_new_tokens=9)
    assert len(toks) - len(ids) > 9 and len(lp) == len(toks) - len(ids)
    check_against_oracle(ot, toks, len(ids), lp)
    # EOS: a token the stream is known to produce becomes the eos id (the engine config carries it)
    full = vo.specgenerate(ot, od, ids, max_new_tokens=40, max_pos=T["max_pos"])[0]
    eos = int(full[len(ids) + 9])
    sm2, ot2, od2 = build(eos=eos)
    toks, acc, lp = solo(sm2, ids, max_new_tokens=40)
    o_out = vo.specgenerate(ot2, od2, ids, max_new_tokens=40, eos_token_id=eos, max_pos=T["max_pos"])[0]
    np.testing.assert_array_equal(toks, o_out)
    assert eos in toks[len(ids):] and len(toks) < len(full) and len(lp) == len(toks) - len(ids)
    check_against_oracle(ot2, toks, len(ids), lp)
    # a full KV cache (RuntimeWarning): max_pos = 512 -> the guard stops the request near 512 - 128
    long_ids = np.concatenate([ids, np.random.default_rng(9).integers(3, 900, 330 - len(ids))])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        toks, acc, lp = solo(sm, long_ids, max_new_tokens=400)
    assert any("would not fit a KV cache" in str(x.message) for x in w)
    assert sm.engine.state()["done"] & 4 and len(lp) == len(toks) - len(long_ids) > 0
    check_against_oracle(ot, toks, len(long_ids), lp)
    tail = sm.engine.logprobs(T["max_pos"] + 64)[len(toks) + 1:]
    assert not tail.any()  # nothing was written past the stop


# ---------------------------------------------------------------------------------------------------------------- 4. the default
def test_default_is_untouched_and_the_flag_is_part_of_the_graph_key(g8):
    sm, _, _ = build()
    t_ids = torch.from_numpy(g8["succ0_ids"])[None]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for gen in (dict(), dict(temperature=6.0, top_k=4, seed=1)):
            off = sm.specgenerate(t_ids, max_new_tokens=20, log=True, return_acceptance_len=True, **gen)
            s.synchronize()
            c0 = sm.engine.graph_stats()["captures"]
            assert len(off) == 4
            assert torch.is_tensor(sm.specgenerate(t_ids, max_new_tokens=20, **gen))  # a bare call still returns the ids alone
            s.synchronize()
            assert sm.engine.graph_stats()["captures"] == c0  # same key: replayed
            on = sm.specgenerate(t_ids, max_new_tokens=20, log=True, return_acceptance_len=True, return_logprobs=True, **gen)
            s.synchronize()
            c1 = sm.engine.graph_stats()["captures"]
            assert len(on) == 5 and c1 > c0  # another key: captured again, never the flag-off graph replayed
            np.testing.assert_array_equal(on[0].cpu().numpy(), off[0].cpu().numpy())
            assert on[1:4] == off[1:4]
            again = sm.specgenerate(t_ids, max_new_tokens=20, log=True, return_acceptance_len=True, **gen)
            s.synchronize()
            assert len(again) == 4 and sm.engine.graph_stats()["captures"] == c1  # ... and the flag-off graphs are still cached
            np.testing.assert_array_equal(again[0].cpu().numpy(), off[0].cpu().numpy())
    assert sm.engine.graph_stats()["replays"] > 0


# ---------------------------------------------------------------------------------------------------------------- 5. cohorts, streams, starts
@pytest.fixture(scope="module")
def cohort8(pair):
    sm = pair[0]
    return [sm] + [sm.make_cohort_member() for _ in range(7)]


BUDGETS = [24, 5, 17, 11, 20, 8, 14, 22]  # ragged: request 1 ends first and freezes while the others go on
# Sampled requests (each with its own seed): on this confident pair a greedy token has log-probability ~ 0, a token drawn at temperature
# 6 every now and then one near -15 (requests 0 and 5: their FIRST token) — a value at the wrong position cannot hide inside the bar
SAMPLED = dict(temperature=6.0, top_k=4)
SEEDS = [40, 41, 42, 43, 44, 45, 46, 47]


@pytest.fixture(scope="module")
def solo_runs(pair, g8):
    sm, ot, _ = pair
    runs = []
    for ids, b, sd in zip(prompts(g8, 8), BUDGETS, SEEDS):
        toks, acc, lp = solo(sm, ids, max_new_tokens=b, seed=sd, **SAMPLED)
        assert lp.min() < -5
        check_against_oracle(ot, toks, len(ids), lp)
        runs.append((toks, lp, oracle_logprobs(ot, toks, len(ids))[1]))
    return runs


def same_as_solo(got, want, ids, what):
    toks, lp = got[0][0].cpu().numpy(), got[4]
    w_toks, w_lp, scale = want
    np.testing.assert_array_equal(toks, w_toks, err_msg=what)
    assert lp.dtype == np.float32 and len(lp) == len(toks) - len(ids), what
    assert np.all(np.isfinite(lp)) and np.all(lp <= 0), what
    assert np.abs(lp.astype(np.float64) - w_lp).max() <= loop_bar(scale), what


@pytest.mark.parametrize("n_req", [2, 8])
def test_cohort_logprobs_equal_the_solo_runs_and_a_frozen_request_keeps_its_log(cohort8, solo_runs, g8, n_req):
    """Cohorts of 2 (gemm_wide) and 8 (gemm_c8)."""
    ps = prompts(g8, n_req)
    reqs = [(torch.from_numpy(p)[None], {}) for p in ps]
    got = specgenerate_cohort(cohort8[:n_req], reqs, max_new_tokens=BUDGETS[:n_req], seeds=SEEDS[:n_req], return_logprobs=True, **SAMPLED)
    for t in range(n_req):
        assert len(got[t]) == 5
        same_as_solo(got[t], solo_runs[t], ps[t], f"request {t}")
    # request 1 froze rounds before the cohort ended: its log holds its own values and nothing behind them
    n1 = got[1][0].shape[1]
    log1 = cohort8[1].engine.logprobs(T["max_pos"] + 64)
    np.testing.assert_array_equal(log1[len(ps[1]):n1], got[1][4])
    assert not log1[n1 + 1:].any() and not log1[:len(ps[1])].any()
    assert len(specgenerate_cohort(cohort8[:2], reqs[:2], max_new_tokens=4)[0]) == 4  # the default tuple


def test_cohort_of_four_with_a_64_node_tree(g8):
    sm, ot, _ = build(total_token=64)
    models = [sm] + [sm.make_cohort_member() for _ in range(3)]
    ps = prompts(g8, 4)
    got = specgenerate_cohort(models, [(torch.from_numpy(p)[None], {}) for p in ps], max_new_tokens=BUDGETS[:4], seeds=SEEDS[:4],
                              return_logprobs=True, **SAMPLED)
    for t in range(4):
        toks, _, lp = solo(sm, ps[t], max_new_tokens=BUDGETS[t], seed=SEEDS[t], **SAMPLED)
        check_against_oracle(ot, toks, len(ps[t]), lp)
        same_as_solo(got[t], (toks, lp, oracle_logprobs(ot, toks, len(ps[t]))[1]), ps[t], f"request {t}")


def test_stream_with_more_requests_than_slots_returns_each_requests_own_values(cohort8, solo_runs, g8):
    ps = prompts(g8, 8)
    order = [0, 2, 1, 5, 3, 6]  # long requests first: the slots are re-used by SHORTER requests, whose logs must not show the old tails
    reqs = [(torch.from_numpy(ps[i])[None], {}) for i in order]
    got = specgenerate_stream(cohort8[:2], reqs, max_new_tokens=[BUDGETS[i] for i in order], seeds=[SEEDS[i] for i in order],
                              return_logprobs=True, **SAMPLED)
    for k, i in enumerate(order):
        same_as_solo(got[k], solo_runs[i], ps[i], f"request {i}")
    for m in cohort8[:2]:  # what a slot's log holds in the end is its LAST request's alone
        st, log = m.engine.state(), m.engine.logprobs(T["max_pos"] + 64)
        assert not log[st["n_ctx"] + 1:].any() and not log[:m._prompt_len].any()


def test_first_value_on_every_prefill_flavour(cohort8, pair, g8):
    """batch_prefill=True, prefill_chunk_rows= and prefix= starts: requests 0 and 5 draw a first token whose target log-probability is
    near -15 — it must be present at index 0 and, like every other value, within the bar of the oracle's teacher-forced forward."""
    sm, ot, _ = pair
    pick = [0, 5]
    ps = [prompts(g8, 8)[i] for i in pick]
    reqs = [(torch.from_numpy(p)[None], {}) for p in ps]
    co = dict(max_new_tokens=[BUDGETS[i] for i in pick], seeds=[SEEDS[i] for i in pick], return_logprobs=True, **SAMPLED)
    runs = {"batch_prefill": specgenerate_cohort(cohort8[:2], reqs, batch_prefill=True, **co),
            "prefill_chunk_rows": specgenerate_cohort(cohort8[:2], reqs, prefill_chunk_rows=8, **co)}
    one = dict(log=True, return_acceptance_len=True, return_logprobs=True, **SAMPLED)
    pfx = sm.prefill_prefix(reqs[0][0][:, :10])
    a = sm.specgenerate(reqs[0][0], max_new_tokens=BUDGETS[0], seed=SEEDS[0], prefix=pfx, **one)
    b = sm.specgenerate(reqs[1][0], max_new_tokens=BUDGETS[5], seed=SEEDS[5], prefill_chunk_rows=8, **one)
    runs["prefix / chunked, single request"] = [a[:4] + (a[4][0].cpu().numpy(),), b[:4] + (b[4][0].cpu().numpy(),)]
    for name, got in runs.items():
        for t, r in enumerate(got):
            toks = r[0][0].cpu().numpy()
            want, scale = oracle_logprobs(ot, toks, len(ps[t]))
            assert want[0] < -5, (name, t, want[0])  # (the oracle's own value for the first token: far below the bar)
            assert len(r[4]) == len(toks) - len(ps[t]) and np.all(np.isfinite(r[4])) and np.all(r[4] <= 0), name
            assert np.abs(r[4].astype(np.float64) - want).max() <= loop_bar(scale), (name, t, r[4][:3], want[:3])


# ---------------------------------------------------------------------------------------------------------------- 6. determinism
def test_the_same_request_twice_gives_bit_identical_logprobs(pair, g8):
    sm = pair[0]
    for gen in (dict(), dict(temperature=6.0, top_k=4, seed=1)):
        a = solo(sm, g8["succ1_ids"], max_new_tokens=20, **gen)
        b = solo(sm, g8["succ1_ids"], max_new_tokens=20, **gen)
        np.testing.assert_array_equal(a[0], b[0])
        assert a[2].tobytes() == b[2].tobytes()


# ---------------------------------------------------------------------------------------------------------------- 7. AR cross-check
def test_ar_baseline_logprobs_against_the_speculative_ones(pair, g8):
    sm, ot, _ = pair
    ids = g8["succ0_ids"]
    toks, _, lp = solo(sm, ids, max_new_tokens=24)
    ar, ar_lp = sm.baseline_generate(torch.from_numpy(ids)[None], max_new_tokens=len(toks) - len(ids) - 1, return_logprobs=True)
    ar, ar_lp = ar[0].cpu().numpy(), ar_lp[0].cpu().numpy()
    assert ar_lp.dtype == np.float32 and len(ar_lp) == len(ar) - len(ids)
    n = min(len(ar), len(toks))
    assert n >= len(ids) + 24
    np.testing.assert_array_equal(ar[:n], toks[:n])
    scale = oracle_logprobs(ot, toks, len(ids))[1]
    k = n - len(ids)
    assert np.all(np.isfinite(ar_lp)) and np.all(ar_lp <= 0)
    # each side is within the bar of the oracle (the GEMMs run at different M): twice the bar between them
    assert np.abs(ar_lp[:k].astype(np.float64) - lp[:k]).max() <= 2 * loop_bar(scale)
    check_against_oracle(ot, ar, len(ids), ar_lp)
    assert torch.is_tensor(sm.baseline_generate(torch.from_numpy(ids)[None], max_new_tokens=4))  # the default return
