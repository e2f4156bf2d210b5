"""Top-N alternatives per generated token (top_logprobs=N) on the tiny pair: the HIP selection kernel against float64 on the same bf16
rows (ids exact, values within logprob_helpers.kernel_bar), a scripted round, the bit-level ties to return_logprobs on real loops, the
oracle target's teacher-forced forward, cohorts / streams / mixed N, the ends and prefill flavours, the AR baseline and the default."""
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from helpers import T, vo  # noqa: E402
from logprob_helpers import bf16_round, kernel_bar, loop_bar, ref_token_logprob  # noqa: E402
from top_logprob_helpers import TOP_MAX, ref_top  # noqa: E402
from vispec_amd import synth  # noqa: E402
from vispec_amd.engine import DraftConfig, TargetConfig  # noqa: E402
from vispec_amd.model import SpecModel  # noqa: E402
from vispec_amd.model.spec_model_ours import specgenerate_cohort, specgenerate_stream  # noqa: E402

CAP = T["max_pos"] + 64  # the engine's token capacity: what the position-indexed logs hold
N_LOOP = 5


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


def solo(sm, ids, n_top=N_LOOP, **gen):
    """(tokens, logprobs, top ids, top values) of one request alone."""
    toks, _, _, _, lp, (ti, tv) = sm.specgenerate(torch.from_numpy(ids)[None], log=True, return_acceptance_len=True, return_logprobs=True,
                                                  top_logprobs=n_top, **gen)
    n_gen = toks.shape[1] - len(ids)
    assert ti.dtype == torch.int32 and tv.dtype == torch.float32 and ti.shape == tv.shape == (1, n_gen, n_top) and lp.shape == (1, n_gen)
    assert ti.device == tv.device == toks.device
    return toks[0].cpu().numpy(), lp[0].cpu().numpy(), ti[0].cpu().numpy(), tv[0].cpu().numpy()


def oracle_rows(ot, toks, n_prompt):
    """float64 [len(toks) - n_prompt, V]: the oracle target's teacher-forced logits row of every generated position — ONE forward over
    toks[:-1], as logprob_helpers.oracle_logprobs runs it."""
    toks = np.asarray(toks, np.int64)
    pkv, _, _ = vo.initialize_past_key_values(T["NL"], T["H"], T["max_pos"], T["D"] // T["H"])
    ot.tree_mask = None
    lg, _ = ot.forward(pkv, input_ids=toks[:-1])
    return np.asarray(lg, np.float64)[n_prompt - 1:]


def well_formed(ti, tv, V=T["V"]):
    """What holds for every entry whatever the logits: distinct ids inside the vocabulary, values non-increasing and <= 0."""
    assert np.all((ti >= 0) & (ti < V)) and np.all(np.isfinite(tv)) and np.all(tv <= 0)
    assert np.all(np.diff(tv, axis=-1) <= 0)
    for row in ti.reshape(-1, ti.shape[-1]):
        assert len(set(row.tolist())) == len(row)


def check_top_against_oracle(lg, ti, tv, what=""):
    """The two CONDITIONS of the device's entries against the oracle's rows lg [n_gen, V]: each device value within loop_bar(max|logits|)
    of the oracle's log-probability of the same token id; every oracle token whose logit clears the oracle's N-th value by more than
    twice the project's logits bar (2^-6 max|logits|: each side of a comparison may move by one bar) is in the device's list."""
    n_gen, N = ti.shape
    assert lg.shape[0] == n_gen, (what, lg.shape, ti.shape)
    well_formed(ti, tv)
    scale = float(np.abs(lg).max())
    bar = loop_bar(scale)
    worst = 0.0
    for i in range(n_gen):
        x = lg[i]
        m = x.max()
        lsm = x - m - np.log(np.exp(x - m).sum())
        worst = max(worst, float(np.abs(tv[i].astype(np.float64) - lsm[ti[i]]).max()))
        nth = np.sort(x)[-N]
        must = np.nonzero(x > nth + 2 * 2.0 ** -6 * scale)[0]
        missing = set(must.tolist()) - set(ti[i].tolist())
        assert not missing, (what, i, missing, ti[i])
    print(f"top values vs oracle {what}: max err {worst:.3e}, bar {bar:.3e}")
    assert worst <= bar, (what, worst, bar)


# ---------------------------------------------------------------------------------------------------------------- 1. the row kernel
def chunk_of(V):
    """csrc/tree_kernels.h, token_top_of_row: the contiguous elements one thread owns in the ordered compaction."""
    return ((V + 1023) // 1024 + 7) & ~7


def spread(V, count, rng):
    """`count` distinct ascending ids over the whole row: far-apart chunks and waves when V allows, 0 and V - 1 among them."""
    if count >= V:
        return np.arange(V)
    ids = np.unique(np.linspace(0, V - 1, count).round().astype(np.int64))
    while len(ids) < count:
        ids = np.unique(np.concatenate([ids, rng.integers(0, V, count - len(ids))]))
    return ids


def rows_for(V, N, rng):
    rows = {"normal4": bf16_round(rng.standard_normal(V).astype(np.float32) * 4.0),
            "near_flat": bf16_round(rng.standard_normal(V).astype(np.float32) * 0.05),
            "all_equal": np.full(V, 1.5, np.float32),
            "all_negative": bf16_round(-np.abs(rng.standard_normal(V).astype(np.float32)) * 4.0 - 1.0)}
    low = lambda: np.minimum(bf16_round(rng.standard_normal(V).astype(np.float32)), np.float32(2.5))  # noqa: E731  (a background below)
    for c in (1, 3, 200):  # the N-th value occurs c times, N - 1 larger values: the LOWEST of the c ids wins the last place
        if N - 1 + c > V:
            continue
        r = low()
        where = spread(V, N - 1 + c, rng)
        tie = where[rng.permutation(len(where))[:c]]
        big = np.setdiff1d(where, tie)
        r[tie] = 5.0
        r[big] = 10.0 + 0.5 * rng.permutation(N - 1)
        rows[f"nth_value_x{c}"] = r
    if N <= V:
        r = low()  # the N winners side by side inside (or, for chunks shorter than N, from the start of) one thread's chunk
        lo = (V // chunk_of(V) // 2) * chunk_of(V)
        lo = min(lo, V - N)
        r[lo:lo + N] = 6.0 + 0.25 * rng.permutation(N)
        rows["one_chunk"] = r
    if V >= 2:
        r = low()
        r[0], r[V - 1] = 20.0, 21.0
        rows["first_and_last_id"] = r
    # 1.0, 0.5, 0.25, then zeros of both signs straddling the N-th place (for N <= 3 the leading values shrink so that they still do)
    lead = [1.0, 0.5, 0.25][:max(0, min(3, N - 2))]
    vals = np.array(lead + [0.0, -0.0] * (N + 2), np.float32)[:V]
    r = bf16_round(np.minimum(low(), np.float32(0.0)) - np.float32(1.0))
    at = spread(V, len(vals), rng)
    r[at] = vals
    assert np.signbit(r[at]).any() or V < 3
    rows["signed_zeros"] = r
    return rows


def submit(eng, dev_row, pos, N):
    eng.token_top_logprob_row(dev_row, pos)
    ids, vals = eng.top_logprobs(pos + 1)
    return ids[pos, :N].copy(), vals[pos, :N].copy(), ids[pos, N:].copy(), vals[pos, N:].copy()


@pytest.mark.parametrize("N", [1, 5, 20])
@pytest.mark.parametrize("V", [7, 1000, 1024, 1025, 8195, 32064, 152064])
def test_row_kernel_ids_exactly_and_values_within_the_bar_against_float64(pair, V, N):
    """V < N (7 with 20), threads without a token (7 .. 8195: fewer than 1024 chunks of 8), a partial last chunk (all but 1024), a vector
    body plus a scalar tail (1000 % 8 = 0 is the pure vector case; 1025, 8195 have tails), the real vocabularies (152064: 152 per chunk)."""
    eng = pair[0].engine
    eng.set_logprobs(True)
    eng.set_top_logprobs(N)
    eng.begin_request(np.arange(3, 8), 4)
    rng = np.random.default_rng(1000 * N + V)
    pos = 10
    for name, row in rows_for(V, N, rng).items():
        want_ids, want_vals = ref_top(row, N)
        bar = kernel_bar(V, float(np.abs(row).max()))
        dev = torch.from_numpy(row).cuda().to(torch.bfloat16)
        assert np.array_equal(dev.float().cpu().numpy(), row)  # the test's rows are bf16 values already
        shifted = torch.zeros(V + 9, dtype=torch.bfloat16, device="cuda")
        shifted[1:V + 1].copy_(dev)
        views = {"aligned": dev, "odd_offset": shifted[1:V + 1]}
        assert dev.data_ptr() % 16 == 0 and views["odd_offset"].data_ptr() % 16 == 2 and views["odd_offset"].is_contiguous()
        for how, view in views.items():
            ids, vals, ids_rest, vals_rest = submit(eng, view, pos, N)
            pos += 1
            k = min(N, V)
            np.testing.assert_array_equal(ids, want_ids, err_msg=f"{name} {how} V={V} N={N}")
            err = np.abs(vals[:k].astype(np.float64) - want_vals[:k]).max()
            assert err <= bar, (name, how, V, N, err, bar)
            assert np.all(np.isneginf(vals[k:])) and np.all(ids[k:] == -1)
            assert not ids_rest.any() and not vals_rest.any()  # slots behind N stay as begin_request left them
            again = submit(eng, view, pos, N)  # the same row once more: identical bytes (across the two load paths the values may
            pos += 1                           # differ in the last place: the reduction sums in another order; the ids may not)
            assert (again[0].tobytes(), again[1].tobytes()) == (ids.tobytes(), vals.tobytes()), (name, how)
        if name == "all_equal":
            np.testing.assert_array_equal(ids[:min(N, V)], np.arange(min(N, V)))
        if name.startswith("nth_value"):
            assert ids[N - 1] == np.nonzero(row == 5.0)[0].min() and row[ids[N - 1]] == 5.0
        if name == "first_and_last_id":
            assert ids[0] == V - 1 and (N < 2 or ids[1] == 0)
    assert pos < CAP
    eng.set_logprobs(False)


# ---------------------------------------------------------------------------------------------------------------- 2. a scripted round
@pytest.mark.parametrize("forced", [0, "depth"])
def test_round_kernel_on_a_scripted_round_with_random_logits(pair, g8, forced):
    """One accept step with a scripted accept length (0 and depth) over RANDOM bf16 logits written into the verify buffer: position
    n + j + 1 gets ref_top of row sel[j] (and the log-probability of its token, as without top_logprobs); nothing else is touched."""
    sm = pair[0]
    eng = sm.engine
    ids = g8["succ0_ids"]
    sm.specgenerate(torch.from_numpy(ids)[None], max_new_tokens=1, return_logprobs=True, top_logprobs=N_LOOP)  # a live tree, the option on
    V, Tn = T["V"], eng.total_token
    fa = eng.depth if forced == "depth" else 0
    rng = np.random.default_rng(17 + fa)
    logits = bf16_round(rng.standard_normal((Tn, V)).astype(np.float32) * 3.0)
    eng.buffer("logits", (64, V))[:Tn].copy_(torch.from_numpy(logits).cuda().to(torch.bfloat16))
    eng.buffer("am", (64,), torch.int32)[:Tn].copy_(torch.from_numpy(np.argmax(logits, axis=1).astype(np.int32)).cuda())
    n = eng.state()["n_ctx"]
    before_lp, (before_i, before_v) = eng.logprobs(CAP), eng.top_logprobs(CAP)
    tree_tok = eng.tree()[0]
    eng.accept(fa)
    st = eng.state()
    a = st["accept_len"]
    assert a == fa and st["n_ctx"] == n + a + 1
    sel = eng.buffer("sel", (16,), torch.int32).cpu().numpy()
    after_lp, (after_i, after_v) = eng.logprobs(CAP), eng.top_logprobs(CAP)
    bar = kernel_bar(V, float(np.abs(logits).max()))
    for j in range(a + 1):
        want_ids, want_vals = ref_top(logits[sel[j]], N_LOOP)
        np.testing.assert_array_equal(after_i[n + j + 1, :N_LOOP], want_ids, err_msg=f"depth {j}")
        assert np.abs(after_v[n + j + 1, :N_LOOP].astype(np.float64) - want_vals).max() <= bar
        tok = int(tree_tok[sel[j + 1]]) if j < a else st["next_token"]
        assert abs(float(after_lp[n + j + 1]) - ref_token_logprob(logits[sel[j]], tok)) <= bar
    keep = np.ones(CAP, bool)
    keep[n + 1:n + a + 2] = False
    np.testing.assert_array_equal(after_i[keep], before_i[keep])
    np.testing.assert_array_equal(after_v[keep], before_v[keep])
    np.testing.assert_array_equal(after_lp[keep], before_lp[keep])
    assert not after_i[n + 1:n + a + 2, N_LOOP:].any() and not after_v[n + 1:n + a + 2, N_LOOP:].any()  # slots behind N: untouched
    eng.set_logprobs(False)


# ---------------------------------------------------------------------------------------------------------------- 3. bit-level invariants
GENS = [dict(temperature=0.0), dict(temperature=1.0, seed=0), dict(temperature=6.0, top_k=4, seed=1)]


@pytest.mark.parametrize("gen", GENS, ids=["greedy", "t1", "t6_topk4"])
def test_logprobs_are_byte_identical_with_and_without_and_listed_chosen_tokens_carry_them(pair, g8, gen):
    sm = pair[0]
    ids = g8["succ0_ids"]
    toks, lp, ti, tv = solo(sm, ids, max_new_tokens=24, **gen)
    plain = sm.specgenerate(torch.from_numpy(ids)[None], log=True, return_acceptance_len=True, return_logprobs=True, max_new_tokens=24, **gen)
    assert len(plain) == 5
    np.testing.assert_array_equal(plain[0][0].cpu().numpy(), toks)
    assert plain[4][0].cpu().numpy().tobytes() == lp.tobytes()
    well_formed(ti, tv)
    chosen = toks[len(ids):]
    listed = 0
    for i, tok in enumerate(chosen):
        hit = np.nonzero(ti[i] == tok)[0]
        if hit.size:
            listed += 1
            assert tv[i, hit[0]].tobytes() == lp[i].tobytes(), (i, tok)
        else:
            assert lp[i] <= tv[i, -1]  # a token outside the list is no likelier than the list's last
    assert listed > 0
    if gen["temperature"] == 0.0:
        assert tv[:, 0].tobytes() == lp.tobytes()  # the arg-max holds the row's largest logit
        unique_max = tv[:, 0] != tv[:, 1]
        assert unique_max.any()
        np.testing.assert_array_equal(ti[unique_max, 0], chosen[unique_max])
    again = solo(sm, ids, max_new_tokens=24, **gen)  # run to run: the same bytes
    assert again[2].tobytes() == ti.tobytes() and again[3].tobytes() == tv.tobytes()


# ---------------------------------------------------------------------------------------------------------------- 4. the oracle
@pytest.mark.parametrize("gen", GENS, ids=["greedy", "t1", "t6_topk4"])
def test_loop_entries_against_the_oracles_teacher_forced_forward(pair, g8, gen):
    sm, ot, od = pair
    ids = g8["succ0_ids"]
    toks, lp, ti, tv = solo(sm, ids, max_new_tokens=24, **gen)
    o_out = vo.specgenerate(ot, od, ids, max_new_tokens=24, max_pos=T["max_pos"], **gen)[0]
    np.testing.assert_array_equal(toks, o_out)
    check_top_against_oracle(oracle_rows(ot, toks, len(ids)), ti, tv, str(gen))


# ---------------------------------------------------------------------------------------------------------------- 5. cohorts, streams
@pytest.fixture(scope="module")
def cohort8(pair):
    sm = pair[0]
    return [sm] + [sm.make_cohort_member() for _ in range(7)]


BUDGETS = [24, 5, 17, 11, 20, 8, 14, 22]  # ragged: request 1 ends first and freezes while the others go on
SAMPLED = dict(temperature=6.0, top_k=4)
SEEDS = [40, 41, 42, 43, 44, 45, 46, 47]


@pytest.fixture(scope="module")
def solo_runs(pair, g8):
    """Per request alone, with N = 20 (an entry of N < 20 is its first N columns: the order is total): (toks, lp, ids, vals, oracle rows)."""
    sm, ot, _ = pair
    runs = []
    for ids, b, sd in zip(prompts(g8, 8), BUDGETS, SEEDS):
        toks, lp, ti, tv = solo(sm, ids, n_top=TOP_MAX, max_new_tokens=b, seed=sd, **SAMPLED)
        lg = oracle_rows(ot, toks, len(ids))
        check_top_against_oracle(lg, ti, tv, "solo")
        runs.append((toks, lp, ti, tv, lg))
    return runs


def same_as_solo(got, want, ids, N, what, exact):
    """The rule of the logprobs cohort tests (tests/test_logprobs_gpu.py: same_as_solo) for a tuple with the top-N entry: the solo run's
    tokens; log-probabilities within loop_bar of the solo run's; the entry well formed, of the ids' length, and — it is a function of logits
    that a cohort of five to eight computes in another summation order — under the oracle's two conditions; for cohorts of up to four
    (bit-identical logits) the solo run's entry byte for byte."""
    assert len(got) == 6, what
    toks, lp, (ti, tv) = got[0][0].cpu().numpy(), got[4], got[5]
    w_toks, w_lp, w_ti, w_tv, lg = want
    scale = float(np.abs(lg).max())
    np.testing.assert_array_equal(toks, w_toks, err_msg=what)
    assert lp.dtype == np.float32 and len(lp) == len(toks) - len(ids), what
    assert np.abs(lp.astype(np.float64) - w_lp).max() <= loop_bar(scale), what
    assert ti.dtype == np.int32 and tv.dtype == np.float32 and ti.shape == tv.shape == (len(toks) - len(ids), N), what
    if N:
        check_top_against_oracle(lg, ti, tv, what)
    if exact:
        assert lp.tobytes() == w_lp.tobytes(), what
        assert ti.tobytes() == np.ascontiguousarray(w_ti[:, :N]).tobytes() and tv.tobytes() == np.ascontiguousarray(w_tv[:, :N]).tobytes(), what


@pytest.mark.parametrize("n_req", [2, 8])
def test_cohort_entries_equal_the_solo_runs_and_a_frozen_request_keeps_its_entry(cohort8, solo_runs, g8, n_req):
    """Cohorts of 2 (gemm_wide: bit-identical to solo) and 8 (gemm_c8)."""
    ps = prompts(g8, n_req)
    reqs = [(torch.from_numpy(p)[None], {}) for p in ps]
    got = specgenerate_cohort(cohort8[:n_req], reqs, max_new_tokens=BUDGETS[:n_req], seeds=SEEDS[:n_req], return_logprobs=True,
                              top_logprobs=N_LOOP, **SAMPLED)
    for t in range(n_req):
        same_as_solo(got[t], solo_runs[t], ps[t], N_LOOP, f"request {t} of {n_req}", exact=n_req <= 4)
    # request 1 froze rounds before the cohort ended: its logs hold its own entries and nothing behind them
    n1 = got[1][0].shape[1]
    log_i, log_v = cohort8[1].engine.top_logprobs(CAP)
    np.testing.assert_array_equal(log_i[len(ps[1]):n1, :N_LOOP], got[1][5][0])
    np.testing.assert_array_equal(log_v[len(ps[1]):n1, :N_LOOP], got[1][5][1])
    assert not log_i[n1 + 1:].any() and not log_v[n1 + 1:].any() and not log_i[:len(ps[1])].any() and not log_v[:len(ps[1])].any()
    assert not log_i[:, N_LOOP:].any() and not log_v[:, N_LOOP:].any()
    assert len(specgenerate_cohort(cohort8[:2], reqs[:2], max_new_tokens=4)[0]) == 4  # the default tuples
    assert len(specgenerate_cohort(cohort8[:2], reqs[:2], max_new_tokens=4, return_logprobs=True)[0]) == 5


def test_mixed_n_across_the_members_of_one_cohort(cohort8, solo_runs, g8):
    """N = 5, 0, 20, 1 in one cohort: one launch serves them all, and n is part of the graph key per member — the same cohort with another
    assignment of N captures again instead of replaying the graphs that baked the first one in."""
    ps = prompts(g8, 4)
    reqs = [(torch.from_numpy(p)[None], {}) for p in ps]
    lead = cohort8[0].engine
    s = torch.cuda.Stream()  # (rounds are captured into graphs on a side stream only)
    for tops in ([5, 0, 20, 1], [1, 20, 0, 5]):
        with torch.cuda.stream(s):
            c0 = lead.graph_stats()["captures"]
            got = specgenerate_cohort(cohort8[:4], reqs, max_new_tokens=BUDGETS[:4], seeds=SEEDS[:4], return_logprobs=True, top_logprobs=tops,
                                      **SAMPLED)
            s.synchronize()
            assert lead.graph_stats()["captures"] > c0
        for t in range(4):
            same_as_solo(got[t], solo_runs[t], ps[t], tops[t], f"request {t}, N = {tops[t]}", exact=True)


def test_cohort_of_four_with_a_64_node_tree(g8):
    sm, ot, _ = build(total_token=64)
    models = [sm] + [sm.make_cohort_member() for _ in range(3)]
    ps = prompts(g8, 4)
    got = specgenerate_cohort(models, [(torch.from_numpy(p)[None], {}) for p in ps], max_new_tokens=BUDGETS[:4], seeds=SEEDS[:4],
                              return_logprobs=True, top_logprobs=N_LOOP, **SAMPLED)
    for t in range(4):
        toks, lp, ti, tv = solo(sm, ps[t], max_new_tokens=BUDGETS[t], seed=SEEDS[t], **SAMPLED)
        same_as_solo(got[t], (toks, lp, ti, tv, oracle_rows(ot, toks, len(ps[t]))), ps[t], N_LOOP, f"request {t}", exact=True)


def test_stream_with_more_requests_than_slots_returns_each_requests_own_entries(cohort8, solo_runs, g8):
    ps = prompts(g8, 8)
    order = [0, 2, 1, 5, 3, 6]  # long requests first: the slots are re-used by SHORTER requests, whose logs must not show the old tails
    reqs = [(torch.from_numpy(ps[i])[None], {}) for i in order]
    got = specgenerate_stream(cohort8[:2], reqs, max_new_tokens=[BUDGETS[i] for i in order], seeds=[SEEDS[i] for i in order],
                              return_logprobs=True, top_logprobs=N_LOOP, **SAMPLED)
    for k, i in enumerate(order):
        same_as_solo(got[k], solo_runs[i], ps[i], N_LOOP, f"request {i}", exact=True)
    for m in cohort8[:2]:  # what a slot's logs hold in the end is its LAST request's alone: a re-used slot started empty
        st, (log_i, log_v) = m.engine.state(), m.engine.top_logprobs(CAP)
        assert not log_i[st["n_ctx"] + 1:].any() and not log_v[st["n_ctx"] + 1:].any()
        assert not log_i[:m._prompt_len].any() and not log_v[:m._prompt_len].any()
    # fewer requests than slots (the plain-cohort route of the stream) and one request (the single-request route): the same tuples
    few = specgenerate_stream(cohort8[:4], reqs[:3], max_new_tokens=[BUDGETS[i] for i in order[:3]], seeds=[SEEDS[i] for i in order[:3]],
                              return_logprobs=True, top_logprobs=[N_LOOP, 0, 2], **SAMPLED)
    for k, (i, N) in enumerate(zip(order[:3], [N_LOOP, 0, 2])):
        same_as_solo(few[k], solo_runs[i], ps[i], N, f"request {i} of three", exact=True)
    one = specgenerate_stream(cohort8[:2], reqs[:1], max_new_tokens=BUDGETS[order[0]], seeds=[SEEDS[order[0]]], return_logprobs=True,
                              top_logprobs=N_LOOP, **SAMPLED)
    same_as_solo(one[0], solo_runs[order[0]], ps[order[0]], N_LOOP, "a stream of one", exact=True)


# ---------------------------------------------------------------------------------------------------------------- 6. ends, prefill flavours
def test_the_entry_ends_where_the_ids_end_at_eos_budget_and_a_full_kv_cache(pair, g8):
    sm, ot, od = pair
    ids = g8["succ0_ids"]
    # budget
    toks, lp, ti, tv = solo(sm, ids, max_new_tokens=9)
    assert len(toks) - len(ids) > 9 and len(ti) == len(lp) == len(toks) - len(ids)
    check_top_against_oracle(oracle_rows(ot, toks, len(ids)), ti, tv, "budget")
    # EOS: a token the stream is known to produce becomes the eos id (the engine config carries it)
    full = vo.specgenerate(ot, od, ids, max_new_tokens=40, max_pos=T["max_pos"])[0]
    eos = int(full[len(ids) + 9])
    sm2, ot2, od2 = build(eos=eos)
    toks, lp, ti, tv = solo(sm2, ids, max_new_tokens=40)
    assert eos in toks[len(ids):] and len(toks) < len(full) and len(ti) == len(toks) - len(ids)
    check_top_against_oracle(oracle_rows(ot2, toks, len(ids)), ti, tv, "eos")
    # a full KV cache (RuntimeWarning): the guard stops the request, frozen on the device, near max_pos - 128
    long_ids = np.concatenate([ids, np.random.default_rng(9).integers(3, 900, 330 - len(ids))])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        toks, lp, ti, tv = solo(sm, long_ids, max_new_tokens=400)
    assert any("would not fit a KV cache" in str(x.message) for x in w)
    assert sm.engine.state()["done"] & 4 and len(ti) == len(toks) - len(long_ids) > 0
    check_top_against_oracle(oracle_rows(ot, toks, len(long_ids)), ti, tv, "full cache")
    log_i, log_v = sm.engine.top_logprobs(CAP)
    assert not log_i[len(toks) + 1:].any() and not log_v[len(toks) + 1:].any()  # nothing was written past the stop


def test_first_entry_on_every_prefill_flavour(cohort8, pair, g8):
    """batch_prefill=True, prefill_chunk_rows= and prefix= starts (requests 0 and 5: a first token drawn far down the distribution): the
    first position's entry is there, and every entry meets the oracle's conditions."""
    sm, ot, _ = pair
    pick = [0, 5]
    ps = [prompts(g8, 8)[i] for i in pick]
    reqs = [(torch.from_numpy(p)[None], {}) for p in ps]
    co = dict(max_new_tokens=[BUDGETS[i] for i in pick], seeds=[SEEDS[i] for i in pick], return_logprobs=True, top_logprobs=N_LOOP, **SAMPLED)
    runs = {"batch_prefill": specgenerate_cohort(cohort8[:2], reqs, batch_prefill=True, **co),
            "prefill_chunk_rows": specgenerate_cohort(cohort8[:2], reqs, prefill_chunk_rows=8, **co),
            "whole": specgenerate_cohort(cohort8[:2], reqs, **co)}
    one = dict(log=True, return_acceptance_len=True, return_logprobs=True, top_logprobs=N_LOOP, **SAMPLED)
    pfx = sm.prefill_prefix(reqs[0][0][:, :10])
    a = sm.specgenerate(reqs[0][0], max_new_tokens=BUDGETS[0], seed=SEEDS[0], prefix=pfx, **one)
    b = sm.specgenerate(reqs[1][0], max_new_tokens=BUDGETS[5], seed=SEEDS[5], prefill_chunk_rows=8, **one)
    runs["prefix / chunked, single request"] = [x[:5] + (tuple(y[0].cpu().numpy() for y in x[5]),) for x in (a, b)]
    for name, got in runs.items():
        for t, r in enumerate(got):
            toks = r[0][0].cpu().numpy()
            ti, tv = r[5]
            assert ti.shape == tv.shape == (len(toks) - len(ps[t]), N_LOOP), name
            assert len(set(ti[0].tolist())) == N_LOOP, name  # position 0 was written (an empty entry is five zeros)
            check_top_against_oracle(oracle_rows(ot, toks, len(ps[t])), ti, tv, f"{name}, request {t}")


# ---------------------------------------------------------------------------------------------------------------- 7. the AR baseline
def test_ar_baseline_entries_against_the_speculative_ones(pair, g8):
    sm, ot, _ = pair
    ids = g8["succ0_ids"]
    toks, lp, ti, tv = solo(sm, ids, max_new_tokens=24)
    out = sm.baseline_generate(torch.from_numpy(ids)[None], max_new_tokens=len(toks) - len(ids) - 1, return_logprobs=True, top_logprobs=N_LOOP)
    assert len(out) == 3
    ar, ar_lp, (ar_ti, ar_tv) = out[0][0].cpu().numpy(), out[1][0].cpu().numpy(), [x[0].cpu().numpy() for x in out[2]]
    assert ar_ti.dtype == np.int32 and ar_tv.dtype == np.float32 and ar_ti.shape == ar_tv.shape == (len(ar) - len(ids), N_LOOP)
    n = min(len(ar), len(toks))
    assert n >= len(ids) + 24
    np.testing.assert_array_equal(ar[:n], toks[:n])
    lg = oracle_rows(ot, toks, len(ids))
    k = n - len(ids)
    # each side is within the bar of the oracle (the GEMMs run at different M): twice the bar between them, token by token
    bar2 = 2 * loop_bar(float(np.abs(lg).max()))
    for i in range(k):
        for slot, tok in enumerate(ar_ti[i]):
            hit = np.nonzero(ti[i] == tok)[0]
            if hit.size:
                assert abs(float(ar_tv[i, slot]) - float(tv[i, hit[0]])) <= bar2, (i, tok)
    assert ar_tv[:, 0].tobytes() == ar_lp.tobytes()  # greedy: the chosen token holds the row's largest logit
    check_top_against_oracle(oracle_rows(ot, ar, len(ids)), ar_ti, ar_tv, "AR")
    plain = sm.baseline_generate(torch.from_numpy(ids)[None], max_new_tokens=len(toks) - len(ids) - 1, return_logprobs=True)
    assert len(plain) == 2 and plain[1][0].cpu().numpy().tobytes() == ar_lp.tobytes()
    assert torch.is_tensor(sm.baseline_generate(torch.from_numpy(ids)[None], max_new_tokens=4))  # the default return


# ---------------------------------------------------------------------------------------------------------------- 8. the default
def test_default_is_untouched_and_n_is_part_of_the_graph_key(g8):
    sm, _, _ = build()
    t_ids = torch.from_numpy(g8["succ0_ids"])[None]
    kw = dict(max_new_tokens=20, log=True, return_acceptance_len=True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        off = sm.specgenerate(t_ids, **kw)
        on = sm.specgenerate(t_ids, return_logprobs=True, **kw)
        s.synchronize()
        c0 = sm.engine.graph_stats()["captures"]
        assert len(off) == 4 and len(on) == 5
        top = sm.specgenerate(t_ids, return_logprobs=True, top_logprobs=3, **kw)
        s.synchronize()
        c1 = sm.engine.graph_stats()["captures"]
        assert len(top) == 6 and c1 > c0  # another key: captured, never a graph without the kernel replayed
        top7 = sm.specgenerate(t_ids, return_logprobs=True, top_logprobs=7, **kw)
        s.synchronize()
        c2 = sm.engine.graph_stats()["captures"]
        assert c2 > c1 and top7[5][0].shape[-1] == 7
        np.testing.assert_array_equal(top7[5][0][..., :3].cpu().numpy(), top[5][0].cpu().numpy())
        off2 = sm.specgenerate(t_ids, **kw)
        on2 = sm.specgenerate(t_ids, return_logprobs=True, **kw)
        s.synchronize()
        assert sm.engine.graph_stats()["captures"] == c2  # the graphs of both earlier settings are still cached, and still theirs
        assert len(off2) == 4 and len(on2) == 5 and torch.is_tensor(sm.specgenerate(t_ids, max_new_tokens=20))
        for a, b in ((off, off2), (on, on2), (off, top), (on, top)):
            np.testing.assert_array_equal(a[0].cpu().numpy(), b[0].cpu().numpy())
            assert a[1:4] == b[1:4]
        assert on[4].cpu().numpy().tobytes() == on2[4].cpu().numpy().tobytes() == top[4].cpu().numpy().tobytes()
        caps = sm.engine.graph_stats()["captures"]
        for bad in (dict(top_logprobs=3), dict(top_logprobs=21, return_logprobs=True)):
            with pytest.raises(ValueError):
                sm.specgenerate(t_ids, max_new_tokens=4, **bad)
            with pytest.raises(ValueError):
                sm.baseline_generate(t_ids, max_new_tokens=4, **bad)
        assert sm.engine.graph_stats()["captures"] == caps
    with pytest.raises(Exception, match="top"):
        sm.engine.set_logprobs(False)
        sm.engine.set_top_logprobs(3)  # the library refuses n > 0 while log-probabilities are off
    with pytest.raises(Exception):
        sm.engine.set_logprobs(True)
        sm.engine.set_top_logprobs(21)
    sm.engine.set_logprobs(False)
