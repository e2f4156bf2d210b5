"""The float64 sampling reference of tests/sampling_helpers.py against the oracle on the reference's own G7 fixture, and the conditions the
GPU tests (tests/test_sampling_kernels_gpu.py) put on their inputs — checked here, so that a changed bar or input fails without a GPU."""
import os

import numpy as np
import pytest

from helpers import vo
from logprob_helpers import bf16_round
import sampling_helpers as sh


@pytest.fixture(scope="module")
def g7(golden_dir):
    return np.load(os.path.join(golden_dir, "g7_posterior_sampling.npz"))


def g7_cases(g):
    for i in range(int(g["n"])):
        yield i, bf16_round(g[f"logits{i}"]).reshape(g[f"logits{i}"].shape), g[f"cand{i}"], np.ascontiguousarray(g[f"u{i}"], np.float32), \
            float(g[f"T{i}"]), int(g[f"K{i}"])


def test_ref_posterior_and_ref_draw_equal_the_oracle_on_all_36_g7_cases(g7):
    n = 0
    for i, lg, cand, u, T, K in g7_cases(g7):
        ob, oa, op_ = vo.evaluate_posterior_sampling(lg, cand, T, lambda j, c: u[j, c], top_k=K)
        best, acc, removed, (rj, rc), comps = sh.ref_posterior(lg, cand, T, K, lambda j, c: u[j, c])
        assert (best, acc) == (ob, oa), i
        assert all(c[2] == u[c[0], c[1]] for c in comps)
        w = sh.ref_weights(lg[rj, rc], T, K, removed)
        np.testing.assert_array_equal(w > 0, op_ > 0, err_msg=f"case {i}: support of the final distribution")
        np.testing.assert_allclose(w / w.sum(), op_, rtol=1e-5, atol=1e-9)
        for uf in (0.0, 0.37 + 0.01 * (i % 7), 0.5, sh.U_LAST):
            assert sh.ref_draw(w, uf)[0] == vo.multinomial_inverse_cdf(op_, uf), (i, uf)
        n += 1
    assert n == 36


def test_ref_threshold_keeps_the_oracles_survivors(g7):
    for i, lg, cand, u, T, K in g7_cases(g7):
        for row in lg.reshape(-1, lg.shape[-1])[:4]:
            for k in sorted({K, 1, 3, 39, 40, 41}):
                keep = row >= sh.ref_threshold(row, k)
                np.testing.assert_array_equal(keep, vo.softmax_T(row, T, k) > 0, err_msg=f"case {i}, top_k {k}")
                np.testing.assert_array_equal(sh.ref_weights(row, T, k) > 0, keep)
    tied = np.float32([1.0, 3.0, 3.0, -2.0, 3.0, 0.0, -0.0, 5.0])
    assert sh.ref_threshold(tied, 2) == 3.0 and (tied >= sh.ref_threshold(tied, 2)).sum() == 4  # ties survive
    assert (tied >= sh.ref_threshold(tied, 6)).sum() == 7  # +0.0 and -0.0 are one value
    assert sh.ref_threshold(tied, 0) == -np.inf and sh.ref_threshold(tied, 8) == -np.inf and sh.ref_threshold(tied, 9) == -np.inf


def test_ref_draw_and_the_admissible_set():
    w = np.array([0.1, 0.0, 0.6, 0.3])
    assert [sh.ref_draw(w, u)[0] for u in (0.0, 0.0999, 0.1, 0.69, 0.7, 0.9999)] == [0, 0, 2, 2, 3, 3]
    assert abs(sh.ref_draw(w, 0.25)[1] - 0.15) < 1e-12 and abs(sh.ref_draw(w, 0.65)[1] - 0.05) < 1e-12
    cdf = sh.Cdf(w)
    assert cdf.admissible(0.4, 1e-3) == {2}
    assert cdf.admissible(0.1 + 1e-4, 1e-3) == {0, 2} and cdf.admissible(0.7 - 1e-4, 1e-3) == {2, 3}  # the side of the near step only
    assert cdf.admissible(1e-4, 1e-3) == {0} and cdf.admissible(1 - 1e-4, 1e-3) == {3}  # nothing lies beyond the ends
    tiny = sh.Cdf(np.array([0.5, 1e-6, 1e-6, 0.5]))  # neighbours below the bar: the walk passes them
    assert tiny.admissible(0.5 - 1e-5, 1e-3) == {0, 1, 2, 3} and tiny.admissible(0.5 - 1e-5, 1e-7) == {0}
    assert sh.draw_bar() == 2.0 ** -22


@pytest.mark.parametrize("V", sh.DRAW_V)
def test_first_token_configurations_stay_under_the_ambiguity_limit(V):
    """Condition of the GPU test (2a): at most 15 % of a configuration's 256 draws are ambiguous under draw_bar()."""
    u = sh.uniforms()
    worst = (-1.0, ("", 0.0, 0))
    for name, row, T, k in sh.draw_configs(V):
        assert np.array_equal(bf16_round(row), row)
        cdf = sh.Cdf(sh.ref_weights(row, T, k))
        tok, gap = cdf.draw(u)
        share = float((gap < sh.draw_bar()).mean())
        worst = max(worst, (share, (name, T, k)))
        assert share <= sh.MAX_AMBIGUOUS, (V, name, T, k, share)
        if name == "equal":  # the all-equal row: token floor(u * V)
            np.testing.assert_array_equal(tok[gap >= sh.draw_bar()], np.minimum(V - 1, np.floor(u * V))[gap >= sh.draw_bar()])
        if name == "wide" and k == 1:
            assert (tok == np.argmax(row)).all()
    print(f"V = {V}: worst ambiguous share {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("V", sh.EDGE_V)
def test_threshold_edge_rows_are_what_they_claim(V):
    u = sh.uniforms()
    chunk = -(-V // sh.THREADS)
    rows = {name: (row, k) for name, row, k in sh.edge_rows(V)}
    sup = lambda name: np.nonzero(sh.ref_weights(rows[name][0], 1.0, rows[name][1]) > 0)[0]
    assert len(set(sup("one_chunk") // chunk)) == 1 and len(sup("one_chunk")) == min(8, chunk)
    per_wave = sup("one_per_wave") // chunk // 64
    assert len(set(per_wave)) == len(per_wave) == (16 if V > 1025 else 8)  # (at V = 1025 only threads 0 .. 512 hold tokens)
    assert list(sup("ends")) == [0, V - 1]
    assert (sup("last_chunk") // chunk == (V - 1) // chunk).all() and sup("last_chunk")[-1] == V - 1
    for ties in (1, 3, 200):
        assert len(sup(f"tied_{ties}")) == 7 + ties
    assert rows["all_negative"][0].max() < 0 and len(sup("all_negative")) >= 8
    assert len(sup("signed_zeros")) == 9
    assert len(sup("top_k_is_V")) == V and len(sup("top_k_is_V_plus_1")) == V
    for name, (row, k) in rows.items():
        cdf = sh.Cdf(sh.ref_weights(row, 1.0, k))
        tok, gap = cdf.draw(u)
        assert (gap < sh.draw_bar()).mean() <= sh.MAX_AMBIGUOUS, name
        if len(cdf.support) <= 16 and (cdf.w[cdf.support] / cdf.total).min() >= 1 / 64:
            assert set(tok.tolist()) == set(cdf.support.tolist()), name  # the fixed seeds reach every supported token (see the GPU test)


@pytest.mark.parametrize("V", sh.ACCEPT_V)
def test_accept_cases_are_decided_and_cover_the_branches(V):
    """Conditions of the GPU test (2c): the redraw loop ends and changes fewer than 5 % of the uniforms, every comparison is decided,
    accept lengths 0 and >= 2 occur, at least 6 cases take the residual branch with two or more removed tokens."""
    accs, residual, redrawn, total = [], 0, 0, 0
    for c in range(sh.ACCEPT_CASES):
        cand, logits, T, top_k, u, u_final, nre = sh.accept_case(V, c)
        assert np.array_equal(bf16_round(logits).reshape(logits.shape), logits)
        assert (cand[:, 0] == cand[0, 0]).all() and (cand == -1).any()
        best, acc, removed, row, comps = sh.ref_posterior(logits, cand, T, top_k, lambda j, i: u[j, i])
        assert all(abs(uu - px) > sh.accept_bar(V, px, rm) for _, _, uu, px, rm in comps), c
        accs.append(acc)
        residual += len(removed) >= 2
        redrawn += nre
        total += u.size
        far = np.unique(cand[cand >= 0]) // (-(-V // sh.THREADS))
        assert len(np.unique(far)) >= 3  # candidate tokens in chunks far apart
    print(f"V = {V}: accept lengths {accs}, {residual} residual cases with >= 2 removed, {redrawn} of {total} uniforms redrawn")
    assert redrawn < 0.05 * total
    assert 0 in accs and max(accs) >= 2 and residual >= 6
    for u_final in (0.0, sh.U_LAST):
        cand, logits, T, top_k, u, uf = sh.scripted_case(V, u_final)
        best, acc, removed, (rj, rc), _ = sh.ref_posterior(logits, cand, T, top_k, lambda j, i: u[j, i])
        assert acc == 0 and len(removed) >= 2
        cdf = sh.Cdf(sh.ref_weights(logits[rj, rc], T, top_k, removed))
        want = cdf.support[0] if u_final == 0.0 else cdf.support[-1]
        assert cdf.draw(uf)[0][0] == want and cdf.admissible(uf, sh.draw_bar()) == {int(want)}
        assert len(cdf.support) <= 12 - 1  # top-12 survivors minus the removed ones among them


def test_accept_bar_shape():
    u = 2.0 ** -24
    assert sh.accept_bar(1008, 0.0, 0.3) == 0.0 and sh.accept_bar(1008, 0.5, 1.0) == float("inf")
    assert abs(sh.accept_bar(152064, 0.5, 0.0) - 0.5 * (149 + 29) * u) < 1e-18
    assert sh.accept_bar(32064, 0.5, 0.9) > sh.accept_bar(32064, 0.5, 0.1) > sh.accept_bar(32064, 0.5, 0.0)
