"""The temperature > 0 kernels of csrc/tree_kernels.h (vs_topk_threshold, vs_row_stats, vs_multinomial, verify_accept_sample_body) at the
vocabulary sizes of the shipped models, against the float64 reference of tests/sampling_helpers.py on the same bf16 logits.  At V <= 1024
every thread of the draw holds at most one token; here chunks of 2, 32 and 149 tokens, empty chunks, threads past the row's end and rows
with ties at the k-th value run under a test.  The bars (sampling_helpers.draw_bar, accept_bar) are derived there; the conditions these
tests put on their inputs are checked on the CPU by tests/test_sampling_ref_cpu.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch  # noqa: E402
from helpers import T, vo  # noqa: E402
import sampling_helpers as sh  # noqa: E402
from vispec_amd import lib as L, synth  # noqa: E402
from vispec_amd.engine import DraftConfig, TargetConfig  # noqa: E402
from vispec_amd.model import SpecModel  # noqa: E402

from test_fixtures_gpu import install  # noqa: E402
from test_kernels_gpu import p, stream  # noqa: E402


def build(V, D=256, NL=1):
    """tests/test_logprobs_gpu.build with vocab_size = V, D = 256 and one layer: the weights are irrelevant here, only the ctx's V and its
    verify-logits buffer matter."""
    tw = synth.make_target_weights(D, T["H"], T["I"], V, NL, seed=50, structured=True)
    dw = synth.make_draft_weights(D, T["H"], T["I"], V, num_q=2, seed=60, structured=True, target_embed=tw["model.embed_tokens.weight"], rho=0.25)
    tcfg = TargetConfig(hidden_size=D, num_heads=T["H"], num_kv_heads=T["H"], intermediate_size=T["I"], vocab_size=V, num_layers=NL,
                        max_position_embeddings=T["max_pos"], architectures=("LlamaForCausalLM",))
    dcfg = DraftConfig(hidden_size=D, num_heads=T["H"], intermediate_size=T["I"], vocab_size=V, max_position_embeddings=T["max_pos"])
    return SpecModel.from_weights(tcfg, dcfg, tw, dw, num_q=2)


@pytest.fixture(scope="module")
def models():
    """One model per vocabulary size, built on first use and kept for the module."""
    cache = {}

    def get(V):
        if V not in cache:
            cache[V] = build(V)
        return cache[V]

    return get


def device_row(row):
    dev = torch.from_numpy(row).cuda().to(torch.bfloat16)
    assert np.array_equal(dev.float().cpu().numpy(), row)  # the rows go in as exact bf16 values
    return dev


def draws(eng, dev_row, V, T_, top_k, out):
    """The first-token draw of seeds 0 .. 255 into ONE device array (vispec_sample_row writes through a pointer), one synchronisation."""
    out.fill_(-1)
    for s in sh.SEEDS:
        eng.set_sampling(T_, seed=s, top_k=top_k)
        L.check(eng.lib.vispec_sample_row(eng.h, stream(), p(dev_row), V, C.c_void_p(out.data_ptr() + 4 * s)))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def check_draws(got, cdf, u, what):
    """Every draw has positive reference weight; an unambiguous draw is the reference's; an ambiguous one is the reference's or the
    adjacent surviving token on the side of the near step (sampling_helpers.Cdf.admissible).  -> the number of ambiguous draws."""
    bar = sh.draw_bar()
    want, gap = cdf.draw(u)
    assert ((got >= 0) & (got < len(cdf.w))).all(), what
    assert (cdf.w[got] > 0).all(), (what, "a drawn token has no mass", got[cdf.w[got] <= 0][:8])
    clear = gap >= bar
    np.testing.assert_array_equal(got[clear], want[clear], err_msg=f"{what}: unambiguous draws")
    for s in np.nonzero(~clear)[0]:
        assert int(got[s]) in cdf.admissible(u[s], bar), (what, int(s), int(got[s]), int(want[s]), float(gap[s]))
    return int((~clear).sum())


# ---------------------------------------------------------------------------------------------------------------- a. the first-token draw
@pytest.mark.parametrize("V", sh.DRAW_V)
def test_first_token_draw_against_float64(models, V):
    """vispec_sample_row over V x T {0.7, 1, 6} x top_k {0, 1, 8, 50} x {N(0, 4^2), near-flat, all-equal} x seeds 0 .. 255: each draw against
    the inverse-CDF draw of the float64 weights with the same uniform, exact outside the ambiguity bar of draw_bar()."""
    eng = models(T["V"]).engine  # vispec_sample_row takes V as an argument: the tiny engine serves every V
    u = sh.uniforms()
    out = torch.empty(len(sh.SEEDS), dtype=torch.int32, device="cuda")
    rows, worst, total = {}, (-1, ("", 0.0, 0)), 0
    for name, row, T_, k in sh.draw_configs(V):
        if name not in rows:
            rows[name] = device_row(row)
        got = draws(eng, rows[name], V, T_, k, out)
        cdf = sh.Cdf(sh.ref_weights(row, T_, k))
        amb = check_draws(got, cdf, u, (V, name, T_, k))
        assert amb <= sh.MAX_AMBIGUOUS * len(u)
        worst, total = max(worst, (amb, (name, T_, k))), total + amb
        if name == "equal":  # floor(u * V), up to the ambiguity rule
            for s in range(len(u)):
                assert abs(int(got[s]) - min(V - 1, int(np.floor(u[s] * V)))) <= (cdf.draw(u[s])[1][0] < sh.draw_bar())
        if name == "wide" and k == 1:
            assert (got == np.argmax(row)).all()  # one strict maximum: that token for every seed
    eng.set_sampling(0.0)
    print(f"first-token draw, V = {V}: {total} ambiguous draws of {36 * len(u)}, worst configuration {worst[0]} of {len(u)} at {worst[1]}")


# ---------------------------------------------------------------------------------------------------------------- b. threshold edges
@pytest.mark.parametrize("V", sh.EDGE_V)
def test_topk_threshold_edges_through_the_draw(models, V):
    """Rows whose k survivors sit in one chunk, one per wave, at 0 and V - 1, in the last (partial) chunk; a k-th value tied 1, 3 and 200
    times; all-negative logits; +0.0 / -0.0 around the k-th value; top_k = V and V + 1 (threshold off).  Over 256 seeds no token outside
    the reference's support is drawn and every draw is the reference's (rule of a).  Where the support has <= 16 tokens of weight >= 1/64
    each, every supported token is drawn at least once: for weights >= 1/64 a token is missed by 256 independent uniforms with
    probability <= (63/64)^256 = 1.8 %, for the near-equal weights of these rows (>= 1/26 each) <= 16 * (25/26)^256 = 7e-4 — and the
    seeds are fixed: tests/test_sampling_ref_cpu.py asserts that the reference itself reaches every token with them."""
    eng = models(T["V"]).engine
    u = sh.uniforms()
    out = torch.empty(len(sh.SEEDS), dtype=torch.int32, device="cuda")
    covered = 0
    for name, row, k in sh.edge_rows(V):
        got = draws(eng, device_row(row), V, 1.0, k, out)
        cdf = sh.Cdf(sh.ref_weights(row, 1.0, k))
        assert set(got.tolist()) <= set(cdf.support.tolist()), (V, name, sorted(set(got.tolist()) - set(cdf.support.tolist()))[:8])
        check_draws(got, cdf, u, (V, name, k))
        if len(cdf.support) <= 16 and (cdf.w[cdf.support] / cdf.total).min() >= 1 / 64:
            assert set(got.tolist()) == set(cdf.support.tolist()), (V, name)
            covered += 1
        if name == "tied_200":
            assert len(set(got.tolist())) > 64  # the ties carry the mass: a threshold that kept 8 tokens could not draw this many
    assert covered >= 6
    eng.set_sampling(0.0)


# ---------------------------------------------------------------------------------------------------------------- c. accept + residual draw
def override(eng, u, u_final):
    u = np.ascontiguousarray(u, np.float32)
    L.check(eng.lib.vispec_set_uniform_override_host(eng.h, stream(), u.ctypes.data_as(C.c_void_p), u.shape[0], u.shape[1], C.c_float(u_final)))


def override_off(eng):
    L.check(eng.lib.vispec_set_uniform_override_host(eng.h, stream(), None, 0, 0, C.c_float(0)))
    eng.set_sampling(0.0, 0)


PROMPT = np.arange(3, 15, dtype=np.int32)


def accept_and_check(eng, cand, logits, T_, top_k, uni, u_final, what):
    """One vispec_accept on an installed tree against ref_posterior with the uniforms uni(j, i) / u_final: (best, accept_len), the accepted
    ids and n_ctx exact, the next token under the rule of (a) in the residual distribution.  -> (accept_len, removed count, ambiguous)."""
    eng.accept()
    best, acc = eng.last_accept()
    st = eng.state()
    rb, ra, removed, (rj, rc), _ = sh.ref_posterior(logits, cand, T_, top_k, uni)
    assert (best, acc) == (rb, ra), (what, (best, acc), (rb, ra))
    assert st["n_ctx"] == len(PROMPT) + acc + 1 and st["accept_len"] == acc, what
    np.testing.assert_array_equal(eng.tokens(st["n_ctx"])[len(PROMPT):], cand[best, : acc + 1], err_msg=f"{what}: accepted ids")
    nxt = st["next_token"]
    cdf = sh.Cdf(sh.ref_weights(logits[rj, rc], T_, top_k, removed))
    assert nxt not in removed, (what, nxt, removed)
    amb = check_draws(np.array([nxt]), cdf, np.array([u_final], np.float64), what)
    return acc, len(removed), amb, nxt, cdf


@pytest.mark.parametrize("V", sh.ACCEPT_V)
def test_accept_and_residual_draw_against_float64(models, V):
    """vispec_accept (verify_accept_sample_kernel) on 24 G7-like trees over N(0, 4^2) rows of the real vocabulary sizes, T {0.7, 1.3} x
    top_k {0, 12}, the uniforms through the override table with every comparison decided (further than accept_bar from its px)."""
    eng = models(V).engine
    accs, residual, amb = [], 0, 0
    try:
        for c in range(sh.ACCEPT_CASES):
            cand, logits, T_, top_k, u, u_final, _ = sh.accept_case(V, c)
            install(eng, cand, logits, PROMPT)
            eng.set_sampling(T_, seed=1, top_k=top_k)
            override(eng, u, u_final)
            a, nrem, am, _, _ = accept_and_check(eng, cand, logits, T_, top_k, lambda j, i: u[j, i], u_final, (V, c))
            accs.append(a)
            residual += nrem >= 2
            amb += am
        assert 0 in accs and max(accs) >= 2
        assert residual >= 6
        for u_final in (0.0, sh.U_LAST):  # the generator's extremes: the first and the last surviving, non-removed token
            cand, logits, T_, top_k, u, uf = sh.scripted_case(V, u_final)
            install(eng, cand, logits, PROMPT)
            eng.set_sampling(T_, seed=1, top_k=top_k)
            override(eng, u, uf)
            a, nrem, _, nxt, cdf = accept_and_check(eng, cand, logits, T_, top_k, lambda j, i: u[j, i], uf, (V, "scripted", u_final))
            assert a == 0 and nrem >= 2 and nxt == (cdf.support[0] if u_final == 0.0 else cdf.support[-1])
    finally:  # the engine is shared with the tests below: the override never outlives this one
        override_off(eng)
    print(f"accept, V = {V}: accept lengths {accs}, {residual} residual draws with >= 2 removed tokens, {amb} ambiguous final draws of {len(accs)}")


@pytest.mark.parametrize("V", sh.ACCEPT_V)
def test_accept_on_the_counter_generator(models, V):
    """No override: the uniforms are vs_uniform(seed, rounds, j, i) and (seed, rounds, 255, 255).  16 seeds on one tree; a comparison within
    accept_bar of its px leaves a seed undecided (nothing is asserted for it): at most 2 may be."""
    eng = models(V).engine
    cand, logits, T_, top_k, _, _, _ = sh.accept_case(V, 3)
    undecided = 0
    accs = []
    for seed in range(16):
        install(eng, cand, logits, PROMPT)
        eng.set_sampling(T_, seed=seed, top_k=top_k)
        rounds = eng.state()["rounds"]
        uni = lambda j, i: vo.uniform_hash(seed, rounds, j, i)
        comps = sh.ref_posterior(logits, cand, T_, top_k, uni)[4]
        if any(abs(uu - px) <= sh.accept_bar(V, px, rm) for _, _, uu, px, rm in comps):
            undecided += 1
            continue
        accs.append(accept_and_check(eng, cand, logits, T_, top_k, uni, vo.uniform_hash(seed, rounds, 255, 255), (V, "seed", seed))[0])
    eng.set_sampling(0.0, 0)
    print(f"accept on the counter generator, V = {V}: {undecided} of 16 seeds undecided, accept lengths {accs}")
    assert undecided <= 2
