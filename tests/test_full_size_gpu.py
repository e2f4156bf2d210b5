"""Full BASELINE sizes — every model of BASELINE.json's configs (bench.MODELS): LLaVA-v1.6-vicuna-7B (L = 2704 = 48 + 2144 image +
512 text tokens), LLaVA-v1.6-vicuna-13B (40 layers, 40 heads: the 8-GPU config's replica), Qwen2.5-VL-7B with a 4-image multi-turn
prompt (GQA 28/4, q/k/v bias, V = 152 064, multimodal rotary prefill, rope_delta) and Qwen2.5-VL-7B with fp8 target weights on a
1280x960 image.  The numpy oracle cannot run at these sizes in seconds, so parity here is size-independent properties: (1) the
reference's own invariant — speculative output == greedy AR output of the same target, token for token; (2) exact integer logic
replayed by the oracle on the device's buffers; (3) bookkeeping identities of the compressed draft KV and of the accept log."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from helpers import vo  # noqa: E402


# model -> (prompt length, image tokens, image runs)
SHAPES = {"llava7b": (2704, 2144, 1), "llava13b": (2704, 2144, 1), "qwen7b": (1584, 1024, 4), "qwen7b-fp8": (2124, 1564, 1),
          "qwen7b-fp8a8": (2124, 1564, 1)}  # (the last one: fp8 weights AND fp8 activations on the f8f6f4 MFMA — no BASELINE config, bench.py --model qwen7b-fp8a8)


@pytest.fixture(scope="module", params=list(SHAPES))
def model_full(request):
    import gc
    import bench
    bench.MODEL = request.param
    sms, tcfg, _ = bench.build_models(torch.device("cuda:0"), 0, 0, 1, 1)
    yield sms[0], tcfg, request.param
    bench.MODEL = "llava7b"
    del sms
    gc.collect()
    torch.cuda.empty_cache()


def test_speculative_equals_greedy_ar_at_full_size(model_full):
    import bench
    sm, tcfg, name = model_full
    bench.MODEL = name
    ids, pix = bench.make_request(tcfg, 3, torch.device("cuda:0"))
    out, new_token, idx, acc = sm.specgenerate(ids, max_new_tokens=96, log=True, return_acceptance_len=True, **pix)
    L = ids.shape[1]
    L_want, n_img, n_runs = SHAPES[name]
    assert L == L_want and int((ids == tcfg.image_token_index).sum()) == n_img
    assert new_token > 96 and len(acc) == idx + 1
    assert out.shape[1] == L + sum(a + 1 for a in acc) == L + new_token            # accept log <-> token count
    assert 0 <= min(acc) and max(acc) <= sm.engine.depth + 1
    st = sm.engine.state()
    assert st["n_ctx"] == out.shape[1]
    assert st["draft_len"] == st["n_ctx"] - n_img + n_runs * (sm.engine.num_q - 1)  # every image run compressed to num_q-1 draft rows
    # exact tree logic on the device's own candidate lists at full vocabulary
    k, d = sm.engine.top_k, sm.engine.depth
    n_all = k + d * k * k
    sc = sm.engine.buffer("scores_all", (n_all,), torch.float32).cpu().numpy()
    tk = sm.engine.buffer("tokens_all", (n_all,), torch.int32).cpu().numpy()
    pa = sm.engine.buffer("parents_all", (1 + d * k,), torch.int32).cpu().numpy()
    tok, pos, mask, ret = sm.engine.tree()
    w_tok, w_ret, w_mask, w_pos = vo.build_tree(sc, tk.astype(np.int64), pa.astype(np.int64), tok[0], sm.engine.total_token - 1, k)
    np.testing.assert_array_equal(tok, w_tok)
    np.testing.assert_array_equal(mask, w_mask)
    np.testing.assert_array_equal(ret, w_ret)
    # greedy invariance: same target, same kernels at T = 1
    ar = sm.baseline_generate(ids, max_new_tokens=96, max_steps=97, **pix)
    n = min(ar.shape[1], out.shape[1])
    assert n >= L + 96
    np.testing.assert_array_equal(ar[0, :n].cpu().numpy(), out[0, :n].cpu().numpy())
    assert np.mean(acc) > 1.5  # the structured synthetic pair really exercises multi-token acceptance


def test_idempotent_and_request_independent(model_full):
    """Running the same request twice (KV buffers reused, state reset on the device) gives identical tokens; an interleaved
    different request does not leak into it."""
    import bench
    sm, tcfg, name = model_full
    bench.MODEL = name
    dev = torch.device("cuda:0")
    a_ids, a_pix = bench.make_request(tcfg, 5, dev)
    b_ids, b_pix = bench.make_request(tcfg, 6, dev)
    a1 = sm.specgenerate(a_ids, max_new_tokens=48, **a_pix)
    b1 = sm.specgenerate(b_ids, max_new_tokens=48, **b_pix)
    a2 = sm.specgenerate(a_ids, max_new_tokens=48, **a_pix)
    assert torch.equal(a1, a2) and not torch.equal(a1[:, -40:], b1[:, -40:])


def test_cohort_of_two_equals_the_single_requests_at_full_size(model_full):
    """Two requests on one weight pass (64-row GEMMs, m_tile mode, fused two-request attention) at the real model sizes: token for token
    the single-request results."""
    import bench
    from vispec_amd.model.spec_model_ours import specgenerate_cohort
    sm, tcfg, name = model_full
    bench.MODEL = name
    dev = torch.device("cuda:0")
    reqs = [bench.make_request(tcfg, 7, dev), bench.make_request(tcfg, 8, dev)]
    want = [sm.specgenerate(ids, max_new_tokens=64, log=True, return_acceptance_len=True, **pix) for ids, pix in reqs]
    mb = sm.make_cohort_member()
    got = specgenerate_cohort([sm, mb], reqs, max_new_tokens=64)
    for (toks, new_token, idx, acc), w in zip(got, want):
        assert torch.equal(toks, w[0]) and (new_token, idx, acc) == (w[1], w[2], w[3])
    mb.engine.close()  # hands tile 1 back to the leader for the next test
    del mb


@pytest.mark.parametrize("n_req,row_blocks", [(4, 4), (3, 0), (4, 8), (3, 8), (4, 84)])
def test_wide_cohort_equals_the_single_requests_at_full_size(model_full, n_req, row_blocks):
    """Three / four requests on one weight pass (csrc/gemm_wide.h incl. its fp8 instantiations for the fp8 model, both launch shapes of
    vispec_set_wide_row_blocks, one launch per step for the per-request kernels, four-request attention) at the real sizes of EVERY
    BASELINE model: token for token the single-request results, with ragged budgets so that requests freeze one after the other."""
    import bench
    from vispec_amd.model.spec_model_ours import specgenerate_cohort
    sm, tcfg, name = model_full
    bench.MODEL = name
    dev = torch.device("cuda:0")
    reqs = [bench.make_request(tcfg, 20 + i, dev) for i in range(n_req)]
    budgets = [56, 40, 64, 33][:n_req]
    want = [sm.specgenerate(ids, max_new_tokens=b, log=True, return_acceptance_len=True, **pix) for (ids, pix), b in zip(reqs, budgets)]
    members = [sm.make_cohort_member() for _ in range(n_req - 1)]
    sm.engine.set_wide_row_blocks(row_blocks)
    try:
        got = specgenerate_cohort([sm] + members, reqs, max_new_tokens=budgets)
        for t, ((toks, new_token, idx, acc), w) in enumerate(zip(got, want)):
            assert torch.equal(toks, w[0]) and (new_token, idx, acc) == (w[1], w[2], w[3]), f"{name}: request {t}"
    finally:
        sm.engine.set_wide_row_blocks(4)
        for m in members:
            m.engine.close()
    del members


def test_ragged_cohort_at_full_size(model_full):
    """A cohort whose two requests have nothing in common: the bench request (thousands of context rows, image compression) next to a
    SHORT text-only prompt — attention key splits sized for the long one run mostly empty for the short one, the draft caches differ by
    an order of magnitude, and the short request gets a smaller token budget so that it finishes (and freezes on the device) long before
    its partner.  Each must still produce exactly what it produces alone."""
    import bench
    from vispec_amd.model.spec_model_ours import specgenerate_cohort
    sm, tcfg, name = model_full
    assert name in ("llava7b", "qwen7b")  # (conftest.py collects this property for one LLaVA and one Qwen configuration only)
    bench.MODEL = name
    dev = torch.device("cuda:0")
    long_req = bench.make_request(tcfg, 11, dev)
    rng = np.random.default_rng(12)
    short_ids = torch.from_numpy(rng.integers(3, min(tcfg.image_token_index, 30000), size=(1, 211))).to(dev)
    want_long = sm.specgenerate(long_req[0], max_new_tokens=80, log=True, return_acceptance_len=True, **long_req[1])
    want_short = sm.specgenerate(short_ids, max_new_tokens=24, log=True, return_acceptance_len=True)
    mb = sm.make_cohort_member()
    for order in (0, 1):  # the short request as member, then as leader
        reqs = [long_req, (short_ids, {})] if order == 0 else [(short_ids, {}), long_req]
        budgets = [80, 24] if order == 0 else [24, 80]
        got = specgenerate_cohort([sm, mb], reqs, max_new_tokens=budgets)
        wants = [want_long, want_short] if order == 0 else [want_short, want_long]
        for (toks, new_token, idx, acc), w in zip(got, wants):
            assert torch.equal(toks, w[0]) and (new_token, idx, acc) == (w[1], w[2], w[3])
    mb.engine.close()  # hands tile 1 back to the leader for the next test
    del mb


@pytest.mark.parametrize("CO", [8, 4, 2])
def test_default_bench_configuration_reproduces_single_request_tokens(CO):
    """The configuration bench.py's headline line runs — 4 concurrent lanes (host threads + streams, one weight copy) x cohorts of 8 (round 5:
    the cohort-8 GEMMs, whose summation order differs from the single-request kernel's in fp32 rounding — no greedy decision of these
    requests changes), of 4 and of 2 (rounds 3 / 2: bit-identical rows) at the LLaVA-7B sizes — against the same requests run ONE AT A TIME on one stream: every request's tokens,
    round count and accept lengths must be identical (concurrency and weight-pass sharing change throughput, never a token)."""
    import gc
    import bench
    from vispec_amd.model.spec_model_ours import specgenerate_cohort
    bench.MODEL = "llava7b"
    dev = torch.device("cuda:0")
    R, STEPS, NEW = 4, 2 if CO == 2 else 1, 72
    pairs, tcfg, _ = bench.build_models(dev, 0, 0, 1, R, CO)
    reqs = {i: bench.make_request(tcfg, 100 + i, dev) for i in range(CO * R * STEPS)}
    streams = [torch.cuda.Stream(dev) for _ in range(R)]
    torch.cuda.synchronize()

    def lane(l):
        def f():
            torch.cuda.set_device(dev)
            out = {}
            with torch.cuda.stream(streams[l]):
                for s_ in range(STEPS):
                    mine = [(s_ * R + l) * CO + j for j in range(CO)]
                    got = specgenerate_cohort(pairs[l], [reqs[i] for i in mine], max_new_tokens=NEW, seeds=mine)
                    out.update(zip(mine, got))
                streams[l].synchronize()
            return out
        return f

    res = {}
    for d in bench.run_lanes([lane(l) for l in range(R)]):
        res.update(d)
    sm = pairs[0][0]
    for i, (ids, pix) in reqs.items():
        w = sm.specgenerate(ids, max_new_tokens=NEW, log=True, return_acceptance_len=True, **pix)
        toks, new_token, idx, acc = res[i]
        assert torch.equal(toks, w[0]) and (new_token, idx, acc) == (w[1], w[2], w[3]), f"request {i}"
    assert sum(r[1] for r in res.values()) >= len(reqs) * NEW
    del pairs, sm
    gc.collect()
    torch.cuda.empty_cache()


def assert_close_with_tail(got, want, atol, frac=2e-5, mult=2.0):
    """|got - want| <= atol everywhere, except a statistical tail of <= `frac` of the elements up to mult x atol (the rule of
    test_kernels_gpu.assert_bf16_close: in a million-element tensor a handful of elements sit where two roundings flip together)."""
    err = np.abs(np.asarray(got, np.float32) - np.asarray(want, np.float32))
    bad = err > atol  # (atol: a scalar, or a bar per element broadcast against got, e.g. one per row)
    assert bad.mean() <= frac and not (err > mult * atol).any(), \
        f"{int(bad.sum())} / {bad.size} beyond {float(np.max(atol)):.4g}; worst {err.max():.4g} = {float(np.max(err / atol)):.3g} x its bar"


WIDTHS = {
    # kind: D, H, H_kv, I, V, image token, extra TargetConfig fields, extra synth / DraftConfig fields, fp8 target weights
    "llava7b": dict(D=4096, H=32, Hkv=32, I=11008, V=32064, IMG=32000, tkw={}, dkw={}, qkv_bias=False, fp8=False),
    "qwen7b": dict(D=3584, H=28, Hkv=4, I=18944, V=152064, IMG=151655, qkv_bias=True, fp8=False,
                   tkw=dict(rms_norm_eps=1e-6, rope_theta=1e6, qkv_bias=True, architectures=("Qwen2_5_VLForConditionalGeneration",), attn_impl="sdpa",
                            mrope_section=(16, 24, 24)),
                   dkw=dict(rms_norm_eps=1e-6, rope_theta=1e6, qkv_bias=True)),
}
WIDTHS["llava13b"] = dict(WIDTHS["llava7b"], D=5120, H=40, Hkv=40, I=13824)  # other split-K decompositions (K = 5120 / 13824), 40 heads
WIDTHS["qwen7b-fp8"] = dict(WIDTHS["qwen7b"], fp8=True)
WIDTHS["qwen7b-fp8a8"] = dict(WIDTHS["qwen7b"], fp8=True, a8=True)  # W8A8: both oracles quantise the decode activations too (Ops.linear a8=True)


@pytest.mark.parametrize("kind", list(WIDTHS))
def test_full_width_two_layer_model_against_the_oracle_floats(kind):
    """FLOAT parity at the real WIDTH of every BASELINE model family — LLaVA-7B (D = 4096, H = 32, I = 11008, V = 32064), Qwen2.5-VL-7B
    (D = 3584, GQA 28/4, q/k/v bias, theta 1e6, I = 18944, V = 152064, multimodal rotary prefill) and its fp8 (e4m3, W8A16) instantiation at the
    real K — on a 2-layer target + its draft, the sizes at which the numpy oracle still answers in seconds: (1) the PyTorch-ROCm prefill
    (hipBLASLt GEMMs, the library's causal attention and element-wise steps) against the oracle's eager prefill: final hidden rows, last-row
    logits and the K/V rows it wrote; (2) the draft prefill with image-token compression: last hidden row; (3) the verify forward of the first
    30-node tree (all skinny GEMMs at their real K, tree attention at real head_dim): hidden and logits; (4) integer logic exact.

    Bars (round 4): every tensor within 2^-6 of its largest magnitude of the bf16-emulating oracle (2^-5 until round 3), verify logits mean
    error <= 3e-3 of scale — and TRIANGULATED against the oracle in fp32 (the reference's arithmetic without any bf16 rounding): the kernels'
    error against fp32 truth may not exceed 1.25 x the error of the oracle's bf16 emulation (= the reference's own bf16 graph) against the
    same truth, in mean and in max — i.e. the HIP logits are no worse a bf16 evaluation of the model than the reference's are.
    BASELINE.json's "logits within 1e-3" is a quarter of one bf16 ulp of these logits (the logits ARE bf16 tensors in the reference): both
    implementations sit at the same distance from fp32 truth, which is what is asserted."""
    import gc
    from helpers import synth
    from vispec_amd.engine import DraftConfig, TargetConfig
    from vispec_amd.model import SpecModel
    from test_loop_gpu import check_tree_exact, fp8_codes_of
    Wd = WIDTHS[kind]
    D, H, Hk, I, V, IMG = Wd["D"], Wd["H"], Wd["Hkv"], Wd["I"], Wd["V"], Wd["IMG"]
    NL, MAXP = 2, 1024
    tw = synth.make_target_weights(D, H, I, V, NL, seed=300, qkv_bias=Wd["qkv_bias"], H_kv=Hk)
    dw = synth.make_draft_weights(D, H, I, V, seed=301, target_embed=tw["model.embed_tokens.weight"], qkv_bias=Wd["qkv_bias"])
    tcfg = TargetConfig(hidden_size=D, num_heads=H, num_kv_heads=Hk, intermediate_size=I, vocab_size=V, num_layers=NL, max_position_embeddings=MAXP,
                        image_token_index=IMG, **Wd["tkw"])
    dcfg = DraftConfig(hidden_size=D, num_heads=H, intermediate_size=I, vocab_size=V, max_position_embeddings=MAXP, **Wd["dkw"])
    sm = SpecModel.from_weights(tcfg, dcfg, tw, dw, target_weight_dtype=("fp8a8" if Wd.get("a8") else "fp8") if Wd["fp8"] else "bf16")
    okw = {k: v for k, v in Wd["tkw"].items() if k in ("rms_norm_eps", "rope_theta", "attn_impl", "mrope_section")}
    codes = fp8_codes_of(sm, D, H, Hk, I, NL) if Wd["fp8"] else False
    ocfg = vo.TargetConfig(D, H, Hk, I, V, NL, MAXP, **okw)
    ot = vo.TargetLlama(ocfg, tw, bf16=True, fp8=codes)
    ot32 = vo.TargetLlama(ocfg, tw, bf16=False, fp8=codes)  # fp32 truth (same weights — the same e4m3 codes and scales for the fp8 model)
    ot.a8_decode = ot32.a8_decode = bool(Wd.get("a8"))
    od = vo.DraftModel(vo.DraftConfig(D, H, I, V, MAXP, **{k: v for k, v in Wd["dkw"].items() if k != "qkv_bias"}), dw, bf16=True)
    eng = sm.engine
    rng = np.random.default_rng(302)
    n_pre, n_img, n_post = 24, 144, 40
    ids = np.concatenate([rng.integers(3, min(IMG, 150000), n_pre), np.full(n_img, IMG), rng.integers(3, min(IMG, 150000), n_post)])
    L = len(ids)
    feats = synth.bf16_grid(rng.standard_normal((n_img, D), dtype=np.float32) * 0.05)
    kw = dict(pixel_values=torch.from_numpy(feats).to(torch.bfloat16).cuda())
    pos3, delta = None, 0
    if "mrope_section" in Wd["tkw"]:
        grids = [(1, 24, 24)]  # 576 patches -> 144 merged tokens
        kw["image_grid_thw"] = torch.tensor(grids)
        pos3, delta = synth.qwen_rope_index(ids, IMG, grids)
    hidden, demb, mask_np, first = sm._start_request(torch.from_numpy(ids)[None], None, kw, max_new_tokens=64)
    # ---- (1) target prefill
    emb = ot.w["model.embed_tokens.weight"][ids].copy()
    emb[ids == IMG] = feats
    hd = D // H
    pkv, pkv_data, cur = vo.initialize_past_key_values(NL, Hk, MAXP, hd)
    pkv32, pkv32_data, cur32 = vo.initialize_past_key_values(NL, Hk, MAXP, hd)
    lg, hid = ot.forward(pkv, inputs_embeds=emb, position_ids=pos3)
    lg32, hid32 = ot32.forward(pkv32, inputs_embeds=emb, position_ids=pos3)
    tol = lambda want: 2.0 ** -6 * float(np.abs(want).max())
    a8 = bool(Wd.get("a8"))  # W8A8: element-wise bars cannot hold between two correct evaluations (see step 3): mean errors + the triangulation
    got_h = hidden.float().cpu().numpy()
    kvd = eng.target_kv.float().cpu().numpy()  # [2*NL, 1, H_kv, max_pos, hd]
    want_kv = pkv_data[0][:, 0, :, :L]
    if not a8:
        assert_close_with_tail(got_h, hid, tol(hid))  # (13B width: one of 1 064 960 prefill elements at 1.13 x the bar)
        assert_close_with_tail(kvd[:, 0, :, :L], want_kv, tol(want_kv))
    else:
        assert np.abs(got_h - hid).mean() <= 3e-2 * np.abs(hid).max() and np.abs(kvd[:, 0, :, :L] - want_kv).mean() <= 3e-2 * np.abs(want_kv).max()
        e_p, e_o = np.abs(got_h - hid32), np.abs(hid - hid32)  # the prefill's own triangulation against the fp32 evaluation
        assert e_p.mean() <= 1.25 * e_o.mean() and e_p.max() <= 1.5 * e_o.max(), "W8A8 prefill further from fp32 truth than the oracle's bf16 evaluation"
    first_tok = int(first.cpu()[0])
    top2 = np.sort(lg[-1])[-2:]
    if top2[1] - top2[0] > tol(lg[-1]):  # the first token is unambiguous at the test's tolerance
        assert first_tok == int(np.argmax(lg[-1]))
    # ---- (2) draft prefill on the DEVICE's hidden states (only the draft's arithmetic is compared)
    e_np = demb.float().cpu().numpy()
    e_shift = np.concatenate([e_np[1:], od.ops.rd(od.w["embed_tokens.weight"][[first_tok]])], 0)
    od.reset_kv()
    out_c, kv, _ = od.forward_prefill(got_h, e_shift, mask_np.astype(bool))
    dlast = eng.buffer("draft_last", (16, D))[:1].float().cpu().numpy()
    np.testing.assert_allclose(dlast, out_c[-1:], rtol=0, atol=tol(out_c[-1:]))
    assert eng.state()["draft_len"] >= L - n_img + (eng.num_q - 1)
    tok, pos, tmask, ret = check_tree_exact(eng)
    # ---- (3) verify forward of the first tree, each oracle on ITS OWN prefill KV (independent computations of the same model)
    eng.target_forward()
    Tn = len(tok)
    got_logits = eng.buffer("logits", (64, V))[:Tn].float().cpu().numpy()
    got_hidden = eng.buffer("hidden_new", (64, D))[:Tn].float().cpu().numpy()
    ot.tree_mask = ot32.tree_mask = tmask
    want_logits, want_hidden = ot.forward(pkv, input_ids=tok, position_ids=pos + L + delta)
    true_logits, true_hidden = ot32.forward(pkv32, input_ids=tok, position_ids=pos + L + delta)
    if not a8:
        np.testing.assert_allclose(got_hidden, want_hidden, rtol=0, atol=tol(want_hidden))
        np.testing.assert_allclose(got_logits, want_logits, rtol=0, atol=tol(want_logits))
    # (W8A8: re-quantising every GEMM input to 3 mantissa bits amplifies one-ulp differences of the inputs — the oracle against ITSELF with a quarter
    #  of the tree's embeddings moved by one bf16 ulp: mean 2e-2, max 1.3e-1 of scale at this width, 53 % of the hidden elements beyond 2^-6
    #  (NOTEBOOK.md, round 4) — so two correct bf16 evaluations of the W8A8 model differ element-wise by more than any ulp-sized bar; what is
    #  asserted is the triangulation below, the mean error, and the integer logic)
    scale = np.abs(true_logits).max()
    rel = np.abs(got_logits - want_logits) / scale
    e_hip, e_ora = np.abs(got_logits - true_logits) / scale, np.abs(want_logits - true_logits) / scale
    h_hip, h_ora = np.abs(got_hidden - true_hidden), np.abs(want_hidden - true_hidden)
    print(f"{kind} full-width verify logits: HIP vs bf16 oracle mean {rel.mean():.2e} max {rel.max():.2e} of scale | vs fp32 truth: HIP mean "
          f"{e_hip.mean():.2e} max {e_hip.max():.2e}, bf16 oracle mean {e_ora.mean():.2e} max {e_ora.max():.2e} | prefill hidden max err "
          f"{np.abs(got_h - hid).max() / np.abs(hid).max():.2e} of scale")
    assert rel.mean() <= (3e-2 if a8 else 3e-3)
    mx = 1.5 if a8 else 1.25  # (maxima of two chaotic error fields: a wider band for W8A8)
    assert e_hip.mean() <= 1.25 * e_ora.mean() and e_hip.max() <= mx * e_ora.max(), "HIP logits further from fp32 truth than the reference's bf16 graph"
    assert h_hip.mean() <= 1.25 * h_ora.mean() and h_hip.max() <= mx * h_ora.max(), "HIP hidden states further from fp32 truth than the reference's bf16 graph"
    # ---- (4) accept on the device's logits == the oracle's evaluate_posterior on the same numbers
    cand = np.concatenate([tok, [-1]])[ret]
    best, a, _ = vo.evaluate_posterior_greedy(got_logits[ret], cand)
    eng.accept()
    st = eng.state()
    assert (st["accept_len"], st["n_ctx"]) == (a, L + a + 1)
    del sm, ot, ot32, od, tw, dw
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", list(WIDTHS))
def test_full_width_cohort_of_eight_verify_logits_against_the_oracle(kind):
    """The cohort-8 GEMMs (csrc/gemm_c8.h: one accumulator chain per element instead of the single-request kernel's four folded K-quarters)
    at the real WIDTH of every model family: eight contexts prefill the same request, ONE cohort round verifies their (identical) first
    trees on one weight pass, and every context's verify logits / hidden states are held to the bars of the single-request test above —
    2^-6 of scale against the bf16-emulating oracle, mean <= 3e-3, and no further from the fp32 evaluation than 1.25 x the oracle's own
    bf16 evaluation (W8A8: the mean + triangulation bars of that test) — and the eight contexts agree bit for bit (a row does not depend on
    its tile)."""
    import gc
    from helpers import synth
    from vispec_amd.engine import DraftConfig, TargetConfig
    from vispec_amd.model import SpecModel
    from test_loop_gpu import check_tree_exact, fp8_codes_of
    Wd = WIDTHS[kind]
    D, H, Hk, I, V, IMG = Wd["D"], Wd["H"], Wd["Hkv"], Wd["I"], Wd["V"], Wd["IMG"]
    NL, MAXP = 2, 1024
    tw = synth.make_target_weights(D, H, I, V, NL, seed=300, qkv_bias=Wd["qkv_bias"], H_kv=Hk)
    dw = synth.make_draft_weights(D, H, I, V, seed=301, target_embed=tw["model.embed_tokens.weight"], qkv_bias=Wd["qkv_bias"])
    tcfg = TargetConfig(hidden_size=D, num_heads=H, num_kv_heads=Hk, intermediate_size=I, vocab_size=V, num_layers=NL, max_position_embeddings=MAXP,
                        image_token_index=IMG, **Wd["tkw"])
    dcfg = DraftConfig(hidden_size=D, num_heads=H, intermediate_size=I, vocab_size=V, max_position_embeddings=MAXP, **Wd["dkw"])
    sm = SpecModel.from_weights(tcfg, dcfg, tw, dw, target_weight_dtype=("fp8a8" if Wd.get("a8") else "fp8") if Wd["fp8"] else "bf16")
    models = [sm] + [sm.make_cohort_member() for _ in range(7)]
    okw = {k: v for k, v in Wd["tkw"].items() if k in ("rms_norm_eps", "rope_theta", "attn_impl", "mrope_section")}
    codes = fp8_codes_of(sm, D, H, Hk, I, NL) if Wd["fp8"] else False
    ocfg = vo.TargetConfig(D, H, Hk, I, V, NL, MAXP, **okw)
    ot = vo.TargetLlama(ocfg, tw, bf16=True, fp8=codes)
    ot32 = vo.TargetLlama(ocfg, tw, bf16=False, fp8=codes)
    ot.a8_decode = ot32.a8_decode = bool(Wd.get("a8"))
    rng = np.random.default_rng(302)
    n_pre, n_img, n_post = 24, 144, 40
    ids = np.concatenate([rng.integers(3, min(IMG, 150000), n_pre), np.full(n_img, IMG), rng.integers(3, min(IMG, 150000), n_post)])
    L = len(ids)
    feats = synth.bf16_grid(rng.standard_normal((n_img, D), dtype=np.float32) * 0.05)
    kw = dict(pixel_values=torch.from_numpy(feats).to(torch.bfloat16).cuda())
    pos3, delta = None, 0
    if "mrope_section" in Wd["tkw"]:
        grids = [(1, 24, 24)]
        kw["image_grid_thw"] = torch.tensor(grids)
        pos3, delta = synth.qwen_rope_index(ids, IMG, grids)
    for m in models:
        m._start_request(torch.from_numpy(ids)[None], None, dict(kw), max_new_tokens=64)
    emb = ot.w["model.embed_tokens.weight"][ids].copy()
    emb[ids == IMG] = feats
    hd = D // H
    pkv, _, _ = vo.initialize_past_key_values(NL, Hk, MAXP, hd)
    pkv32, _, _ = vo.initialize_past_key_values(NL, Hk, MAXP, hd)
    ot.forward(pkv, inputs_embeds=emb, position_ids=pos3)
    ot32.forward(pkv32, inputs_embeds=emb, position_ids=pos3)
    trees = [check_tree_exact(m.engine) for m in models]
    tok, pos, tmask, ret = trees[0]
    for t in trees[1:]:
        np.testing.assert_array_equal(t[0], tok)
        np.testing.assert_array_equal(t[2], tmask)
    sm.engine.cohort_round([m.engine for m in models[1:]])  # verify (all eight trees on one weight pass) + accept + the next draft round
    Tn = len(tok)
    ot.tree_mask = ot32.tree_mask = tmask
    want_logits, want_hidden = ot.forward(pkv, input_ids=tok, position_ids=pos + L + delta)
    true_logits, true_hidden = ot32.forward(pkv32, input_ids=tok, position_ids=pos + L + delta)
    tol = lambda want: 2.0 ** -6 * float(np.abs(want).max())
    a8 = bool(Wd.get("a8"))
    scale = np.abs(true_logits).max()
    first = None
    for t, m in enumerate(models):
        got_logits = m.engine.buffer("logits", (32, V))[:Tn].float().cpu().numpy()
        got_hidden = m.engine.buffer("hidden_new", (32, D))[:Tn].float().cpu().numpy()
        if first is None:
            first = (got_logits, got_hidden)
        else:
            np.testing.assert_array_equal(got_logits, first[0], err_msg=f"context {t}: a row must not depend on its tile")
            np.testing.assert_array_equal(got_hidden, first[1])
            continue
        if not a8:
            eh = np.abs(got_hidden - want_hidden)
            print(f"{kind} COHORT-8 hidden: worst {eh.max() / tol(want_hidden):.2f} x the 2^-6 bar, {int((eh > tol(want_hidden)).sum())} of {eh.size} beyond it")
            assert_close_with_tail(got_hidden, want_hidden, tol(want_hidden))  # (the tail rule of the GEMM tests: <= 2e-5 of the elements up to 2 x)
            assert_close_with_tail(got_logits, want_logits, tol(want_logits))
        rel = np.abs(got_logits - want_logits) / scale
        e_hip, e_ora = np.abs(got_logits - true_logits) / scale, np.abs(want_logits - true_logits) / scale
        h_hip, h_ora = np.abs(got_hidden - true_hidden), np.abs(want_hidden - true_hidden)
        print(f"{kind} full-width COHORT-8 verify logits: HIP vs bf16 oracle mean {rel.mean():.2e} max {rel.max():.2e} of scale | vs fp32 truth: HIP mean "
              f"{e_hip.mean():.2e} max {e_hip.max():.2e}, bf16 oracle mean {e_ora.mean():.2e} max {e_ora.max():.2e}")
        assert rel.mean() <= (3e-2 if a8 else 3e-3)
        mx = 1.5 if a8 else 1.25
        assert e_hip.mean() <= 1.25 * e_ora.mean() and e_hip.max() <= mx * e_ora.max(), "cohort-8 logits further from fp32 truth than the reference's bf16 graph"
        assert h_hip.mean() <= 1.25 * h_ora.mean() and h_hip.max() <= mx * h_ora.max(), "cohort-8 hidden states further from fp32 truth than the reference's bf16 graph"
        # the accept the device took on these logits == the oracle's evaluate_posterior on the same numbers
        cand = np.concatenate([tok, [-1]])[ret]
        best, a, _ = vo.evaluate_posterior_greedy(got_logits[ret], cand)
        st = m.engine.state()
        assert (st["accept_len"], st["n_ctx"]) == (a, L + a + 1)
    del models, sm, ot, ot32, tw, dw
    gc.collect()
    torch.cuda.empty_cache()


def test_cohort_of_eight_at_full_size(model_full):
    """Eight requests on one weight pass at the real sizes of EVERY BASELINE model (csrc/gemm_c8.h, eight-request attention launches, the
    two-tile slab of the draft GEMMs), ragged budgets: (1) a request's tokens do not depend on the cohort's composition (the same requests in
    reverse order through other tiles); (2) speculative == greedy AR at the same batching, token for token; (3) the c8 summation order changes
    no greedy decision of these requests: token for token the single-request results."""
    import bench
    from vispec_amd.model.spec_model_ours import baseline_generate_cohort, specgenerate_cohort
    sm, tcfg, name = model_full
    bench.MODEL = name
    dev = torch.device("cuda:0")
    reqs = [bench.make_request(tcfg, 40 + i, dev) for i in range(8)]
    budgets = [56, 40, 64, 33, 48, 61, 37, 52]
    members = [sm.make_cohort_member() for _ in range(7)]
    models = [sm] + members
    try:
        got = specgenerate_cohort(models, reqs, max_new_tokens=budgets)
        rev = specgenerate_cohort(models, reqs[::-1], max_new_tokens=budgets[::-1])[::-1]
        for t, (a, b) in enumerate(zip(got, rev)):
            assert torch.equal(a[0], b[0]) and a[1:] == b[1:], f"{name}: request {t} depends on its cohort"
        ar = baseline_generate_cohort(models, reqs, max_new_tokens=budgets)
        for t, ((toks, new_token, idx, acc), a) in enumerate(zip(got, ar)):
            n = min(toks.shape[1], a.shape[1])
            assert n >= reqs[t][0].shape[1] + budgets[t]
            assert torch.equal(toks[0, :n], a[0, :n]), f"{name}: request {t}: speculative != AR"
        same = 0
        for t, ((ids, pix), b) in enumerate(zip(reqs, budgets)):
            w = sm.specgenerate(ids, max_new_tokens=b, log=True, return_acceptance_len=True, **pix)
            same += int(torch.equal(got[t][0], w[0]) and got[t][1:] == (w[1], w[2], w[3]))
        print(f"{name}: {same} of 8 cohort-8 requests token-for-token equal to their single-request runs")
        assert same == 8
    finally:
        for m in members:
            m.engine.close()
    del members


def test_wide_tree_cohort_at_full_size(model_full):
    """Trees of 60 nodes (what the reference's total_token = -1 autotune may pick, spec_model_ours.py:179-201) in a cohort of FOUR at full size
    (round 6): two activation tiles per request, eight tiles on the cohort-8 kernel, the q|k|v epilogue with per-tile row counts, 2 q-tiles per
    head in the attention.  == the single-request runs token for token, composition-independent, speculative == AR; then back to 30 nodes."""
    import bench
    from vispec_amd.model.spec_model_ours import baseline_generate_cohort, specgenerate_cohort
    sm, tcfg, name = model_full
    assert name in ("llava7b", "qwen7b")  # (conftest.py collects this property for one LLaVA and one Qwen configuration only)
    bench.MODEL = name
    dev = torch.device("cuda:0")
    reqs = [bench.make_request(tcfg, 80 + i, dev) for i in range(4)]
    budgets = [44, 31, 52, 38]
    members = [sm.make_cohort_member() for _ in range(3)]
    models = [sm] + members
    try:
        sm.spec_layer.total_tokens = 59
        want = [sm.specgenerate(ids, max_new_tokens=b, log=True, return_acceptance_len=True, **pix) for (ids, pix), b in zip(reqs, budgets)]
        got = specgenerate_cohort(models, reqs, max_new_tokens=budgets)
        assert all(m.engine.total_token == 60 for m in models)
        rev = specgenerate_cohort(models, reqs[::-1], max_new_tokens=budgets[::-1])[::-1]
        for t, (a, b) in enumerate(zip(got, rev)):
            assert torch.equal(a[0], b[0]) and a[1:] == b[1:], f"{name}: request {t} depends on its cohort"
        same = sum(int(torch.equal(g[0], w[0]) and g[1:] == (w[1], w[2], w[3])) for g, w in zip(got, want))
        print(f"{name}: {same} of 4 wide-tree cohort requests token-for-token equal to their single-request runs; accept lengths {[round(float(np.mean(g[3])), 2) for g in got]}")
        assert same == 4
        ar = baseline_generate_cohort(models, reqs, max_new_tokens=budgets)
        for t, ((toks, new_token, idx, acc), a) in enumerate(zip(got, ar)):
            n = min(toks.shape[1], a.shape[1])
            assert n >= reqs[t][0].shape[1] + budgets[t] and torch.equal(toks[0, :n], a[0, :n]), f"{name}: request {t}: speculative != AR"
    finally:
        sm.spec_layer.total_tokens = 29
        for m in members:
            m.engine.close()
    out = sm.specgenerate(reqs[0][0], max_new_tokens=24, **reqs[0][1])
    assert out.shape[1] >= reqs[0][0].shape[1] + 24

