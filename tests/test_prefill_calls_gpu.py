"""Which library entries a prefill calls, and in which order: TargetLM.prefill and TargetLM.prefill_batch share one layer walk and differ in
one step, rotary + KV append + attention — the single-sequence entries for prefill(), the varlen entries for prefill_batch (a batch of one
included).  The expected lists below were recorded from the code of the commit before the two walks were folded into one, driven against a
recording stand-in for the library (NOTEBOOK.md, "One prefill walk ..."); they are literals on purpose.
Also here: the host-side refusal of a cohort call on a closed context."""
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from helpers import T  # noqa: E402
from test_loop_gpu import build  # noqa: E402
from vispec_amd import lib as L  # noqa: E402

# the tiny model has two layers: layer 0 opens with the plain norm, every later norm also adds the previous GEMM's output to the residual stream
SINGLE = ["vispec_rmsnorm", "vispec_rope_append", "vispec_prefill_attention", "vispec_add_rmsnorm", "vispec_silu_mul",
          "vispec_add_rmsnorm", "vispec_rope_append", "vispec_prefill_attention", "vispec_add_rmsnorm", "vispec_silu_mul",
          "vispec_add_rmsnorm"]
VARLEN = ["vispec_rmsnorm", "vispec_rope_append_varlen", "vispec_prefill_attention_varlen", "vispec_add_rmsnorm", "vispec_silu_mul",
          "vispec_add_rmsnorm", "vispec_rope_append_varlen", "vispec_prefill_attention_varlen", "vispec_add_rmsnorm", "vispec_silu_mul",
          "vispec_add_rmsnorm"]
# W8A8: the q|k|v, gate|up and down inputs are quantised row by row (three launches per layer); o_proj and the lm_head stay W8A16, whose
# fp32 product is scaled and rounded by vispec_scale_bias_cast (one lm_head per request)
SINGLE_A8 = ["vispec_rmsnorm", "vispec_quant_rows_e4m3", "vispec_rope_append", "vispec_prefill_attention", "vispec_scale_bias_cast",
             "vispec_add_rmsnorm", "vispec_quant_rows_e4m3", "vispec_silu_mul", "vispec_quant_rows_e4m3",
             "vispec_add_rmsnorm", "vispec_quant_rows_e4m3", "vispec_rope_append", "vispec_prefill_attention", "vispec_scale_bias_cast",
             "vispec_add_rmsnorm", "vispec_quant_rows_e4m3", "vispec_silu_mul", "vispec_quant_rows_e4m3",
             "vispec_add_rmsnorm", "vispec_scale_bias_cast"]
VARLEN_A8 = ["vispec_rmsnorm", "vispec_quant_rows_e4m3", "vispec_rope_append_varlen", "vispec_prefill_attention_varlen", "vispec_scale_bias_cast",
             "vispec_add_rmsnorm", "vispec_quant_rows_e4m3", "vispec_silu_mul", "vispec_quant_rows_e4m3",
             "vispec_add_rmsnorm", "vispec_quant_rows_e4m3", "vispec_rope_append_varlen", "vispec_prefill_attention_varlen", "vispec_scale_bias_cast",
             "vispec_add_rmsnorm", "vispec_quant_rows_e4m3", "vispec_silu_mul", "vispec_quant_rows_e4m3",
             "vispec_add_rmsnorm"]
LM_HEAD_A8 = ["vispec_scale_bias_cast"]
EXPECTED = {"bf16": (SINGLE, VARLEN, []), "fp8a8": (SINGLE_A8, VARLEN_A8, LM_HEAD_A8)}


class Recorder:
    """Stands in for the loaded library: forwards every call and notes the name of each vispec_* entry."""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("vispec_"):
            return fn

        def call(*a):
            self.names.append(name)
            return fn(*a)
        return call


def recorded(monkeypatch, engines, f):
    rec = Recorder(L.load())
    with monkeypatch.context() as mp:
        for e in engines:
            mp.setattr(e, "lib", rec)
        mp.setattr(L, "_lib", rec)  # (scaled_linear reaches the library through L.load())
        f()
        torch.cuda.synchronize()
    return rec.names


@pytest.fixture(scope="module", params=["bf16", "fp8a8"])
def cohort(request):
    sm, _, _ = build(50, 60, True, arch="LlavaNextForConditionalGeneration", target_weight_dtype=request.param)
    models = [sm] + [sm.make_cohort_member() for _ in range(2)]
    yield models, request.param
    for m in models[::-1]:
        m.engine.close()


def embeds(Ln):
    g = torch.Generator().manual_seed(7 + Ln)
    return (torch.randn(Ln, T["D"], generator=g) * 0.05).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("Ln", [5, 129])  # 129: the smallest length that crosses the attention kernel's 128-row block
def test_prefill_issues_the_single_sequence_entries(monkeypatch, cohort, Ln):
    models, kind = cohort
    names = recorded(monkeypatch, [m.engine for m in models], lambda: models[0].base_model.prefill(embeds(Ln)))
    assert names == EXPECTED[kind][0]
    assert not any(n.endswith("_varlen") for n in names)


@pytest.mark.parametrize("lens", [(129,), (5, 129, 130)])
def test_prefill_batch_issues_the_varlen_entries(monkeypatch, cohort, lens):
    models, kind = cohort
    engines = [m.engine for m in models]
    names = recorded(monkeypatch, engines, lambda: models[0].base_model.prefill_batch(engines[:len(lens)], [embeds(ln) for ln in lens]))
    assert names == EXPECTED[kind][1] + EXPECTED[kind][2] * len(lens)
    assert "vispec_rope_append" not in names and "vispec_prefill_attention" not in names


START_ROUTES = {"per-request": {}, "batched": dict(batch_prefill=True), "prefixed": dict(prefix=True), "prefixed, batched": dict(prefix=True, batch_prefill=True),
                "per-request, chunked": dict(prefill_chunk_rows=64), "batched, chunked": dict(batch_prefill=True, prefill_chunk_rows=64)}
CONFIG = ["vispec_set_logprobs", "vispec_set_sampling"]  # stage one of a start
FINISH = ["vispec_argmax_rows", "vispec_begin_request", "vispec_draft_prefill"]  # stage three


def start_calls(kind):
    """The entries of each route's start for prompts of 5, 129 and 130 rows, as recorded by running the test below on the commit before
    the three start routes became one (spelled with the walks above; compared name by name with that recording).  The walk of a prefixed or
    chunked prefill is the varlen walk through the offset (`_at`) entries; 64-row chunks cut 129 and 130 rows into three pieces (5 rows
    stay whole) and the batch's 264 rows into five."""
    single, varlen, head = EXPECTED[kind]  # (the single-sequence walk of W8A8 ends with its lm_head's cast)
    offset = [n + "_at" if n.endswith("_varlen") else n for n in varlen]
    staged = lambda walks, copy=[]: CONFIG * 3 + copy + walks + FINISH * 3
    return {route: calls + ["vispec_get_state_host"] * 3 for route, calls in {
        "per-request": (CONFIG + single + FINISH) * 3,
        "batched": staged(varlen + head * 3),
        "prefixed": staged((offset + head) * 3, ["vispec_kv_copy_rows"]),
        "prefixed, batched": staged(offset + head * 3, ["vispec_kv_copy_rows"]),
        "per-request, chunked": CONFIG + single + FINISH + (CONFIG + offset * 3 + head + FINISH) * 2,
        "batched, chunked": staged(offset * 5 + head * 3),
    }.items()}


def test_a_whole_start_issues_the_recorded_entries(monkeypatch, cohort):
    """Every entry of the library between the call of specgenerate_cohort and its first round, on each route a request start can take:
    three prompts of 5, 129 and 130 rows with the same first four ids (the text-only prefix of the prefixed routes)."""
    from vispec_amd.model.spec_model_ours import specgenerate_cohort
    models, kind = cohort
    g = torch.Generator().manual_seed(11)
    head = torch.randint(3, T["V"] - 1, (4,), generator=g)
    reqs = [(torch.cat([head, torch.randint(3, T["V"] - 1, (Ln - 4,), generator=g)])[None], {}) for Ln in (5, 129, 130)]
    pfx = models[0].prefill_prefix(reqs[0][0][:, :4])
    got = {}
    for route, kw in START_ROUTES.items():
        kw = dict(kw, prefix=pfx) if "prefix" in kw else kw
        names = recorded(monkeypatch, [m.engine for m in models], lambda: specgenerate_cohort(models, reqs, max_new_tokens=1, **kw))
        got[route] = names[:names.index("vispec_cohortn_verify_accept")]
    assert got == start_calls(kind)


def test_cohort_calls_refuse_a_closed_context():
    """Host-side, before any library call: every cohort method names itself in the VispecError when a member's context was closed (the member
    closed here never ran a round)."""
    sm, _, _ = build(50, 60, True, arch="LlavaNextForConditionalGeneration")
    m1, m2 = sm.make_cohort_member(), sm.make_cohort_member()
    m2.engine.close()
    members, lead = [m1.engine, m2.engine], sm.engine
    calls = dict(cohort_round=lambda: lead.cohort_round(members), cohort_ar_step=lambda: lead.cohort_ar_step(members),
                 cohort_states=lambda: lead.cohort_states(members), cohort_states_enqueue=lambda: lead.cohort_states_enqueue(members, 0),
                 cohort_states_wait=lambda: lead.cohort_states_wait(members, 0))
    for name, call in calls.items():
        with pytest.raises(L.VispecError, match=f"^{name}: a context of this cohort was closed$"):
            call()
    m1.engine.close()
    sm.engine.close()
