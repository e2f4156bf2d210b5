"""CPU (no GPU, no library): the host side of a shared prompt prefix — plan_prefill_pieces(past_lens=), PromptPrefix's matching and refusal
logic on CPU tensors, and the order of calls of a prefixed request start on recording stand-ins (copy with the right fan-out, then the
offset prefill at past_len = P, then the last stage on an [L, D] hidden)."""
from types import SimpleNamespace

import pytest

import helpers  # noqa: F401  (puts the repository root on sys.path)

LENS = [(300,), (1, 5, 33, 100), (129, 128, 127), (3, 7, 1, 20, 64, 2, 9, 31), (4,) * 9]


def pasts_of(lens):
    return [[0] * len(lens), [200] * len(lens), [(37 * (i + 1)) % 211 for i in range(len(lens))], [0 if i % 2 else 150 for i in range(len(lens))]]


# ----------------------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("lens", LENS)
def test_pieces_with_past_lens_cover_every_new_row_once_in_order(lens):
    from vispec_amd.prefill_plan import plan_prefill_pieces
    for past in pasts_of(lens):
        for C in (1, 37, 128, 129, sum(lens), sum(lens) + 5):
            pieces = plan_prefill_pieces(lens, C, 8, past_lens=past)
            placed = [0] * len(lens)
            stream = []
            for piece in pieces:
                assert 1 <= len(piece) <= 8, "at most 8 segments"
                end = 0
                for r, row0, pos0, ln in piece:
                    assert ln >= 1 and row0 == end, "segments are ascending and packed"
                    assert pos0 == past[r] + placed[r], "pos0 = P_r + the new rows already placed"
                    end = row0 + ln
                    placed[r] += ln
                    stream += [(r, pos0 - past[r] + k) for k in range(ln)]
                assert end <= C, "piece rows <= chunk_rows"
            assert placed == list(lens)
            assert stream == [(r, k) for r, ln in enumerate(lens) for k in range(ln)], "every new row exactly once, in order"
            # the cuts do not depend on the past lengths: only pos0 moves
            plain = plan_prefill_pieces(lens, C, 8)
            assert [[(r, row0, ln) for r, row0, _, ln in piece] for piece in pieces] == [[(r, row0, ln) for r, row0, _, ln in piece] for piece in plain]


@pytest.mark.parametrize("lens", LENS)
def test_without_past_lens_the_plan_is_unchanged(lens):
    from vispec_amd.prefill_plan import plan_prefill_pieces
    for C in (1, 37, 128, 1000):
        assert plan_prefill_pieces(lens, C, 8, past_lens=None) == plan_prefill_pieces(lens, C, 8) == plan_prefill_pieces(lens, C, 8, past_lens=[0] * len(lens))
    assert plan_prefill_pieces((5, 2, 6), 4) == [[(0, 0, 0, 4)], [(0, 0, 4, 1), (1, 1, 0, 2), (2, 3, 0, 1)], [(2, 0, 1, 4)], [(2, 0, 5, 1)]]
    assert plan_prefill_pieces((5, 2), 4, past_lens=(10, 0)) == [[(0, 0, 10, 4)], [(0, 0, 14, 1), (1, 1, 0, 2)]]
    for bad in ((1,), (1, 2, 3), (-1, 0)):
        with pytest.raises(ValueError):
            plan_prefill_pieces((5, 2), 4, past_lens=bad)


# ------------------------------------------------------------------------------------------------------------------------- PromptPrefix
torch = pytest.importorskip("torch")
IMG, VID, P, D = 999, 998, 6, 4


def make_prefix(weights, qwen=False):
    from vispec_amd.model.prefix import PromptPrefix
    ids = torch.tensor([[5, 6, IMG, IMG, 7, 8]])
    emb = torch.arange(P * D, dtype=torch.float32).reshape(P, D).to(torch.bfloat16)
    pos3 = torch.tensor([[0, 1, 2, 2, 3, 4], [0, 1, 2, 2, 3, 4], [0, 1, 2, 3, 4, 5]]) if qwen else None
    return PromptPrefix(torch.zeros(4, 2, P, 8, dtype=torch.bfloat16), emb + 100, emb, True, ids == IMG, ids, pos3=pos3,
                        grids=dict(image_grid_thw=[(1, 2, 4)]) if qwen else None, weights=weights)


def test_prompt_prefix_matching_and_refusals():
    w, other = object(), object()
    pfx = make_prefix(w)
    assert pfx.rows == P
    assert pfx.nbytes == 4 * 2 * P * 8 * 2 + 2 * P * D * 2 + P * 1 + P * 8
    ok = torch.tensor([[5, 6, IMG, IMG, 7, 8, 11, 12, 13]])
    assert pfx.check_request(ok, w, (IMG, VID)) == 9
    assert pfx.check_request(ok.to(torch.int32), w, (IMG, -1)) == 9
    with pytest.raises(ValueError, match="other target weights"):
        pfx.check_request(ok, other, (IMG,))
    with pytest.raises(ValueError, match="at least one new row"):
        pfx.check_request(ok[:, :P], w, (IMG,))
    with pytest.raises(ValueError, match="at least one new row"):
        pfx.check_request(ok[:, :3], w, (IMG,))
    bad = ok.clone()
    bad[0, 4] = 9
    with pytest.raises(ValueError, match="does not begin"):
        pfx.check_request(bad, w, (IMG,))
    for tid in (IMG, VID):
        vis = ok.clone()
        vis[0, -2] = tid
        with pytest.raises(ValueError, match="placeholder"):
            pfx.check_request(vis, w, (IMG, VID))
    with pytest.raises(ValueError):
        pfx.check_request(None, w, ())
    from vispec_amd.model.prefix import PromptPrefix
    with pytest.raises(ValueError):  # a store of other rows than the ids
        PromptPrefix(torch.zeros(4, 2, P + 1, 8), pfx.hidden, pfx.emb, True, None, pfx.ids)


def test_prompt_prefix_extend():
    w = object()
    pfx = make_prefix(w)
    ids = torch.tensor([[5, 6, IMG, IMG, 7, 8, 11, 12, 13]])
    new = torch.full((3, D), 7.0, dtype=torch.bfloat16)
    emb, mask, pos = pfx.extend(ids, new)
    assert pos is None and tuple(emb.shape) == (9, D) and emb.is_contiguous()
    assert torch.equal(emb[:P], pfx.emb) and torch.equal(emb[P:], new)
    assert mask.tolist() == [[False, False, True, True, False, False, False, False, False]]
    with pytest.raises(ValueError):
        pfx.extend(ids, new[:2])
    q = make_prefix(w, qwen=True)
    full = torch.cat([q.pos3, torch.tensor([[5, 6, 7]] * 3)], dim=1)
    emb, mask, pos = q.extend(ids, new, full)
    assert torch.equal(pos, full[:, P:])
    with pytest.raises(ValueError):
        q.extend(ids, new, None)
    moved = full.clone()
    moved[2, 3] += 1
    with pytest.raises(AssertionError):
        q.extend(ids, new, moved)


# ------------------------------------------------------------------------------------------------------- the start on recording stand-ins
class Rec:
    def __init__(self):
        self.calls = []


class FakeEngine:
    def __init__(self, rec, t, cap=64):
        self.rec, self.t, self.cap, self.device = rec, t, cap, torch.device("cpu")

    def check_prompt_fits(self, n):
        from vispec_amd.lib import VispecError
        self.rec.calls.append(("fits", self.t, n))
        if n > self.cap:
            raise VispecError("prompt does not fit")

    def load_kv_rows(self, store, engines):
        self.rec.calls.append(("copy", self.t, int(store.shape[2]), [e.t for e in engines]))


class FakeBase:
    def __init__(self, rec, t, w):
        self.rec, self.t, self.w = rec, t, w

    def prefill(self, x, position_ids=None, **kw):
        self.rec.calls.append(("prefill", self.t, int(x.shape[0]), dict(kw)))
        return torch.zeros(1, 10), torch.full((x.shape[0], D), float(self.t), dtype=torch.bfloat16)

    def prefill_batch(self, engines, xs, pos, **kw):
        for e, x, past in zip(engines, xs, kw.get("past_lens") or [0] * len(xs)):  # TargetLM.prefill_batch's own check, before any row
            e.check_prompt_fits(past + int(x.shape[0]))
        self.rec.calls.append(("prefill_batch", [e.t for e in engines], [int(x.shape[0]) for x in xs], dict(kw)))
        return [(torch.zeros(1, 10), torch.full((x.shape[0], D), float(e.t), dtype=torch.bfloat16)) for e, x in zip(engines, xs)]


class FakeModel:
    """The stages of SpecModel that _start_requests drives, recording; _start_prepare does the real prefix arithmetic."""

    def __init__(self, rec, t, w):
        self.rec, self.engine, self.base_model = rec, FakeEngine(rec, t), FakeBase(rec, t, w)

    def _visual_token_ids(self):
        return (IMG, VID)

    def _start_prepare(self, ids, inputs_embeds, kw, prefix=None, **gen):
        self.rec.calls.append(("prepare", self.engine.t, prefix is not None))
        Ln = ids.shape[1]
        if prefix is None:
            return SimpleNamespace(emb=torch.zeros(Ln, D, dtype=torch.bfloat16), position_ids=None, past=0, prefix=None)
        emb, mask, pos = prefix.extend(ids, torch.zeros(Ln - prefix.rows, D, dtype=torch.bfloat16))
        return SimpleNamespace(emb=emb, position_ids=pos, past=prefix.rows, prefix=prefix)

    def _start_finish(self, prep, logits, hidden):
        self.rec.calls.append(("finish", self.engine.t, tuple(hidden.shape)))
        return hidden

    def _start_request(self, ids, inputs_embeds, kw, **gen):  # the default path of the loops: no prefix keyword reaches it
        assert "prefix" not in gen
        self.rec.calls.append(("start_request", self.engine.t, dict(gen)))


GEN = dict(temperature=0.0, top_k=0.0, is_llama3=False)  # the generation keywords of a default call (_start_kw)


def request(n_new):
    return torch.tensor([[5, 6, IMG, IMG, 7, 8] + list(range(20, 20 + n_new))]), {}


def test_prefixed_start_call_sequence():
    from vispec_amd.model import spec_model_ours as smo
    rec, w = Rec(), object()
    pfx = make_prefix(w)
    models = [FakeModel(rec, t, w) for t in range(3)]
    forks = []
    out = smo._start_requests(models[:1], [request(5)], [0], [8], GEN, prefixes=[pfx], forks=forks)
    L_ = P + 5
    assert rec.calls == [("fits", 0, L_), ("prepare", 0, True), ("copy", 0, P, [0]), ("prefill", 0, 5, {"past_len": P}), ("finish", 0, (L_, D))]
    assert forks == [1]
    assert torch.equal(out[0][:P], pfx.hidden) and (out[0][P:] == 0).all()  # the [L, D] hidden = the prefix's rows, then the new rows
    # three requests, the middle one without a prefix: one copy with fan-out 2, per-request prefills, chunk_rows passed on
    rec.calls.clear()
    forks = []
    smo._start_requests(models, [request(1), request(9), request(33)], [0] * 3, [8] * 3, dict(GEN, prefill_chunk_rows=16),
                        prefixes=[pfx, None, pfx], forks=forks)
    kinds = [c[0] for c in rec.calls]
    assert kinds == ["fits"] * 3 + ["prepare"] * 3 + ["copy"] + ["prefill"] * 3 + ["finish"] * 3
    assert rec.calls[6] == ("copy", 0, P, [0, 2]) and forks == [2]
    assert rec.calls[7:10] == [("prefill", 0, 1, {"past_len": P, "chunk_rows": 16}), ("prefill", 1, P + 9, {"chunk_rows": 16}),
                               ("prefill", 2, 33, {"past_len": P, "chunk_rows": 16})]
    assert [c[2] for c in rec.calls[10:]] == [(P + 1, D), (P + 9, D), (P + 33, D)]
    # batch_prefill: one walk, every request one segment at its own past length
    rec.calls.clear()
    smo._start_requests(models, [request(1), request(9), request(33)], [0] * 3, [8] * 3, GEN, prefixes=[pfx, None, pfx], batch_prefill=True)
    walk = [c for c in rec.calls if c[0].startswith("prefill")]
    assert walk == [("prefill_batch", [0, 1, 2], [1, P + 9, 33], {"past_lens": [P, 0, P]})]
    assert [c[0] for c in rec.calls].index("copy") < [c[0] for c in rec.calls].index("prefill_batch")


def test_a_refusal_comes_before_any_copy_or_prefill():
    from vispec_amd.model import spec_model_ours as smo
    rec, w = Rec(), object()
    pfx, foreign = make_prefix(w), make_prefix(object())
    models = [FakeModel(rec, t, w) for t in range(2)]
    bad_ids = (torch.tensor([[5, 6, IMG, IMG, 7, 9, 20]]), {})
    visual = (torch.tensor([[5, 6, IMG, IMG, 7, 8, 20, IMG]]), {})
    exact = (torch.tensor([[5, 6, IMG, IMG, 7, 8]]), {})
    for reqs, pf, exc in (([request(3), bad_ids], pfx, ValueError), ([request(3), visual], pfx, ValueError), ([request(3), exact], pfx, ValueError),
                          ([request(3), request(4)], [pfx, foreign], ValueError), ([request(3), request(100)], pfx, RuntimeError)):
        rec.calls.clear()
        with pytest.raises(exc):
            smo._start_requests(models, reqs, [0, 0], [8, 8], GEN, prefixes=pf if isinstance(pf, list) else [pf, pf])
        assert all(c[0] == "fits" for c in rec.calls), rec.calls


def test_the_default_path_issues_no_copy():
    """specgenerate_cohort / specgenerate_stream without prefix= reach the models through _start_request with today's keywords only."""
    from vispec_amd.model import spec_model_ours as smo
    import inspect
    for fn in (smo.SpecModel.specgenerate, smo.specgenerate_cohort, smo.specgenerate_stream, smo.SpecModel._start_request, smo.SpecModel._start_prepare):
        assert inspect.signature(fn).parameters["prefix"].default is None
    assert inspect.signature(smo.SpecModel.prefill_prefix).parameters["prefill_chunk_rows"].default is None
    rec, w = Rec(), object()
    m = FakeModel(rec, 0, w)
    # SpecModel._start_request's own default route, on the stand-in: prepare, one whole-prompt prefill, finish
    smo.SpecModel._start_request(m, request(3)[0], None, {})
    assert [c[0] for c in rec.calls] == ["prepare", "prefill", "finish"] and rec.calls[1] == ("prefill", 0, P + 3, {})
    rec.calls.clear()
    smo.SpecModel._start_request(m, request(3)[0], None, {}, prefix=make_prefix(w))
    assert [c[0] for c in rec.calls] == ["fits", "prepare", "copy", "prefill", "finish"] and rec.calls[3] == ("prefill", 0, 3, {"past_len": P})


# ------------------------------------------------------------------------------------------------------------------- the route table
NEW, SEEDS, BUDGETS = (1, 9, 33), (3, 4, 5), (8, 9, 10)  # prompts of P + 1, P + 9 and P + 33 rows
ROUTES = {  # name: (requests, one letter per request — p: on the prefix, N: a whole prompt — or None for no prefix list at all, batch_prefill)
    "per-request": (3, None, False), "batched": (3, None, True), "batched with one request": (1, None, True),
    "prefixed, mixed": (3, "pNp", False), "prefixed, mixed, batched": (3, "pNp", True), "prefixed, all None, batched": (2, "NN", True),
}


def run_route(name, chunk=None, last=None):
    """-> (recorded calls, forks, batches, the exception or None) of _start_requests on route `name`; last = (new rows, prefix letter) puts
    another request in the last place (f: a prefix of other weights)."""
    from vispec_amd.model import spec_model_ours as smo
    n, letters, batch = ROUTES[name]
    rec, w = Rec(), object()
    new = list(NEW[:n])
    if last is not None:
        new[-1], letters = last[0], letters and letters[:-1] + last[1]
    entry = {"p": make_prefix(w), "N": None, "f": make_prefix(object())}  # requests with the same letter share ONE PromptPrefix
    forks, batches, raised = [], [], None
    try:
        smo._start_requests([FakeModel(rec, t, w) for t in range(n)], [request(k) for k in new], list(SEEDS[:n]), list(BUDGETS[:n]),
                            dict(GEN) if chunk is None else dict(GEN, prefill_chunk_rows=chunk),
                            prefixes=None if letters is None else [entry[c] for c in letters], batch_prefill=batch, forks=forks, batches=batches)
    except (ValueError, RuntimeError) as e:
        raised = e
    return rec.calls, forks, batches, raised


def staged(prepared, copies, walk, rows):
    return [("prepare", t, on) for t, on in enumerate(prepared)] + copies + walk + [("finish", t, (r, D)) for t, r in enumerate(rows)]


def expected_route(name, ck, pk):
    """(stage calls, forks, batches) per route: literals recorded from the three start routes and the ladders of the commit before they
    became one function; ck / pk = the chunk keyword as prefill[_batch] / _start_request receive it ({} by default)."""
    one = lambda t: ("start_request", t, dict(GEN, seed=SEEDS[t], max_new_tokens=BUDGETS[t], **pk))
    rows = [P + 1, P + 9, P + 33]
    return {
        "per-request": ([one(0), one(1), one(2)], [], []),
        "batched": (staged([False] * 3, [], [("prefill_batch", [0, 1, 2], rows, dict(ck))], rows), [], [3]),
        "batched with one request": ([one(0)], [], []),
        "prefixed, mixed": (staged([True, False, True], [("copy", 0, P, [0, 2])],
                                   [("prefill", 0, 1, dict(past_len=P, **ck)), ("prefill", 1, P + 9, dict(ck)), ("prefill", 2, 33, dict(past_len=P, **ck))],
                                   rows), [2], []),
        "prefixed, mixed, batched": (staged([True, False, True], [("copy", 0, P, [0, 2])],
                                            [("prefill_batch", [0, 1, 2], [1, P + 9, 33], dict(past_lens=[P, 0, P], **ck))], rows), [2], [3]),
        "prefixed, all None, batched": (staged([False] * 2, [], [("prefill_batch", [0, 1], rows[:2], dict(past_lens=[0, 0], **ck))], rows[:2]), [], [2]),
    }[name]


@pytest.mark.parametrize("chunk", [None, 16])
@pytest.mark.parametrize("name", list(ROUTES))
def test_route_table(name, chunk):
    """_start_requests is the one place that chooses the route of a start.  Stage calls = everything the stand-ins record but the
    check_prompt_fits calls (prefill_batch repeats that check itself, as the real one does): the next test is about those."""
    ck, pk = ({}, {}) if chunk is None else ({"chunk_rows": chunk}, {"prefill_chunk_rows": chunk})
    calls, forks, batches, raised = run_route(name, chunk)
    assert raised is None
    assert ([c for c in calls if c[0] != "fits"], forks, batches) == expected_route(name, ck, pk)


REFUSALS = [(name, last, exc) for name in ROUTES if ROUTES[name][0] > 1 and ROUTES[name] != (3, None, False)
            for last, exc in [((100, "N"), "VispecError")] + ([] if ROUTES[name][1] is None else
                                                              [((100, "p"), "VispecError"), ((0, "p"), "ValueError"), ((3, "f"), "ValueError")])]


@pytest.mark.parametrize("name,last,exc", REFUSALS)
def test_every_refusal_comes_before_any_stage_one_call(name, last, exc):
    """Every staged route; a prompt that does not fit, a prompt no longer than its prefix or a prefix of other weights as the LAST request,
    behind good ones: nothing but checks has run when it is refused.  On the batched route without prefixes this is the one difference
    from the commit before: there TargetLM.prefill_batch's own check refused the prompt, with the same VispecError, after stage one of
    every model."""
    calls, forks, batches, raised = run_route(name, last=last)
    assert type(raised).__name__ == exc
    assert calls and all(c[0] == "fits" for c in calls) and (forks, batches) == ([], [])
