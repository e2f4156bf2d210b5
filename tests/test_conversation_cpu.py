"""CPU (no GPU, no library): the host side of a conversation prefix — PromptPrefix.truncated on hand-made tensors, and conversation_prefix,
the helper that assembles a finished request into the next turn's PromptPrefix, on fake hidden rows, embeddings and ids (the K/V copy, the
hidden-row log and the embedding table are recording stand-ins)."""
import warnings
from types import SimpleNamespace

import pytest

import helpers  # noqa: F401  (puts the repository root on sys.path)

torch = pytest.importorskip("torch")
IMG, VID, L, D = 999, 998, 6, 4


def make_prefix(weights, qwen=False, rows=9):
    from vispec_amd.model.prefix import PromptPrefix
    ids = torch.tensor([[5, 6, IMG, IMG, 7, 8, 11, 12, 13]])[:, :rows]
    emb = torch.arange(rows * D, dtype=torch.float32).reshape(rows, D).to(torch.bfloat16)
    pos3 = torch.tensor([[0, 1, 2, 2, 3, 4, 5, 6, 7], [0, 1, 2, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6, 7, 8]])[:, :rows] if qwen else None
    store = torch.arange(4 * 2 * rows * 8, dtype=torch.float32).reshape(4, 2, rows, 8).to(torch.bfloat16)
    return PromptPrefix(store, emb + 100, emb, True, ids == IMG, ids, pos3=pos3, grids=dict(image_grid_thw=[(1, 2, 4)]) if qwen else None,
                        weights=weights)


def storage(t):
    return t.untyped_storage().data_ptr()


@pytest.mark.parametrize("qwen", [False, True])
def test_truncated_slices_every_field_into_memory_of_its_own(qwen):
    w = object()
    pfx = make_prefix(w, qwen)
    for rows in (4, 5, 8, 9):
        cut = pfx.truncated(rows)
        assert cut.rows == rows and cut.weights is w and cut.draft_emb is True and cut.grids == pfx.grids
        assert tuple(cut.store.shape) == (4, 2, rows, 8) and cut.store.is_contiguous() and torch.equal(cut.store, pfx.store[:, :, :rows])
        assert torch.equal(cut.hidden, pfx.hidden[:rows]) and torch.equal(cut.emb, pfx.emb[:rows])
        assert torch.equal(cut.ids, pfx.ids[:, :rows]) and torch.equal(cut.image_mask, pfx.image_mask[:, :rows])
        assert (cut.pos3 is None) == (not qwen) and (not qwen or torch.equal(cut.pos3, pfx.pos3[:, :rows]))
        fields = ["store", "hidden", "emb", "ids", "image_mask"] + (["pos3"] if qwen else [])
        for f in fields:
            assert storage(getattr(cut, f)) != storage(getattr(pfx, f)), f"{f} shares memory with the source"
        cut.store.zero_(), cut.hidden.zero_(), cut.emb.zero_(), cut.ids.zero_()
        assert pfx.store.abs().sum() > 0 and pfx.hidden.abs().sum() > 0 and int(pfx.ids[0, 0]) == 5
        # a request on the cut prefix is checked like one on any other prefix
        assert pfx.truncated(rows).check_request(pfx.ids[:, :rows].repeat(1, 2)[:, :rows + 2], w, (IMG, VID)) == rows + 2


def test_truncated_refuses_rows_out_of_range_and_a_cut_through_a_visual_run():
    pfx = make_prefix(object())
    for rows in (0, -1, 10, 100):
        with pytest.raises(ValueError, match="rows"):
            pfx.truncated(rows)
    for rows in (1, 2, 3):  # the image run is rows 2 and 3: every True of the mask must lie below `rows`
        with pytest.raises(ValueError, match="visual run"):
            pfx.truncated(rows)
    assert pfx.truncated(4).rows == 4
    from vispec_amd.model.prefix import PromptPrefix
    text = PromptPrefix(pfx.store, pfx.hidden, pfx.emb, False, None, pfx.ids, weights=pfx.weights)  # no mask: any cut from row 1 on
    assert text.truncated(1).rows == 1 and text.truncated(1).image_mask is None


def fake_request(qwen, gen_ids, rope_delta=-3):
    """What a request start keeps of L = 6 prompt rows, the returned ids, and recording stand-ins for the engine and the embedding table."""
    ids = torch.tensor([[5, 6, IMG, IMG, 7, 8] + list(gen_ids)])
    P = ids.shape[1]
    hid = torch.arange(L * D, dtype=torch.float32).reshape(L, D).to(torch.bfloat16)
    prompt = SimpleNamespace(hidden=hid, emb=hid + 50, draft_emb=True, image_mask=ids[:, :L] == IMG,
                             pos3=torch.tensor([[0, 1, 2, 2, 3, 4], [0, 1, 2, 2, 3, 4], [0, 1, 2, 3, 4, 5]]) if qwen else None,
                             rope_delta=rope_delta if qwen else 0, grids=dict(image_grid_thw=[(1, 2, 4)]) if qwen else {}, weights=object())
    calls = []
    save = lambda rows: (calls.append(("save", rows)), torch.full((4, 2, rows, 8), 7.0, dtype=torch.bfloat16))[1]
    log = lambda row0, rows: (calls.append(("log", row0, rows)), torch.full((rows, D), -2.0, dtype=torch.bfloat16))[1]
    embed = lambda t: (calls.append(("embed", t.tolist())), t[:, None].float().expand(-1, D) * 0.5)[1]  # fp32: the helper casts to the prompt's dtype
    return prompt, ids, P, calls, save, log, embed


@pytest.mark.parametrize("qwen", [False, True])
def test_conversation_prefix_assembles_prompt_rows_and_generated_rows(qwen):
    from vispec_amd.model.prefix import PromptPrefix, conversation_prefix
    prompt, ids, P, calls, save, log, embed = fake_request(qwen, [20, 21, 22, 2])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        pfx = conversation_prefix(prompt, ids, (IMG, VID), save, log, embed)
    assert isinstance(pfx, PromptPrefix) and pfx.rows == P == 10 and pfx.weights is prompt.weights and pfx.draft_emb and pfx.grids == prompt.grids
    assert calls == [("save", P), ("log", L, P - L), ("embed", [20, 21, 22, 2])]
    assert tuple(pfx.store.shape) == (4, 2, P, 8)
    assert torch.equal(pfx.hidden[:L], prompt.hidden) and (pfx.hidden[L:] == -2.0).all() and tuple(pfx.hidden.shape) == (P, D)
    assert pfx.emb.dtype == torch.bfloat16 and torch.equal(pfx.emb[:L], prompt.emb)
    assert torch.equal(pfx.emb[L:], (torch.tensor([20, 21, 22, 2])[:, None].float().expand(-1, D) * 0.5).to(torch.bfloat16))
    assert torch.equal(pfx.ids, ids) and pfx.ids.device.type == "cpu"
    # the mask is extended with zeros
    assert pfx.image_mask.dtype == torch.bool and tuple(pfx.image_mask.shape) == (1, P)
    assert torch.equal(pfx.image_mask[:, :L], prompt.image_mask) and not pfx.image_mask[:, L:].any()
    if qwen:  # pos3 continues as p + rope_delta in three equal components
        assert tuple(pfx.pos3.shape) == (3, P) and pfx.pos3.dtype == prompt.pos3.dtype and torch.equal(pfx.pos3[:, :L], prompt.pos3)
        for c in range(3):
            assert pfx.pos3[c, L:].tolist() == [p - 3 for p in range(L, P)]
        # ... which is what PromptPrefix.extend asserts of the next turn's full rope index
        full = torch.cat([pfx.pos3, (torch.arange(P, P + 2) - 3)[None].expand(3, -1)], dim=1)
        nxt = torch.cat([ids, torch.tensor([[30, 31]])], dim=1)
        emb, mask, pos_new = pfx.extend(nxt, torch.zeros(2, D), full)
        assert tuple(emb.shape) == (P + 2, D) and tuple(mask.shape) == (1, P + 2) and torch.equal(pos_new, full[:, P:])
    else:
        assert pfx.pos3 is None
    # and the next turn's request passes the prefix's own checks; the prefix can be cut behind the image run
    assert pfx.check_request(torch.cat([ids, torch.tensor([[30]])], dim=1), prompt.weights, (IMG, VID)) == P + 1
    assert pfx.truncated(L + 2).rows == L + 2


def test_conversation_prefix_of_a_request_without_a_mask_and_without_generated_rows():
    from vispec_amd.model.prefix import conversation_prefix
    prompt, ids, P, calls, save, log, embed = fake_request(False, [])
    prompt.image_mask = None
    pfx = conversation_prefix(prompt, ids, (), save, log, embed)
    assert pfx.rows == L and pfx.image_mask is None and torch.equal(pfx.hidden, prompt.hidden) and torch.equal(pfx.emb, prompt.emb)
    assert calls == [("save", L), ("log", L, 0), ("embed", [])]


@pytest.mark.parametrize("bad", [IMG, VID])
def test_a_placeholder_id_among_the_generated_ids_gives_none_and_a_warning(bad):
    from vispec_amd.model.prefix import conversation_prefix
    prompt, ids, P, calls, save, log, embed = fake_request(True, [20, bad, 22])
    with pytest.warns(RuntimeWarning, match="placeholder"):
        assert conversation_prefix(prompt, ids, (IMG, VID), save, log, embed) is None
    assert calls == [], "nothing is copied for a prefix that is not returned"
    # the prompt's own placeholders (rows 2 and 3) do not count, and ids that are not watched do not either
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert conversation_prefix(prompt, ids, (-1, None), save, log, embed) is not None


def test_the_option_travels_as_a_keyword_only_when_it_is_on():
    from vispec_amd.model.spec_model_ours import _prefix_kw, _start_kw
    assert _prefix_kw(False) == {} and _prefix_kw(True) == {"return_prefix": True}
    off = _start_kw(0.0, 0.0, False, None, False, False)
    assert off == _start_kw(0.0, 0.0, False, None, False) == dict(temperature=0.0, top_k=0.0, is_llama3=False)
    assert _start_kw(0.0, 0.0, False, None, True, True) == dict(off, return_logprobs=True, return_prefix=True)
