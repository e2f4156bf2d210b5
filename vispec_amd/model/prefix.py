"""A prefilled prompt prefix that several requests share (SpecModel.prefill_prefix -> PromptPrefix; specgenerate*(prefix=...)): the K/V rows
of the first P prompt rows (system text + image) in a compact store, with everything a request start needs of those rows — so a request on
it runs the vision front-end never and the target prefill on its new rows only."""
from __future__ import annotations

import warnings
from typing import Optional

import torch


class PromptPrefix:
    """What SpecModel.prefill_prefix keeps of the first P rows of a prompt.  It owns
      store      K/V rows [0, P) of every layer, [2 * layers, H_kv, P, hd] bf16 (Engine.save_kv_rows: no memory shared with any cache)
      hidden     the target's post-final-norm hidden rows [P, D]
      emb        the merged input embeddings [P, D] (vision features scattered in)
      draft_emb  True: the draft prefill consumes `emb` (LLaVA-NeXT, Qwen2.5-VL); False: it embeds the ids with its own table
      image_mask bool [1, P] of the rows the draft compresses, or None
      ids        the P prompt ids [1, P] (on the host)
      pos3       Qwen2.5-VL: the multimodal rotary positions [3, P]; grids = the image / video grids and seconds-per-grid they came from
      weights    the TargetWeights it was computed with (identity: a request on other weights is refused)."""

    def __init__(self, store, hidden, emb, draft_emb, image_mask, ids, pos3=None, grids=None, weights=None):
        self.store, self.hidden, self.emb, self.draft_emb = store, hidden, emb, bool(draft_emb)
        self.image_mask, self.ids, self.pos3, self.grids, self.weights = image_mask, ids, pos3, dict(grids or {}), weights
        if ids.dim() != 2 or ids.shape[0] != 1 or not (ids.shape[1] == hidden.shape[0] == emb.shape[0] == store.shape[2]):
            raise ValueError("PromptPrefix: ids [1, P], hidden [P, D], emb [P, D] and a store of P rows")

    @property
    def rows(self) -> int:
        return int(self.ids.shape[1])

    @property
    def nbytes(self) -> int:
        ts = [self.store, self.hidden, self.emb, self.image_mask, self.ids, self.pos3]
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def check_request(self, input_ids, weights, visual_token_ids=()) -> int:
        """The refusals of a request on this prefix that need no device (ValueError each): other weights, a prompt no longer than the prefix,
        other leading ids, an image / video placeholder token behind the prefix.  -> the prompt's length L."""
        if weights is not self.weights:
            raise ValueError("prefix: this PromptPrefix was computed with other target weights (prefill_prefix of another model)")
        if input_ids is None or input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("prefix: a request on a prefix passes input_ids [1, L]")
        P, Ln = self.rows, int(input_ids.shape[1])
        if Ln <= P:
            raise ValueError(f"prefix: the prompt has {Ln} rows, the prefix {P}: at least one new row is needed for the logits")
        ids = input_ids.detach().cpu()
        if not torch.equal(ids[:, :P].long(), self.ids.long()):
            raise ValueError("prefix: the prompt does not begin with the prefix's ids")
        for tid in visual_token_ids:
            if tid is not None and int(tid) >= 0 and bool((ids[:, P:] == int(tid)).any()):
                raise ValueError("prefix: an image / video placeholder token behind the prefix (the prefix must contain every visual run)")
        return Ln

    def extend(self, input_ids, suffix_emb, pos3_full: Optional[torch.Tensor] = None):
        """The request's prompt on this prefix: -> (emb [L, D] = cat(prefix emb, suffix_emb), image mask [1, L] | None, positions of the new
        rows [3, L - P] | None).  pos3_full: the multimodal rotary positions of the FULL prompt (Qwen2.5-VL) — their first P columns must be
        the prefix's, else the visual runs are not all inside the prefix."""
        P, Ln = self.rows, int(input_ids.shape[1])
        if suffix_emb.shape[0] != Ln - P:
            raise ValueError("prefix: one embedding row per new prompt row")
        emb = torch.cat([self.emb, suffix_emb.to(self.emb.dtype)], dim=0).contiguous()
        mask = None
        if self.image_mask is not None:
            mask = torch.cat([self.image_mask, torch.zeros(1, Ln - P, dtype=self.image_mask.dtype, device=self.image_mask.device)], dim=1)
        pos_new = None
        if self.pos3 is not None:
            if pos3_full is None or pos3_full.shape[-1] != Ln:
                raise ValueError("prefix: a Qwen2.5-VL request needs the rotary positions of its full prompt")
            assert torch.equal(pos3_full[:, :P].cpu().long(), self.pos3.cpu().long()), "the prefix's rotary positions changed under the full prompt"
            pos_new = pos3_full[:, P:]
        return emb, mask, pos_new

    def truncated(self, rows: int) -> "PromptPrefix":
        """The first `rows` rows as a new prefix that shares no memory with this one (the store is sliced into a new contiguous tensor, every
        other field is sliced and copied): how a caller cuts a returned conversation prefix at the EOS the returned ids keep, or at a
        chat-template boundary.  ValueError unless 1 <= rows <= self.rows and every row of image_mask that is set lies below `rows`."""
        rows = int(rows)
        if not 1 <= rows <= self.rows:
            raise ValueError(f"truncated: {rows} rows of a prefix of {self.rows}")
        if self.image_mask is not None and bool(self.image_mask[:, rows:].any()):
            raise ValueError(f"truncated: a visual run reaches behind row {rows} (a prefix holds whole visual runs)")
        return PromptPrefix(self.store[:, :, :rows].clone(memory_format=torch.contiguous_format), self.hidden[:rows].clone(), self.emb[:rows].clone(), self.draft_emb,
                            None if self.image_mask is None else self.image_mask[:, :rows].clone(), self.ids[:, :rows].clone(),
                            pos3=None if self.pos3 is None else self.pos3[:, :rows].clone(), grids=self.grids, weights=self.weights)


def conversation_prefix(prompt, ids, visual_token_ids, save_kv_rows, hidden_log, embed_tokens) -> Optional[PromptPrefix]:
    """A finished request as the prompt prefix of the conversation's next turn: P = ids.shape[1] rows, every row of the returned ids [1, P].
    prompt = what the request's start kept of its L prompt rows: hidden [L, D], emb [L, D], draft_emb, image_mask [1, L] | None,
    pos3 [3, L] | None, rope_delta, grids, weights.  save_kv_rows(P) -> the K/V store, hidden_log(L, P - L) -> the generated rows' hidden,
    embed_tokens(ids [P - L]) -> their input embeddings (Engine.save_kv_rows, Engine.hidden_log, the target's embedding table).
      hidden / emb   the prompt's rows followed by the generated rows' (emb in the prompt's dtype)
      image_mask     the prompt's, extended with zeros
      pos3           the prompt's columns, then p + rope_delta in all three components for p in [L, P): what the rope index of the full
                     ids gives text rows behind the last visual run (PromptPrefix.extend asserts it on the next turn)
    Arithmetic class: prompt rows are the bytes the request started with; generated rows come from the verify kernels of the rounds (their
    K/V from the cache at the finish, their hidden byte for byte what the rounds handed to the draft) — the oracle's arithmetic within the
    bf16 bars, not the bytes a prefill of the whole conversation would give.
    -> None, with a RuntimeWarning and before anything is copied, when a generated id is one of visual_token_ids: the next turn's rope
    index and PromptPrefix.check_request could not be honoured."""
    L, P = int(prompt.hidden.shape[0]), int(ids.shape[1])
    gen = ids[0, L:]
    for tid in visual_token_ids:
        if tid is not None and int(tid) >= 0 and bool((gen == int(tid)).any()):
            warnings.warn(f"return_prefix: the generated ids contain the image / video placeholder id {int(tid)}; no prefix is returned",
                          RuntimeWarning)
            return None
    store = save_kv_rows(P)
    hidden = torch.cat([prompt.hidden, hidden_log(L, P - L)], dim=0)
    emb = torch.cat([prompt.emb, embed_tokens(gen).to(prompt.emb.dtype)], dim=0)
    mask = prompt.image_mask
    if mask is not None:
        mask = torch.cat([mask.reshape(1, L), torch.zeros(1, P - L, dtype=mask.dtype, device=mask.device)], dim=1)
    pos3 = prompt.pos3
    if pos3 is not None:
        tail = torch.arange(L, P, dtype=pos3.dtype, device=pos3.device) + int(prompt.rope_delta)
        pos3 = torch.cat([pos3, tail[None].expand(3, -1)], dim=1)
    return PromptPrefix(store, hidden, emb, prompt.draft_emb, mask, ids.detach().cpu(), pos3=pos3, grids=prompt.grids, weights=prompt.weights)
