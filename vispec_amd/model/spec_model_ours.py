"""SpecModel — the reference's spec-decoding API (vispec/model/spec_model_ours.py): from_pretrained (:109-203),
forward (:205-245), specgenerate (:247-582), get_tokenizer (:101-107), and the attributes the harness reads
(base_model, spec_layer, past_key_values, past_key_values_data, current_length_data, tokenizer).

MI355X design: one SpecModel = one process = one GPU = one `vispec_ctx`.  specgenerate() runs the target prefill in
PyTorch, then each draft-and-verify round is three stream-ordered C calls (verify+accept, draft round, state read-back)
with exactly one host sync per round (the reference has >= 10)."""
from __future__ import annotations

import json
import os
import time
import warnings
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .. import lib as L
from ..engine import DraftConfig, DraftWeightsDev, Engine, TargetConfig, TargetWeights
from .cnets_ours import Model
from .kv_cache import initialize_past_key_values
from .prefix import PromptPrefix, conversation_prefix
from .target import TargetLM
from .utils import initialize_tree, reset_tree_mode


class SpecModel:
    def __init__(self, base_model: TargetLM, spec_layer: Model, tokenizer=None, total_token=30, depth=3, top_k=8, num_q=2,
                 kv_max_pos: Optional[int] = None, draft_max_pos: Optional[int] = None, target_weight_dtype: str = "bf16",
                 cohort_leader: Optional["SpecModel"] = None):
        """cohort_leader: build this model as the second member of a two-request cohort (same weights objects as the leader): see
        specgenerate_cohort()."""
        self.base_model = base_model
        self.config = base_model.config
        self.hidden_size = base_model.cfg.hidden_size
        self.vocab_size = base_model.cfg.vocab_size
        self.tokenizer = tokenizer or SimpleNamespace(eos_token_id=base_model.cfg.eos_token_id, vocab_size=base_model.cfg.vocab_size)
        self.spec_layer = spec_layer
        self.engine = Engine(base_model.cfg, spec_layer.config, base_model.w, spec_layer.w, total_token=total_token, depth=depth,
                             top_k=top_k, num_q=num_q, kv_max_pos=kv_max_pos, draft_max_pos=draft_max_pos,
                             target_weight_dtype=target_weight_dtype, leader=None if cohort_leader is None else cohort_leader.engine)
        base_model.engine = self.engine
        spec_layer.engine = self.engine
        spec_layer.init_tree()
        self.training = False
        self._last_embeds = None

    def eval(self):
        return self

    def make_cohort_member(self) -> "SpecModel":
        """A second model over the SAME weight tensors (nothing is copied or re-packed) whose engine is a cohort member of this one's:
        own KV caches, tree and round state; specgenerate_cohort([self, member], [req_a, req_b]) then runs two requests per weight pass."""
        e = self.engine
        base = TargetLM(self.base_model.cfg, self.base_model.w, vision=self.base_model.vision)
        draft = Model(self.spec_layer.config, self.spec_layer.w, total_tokens=e.total_token, depth=e.depth, top_k=e.top_k, num_q=e.num_q)
        return SpecModel(base, draft, tokenizer=self.tokenizer, total_token=e.total_token, depth=e.depth, top_k=e.top_k, num_q=e.num_q,
                         kv_max_pos=e.kv_max_pos, draft_max_pos=e.draft_max_pos, target_weight_dtype=e.target_weight_dtype, cohort_leader=self)

    def get_tokenizer(self):
        return self.tokenizer

    # ------------------------------------------------------------------------------------------------
    @classmethod
    def from_weights(cls, tcfg: TargetConfig, dcfg: DraftConfig, target_sd, draft_sd, device="cuda:0", **kw):
        """Build from in-memory state dicts (numpy / torch) with the reference's names."""
        device = torch.device(device)
        num_q = kw.get("num_q", 2)
        tw = TargetWeights.from_state_dict(tcfg, target_sd, device)
        dw = DraftWeightsDev.from_state_dict(dcfg, draft_sd, num_q, device)
        base = TargetLM(tcfg, tw)
        draft = Model(dcfg, dw, total_tokens=kw.get("total_token", 30), depth=kw.get("depth", 3), top_k=kw.get("top_k", 8),
                      num_q=num_q)
        return cls(base, draft, **kw)

    @classmethod
    def from_pretrained(cls, Type="LLaMA", base_model_path=None, spec_model_path=None, total_token=30, depth=3, top_k=8,
                        threshold=1.0, num_q=2, device="cuda:0", **kwargs):
        """spec_model_ours.py:109-203.  Local directories only (there is no network on the GPU box):
        base_model_path = HF checkpoint dir of the target (config.json + *.safetensors [+ index]),
        spec_model_path = ViSpec draft dir (config.json + model.safetensors | pytorch_model.bin)."""
        from ..weights_io import load_draft_dir, load_target_dir  # imported lazily: safetensors is optional at import time
        tcfg, target_sd, tokenizer = load_target_dir(base_model_path)
        dcfg, draft_sd = load_draft_dir(spec_model_path, tcfg)
        model = cls.from_weights(tcfg, dcfg, target_sd, draft_sd, device=device, total_token=60 if total_token == -1 else total_token,
                                 depth=depth, top_k=top_k, num_q=num_q, tokenizer=tokenizer,
                                 target_weight_dtype=kwargs.get("target_weight_dtype", "bf16"))  # "fp8" / "fp8a8": quantised at load (engine.py)
        if tcfg.architectures[0] not in ("LlamaForCausalLM", "Qwen2ForCausalLM"):
            # vision tower + projector of the checkpoint (PyTorch-ROCm, HF modules): SURVEY §8 A2
            from .vision import HFVisionFrontEnd
            try:
                model.base_model.vision = HFVisionFrontEnd.from_dir(base_model_path, device, torch.bfloat16)
            except (FileNotFoundError, ImportError) as e:
                warnings.warn(f"{base_model_path}: no usable vision weights ({e}); image prompts need precomputed features")
        if total_token == -1:
            model.autotune_total_token()
        return model

    def autotune_total_token(self, cans=(40, 48, 50, 56, 60), x=(1, 1.05, 1.07, 1.1, 1.13), iters=20):
        """spec_model_ours.py:179-201: time the target forward on `length` tokens for each candidate tree size, weight the times by
        x, keep the cheapest.  Here the timed forward is the one the loop actually runs (the HIP verify pass on a `length`-node chain)."""
        eng, times = self.engine, []
        g = torch.Generator().manual_seed(0)
        for length in cans:
            self.spec_layer.total_tokens = length - 1
            ids = torch.randint(0, max(2, self.vocab_size - 200), (length,), generator=g).numpy().astype(np.int32)
            eng.begin_request(ids[:1], 8)
            causal = np.array([(1 << (i + 1)) - 1 for i in range(length)], np.uint64)
            eng.set_tree(ids, np.arange(length, dtype=np.int32), causal, np.zeros((1, 1), np.int32))
            eng.target_forward()
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(iters):
                eng.target_forward()
            torch.cuda.synchronize()
            times.append((time.time() - t0) / x[len(times)])
        best = cans[times.index(min(times))]
        self.spec_layer.total_tokens = best - 1
        return best

    # ------------------------------------------------------------------------------------------------
    def _first_token(self, orig: torch.Tensor) -> torch.Tensor:
        """argmax(orig[:, -1]) (utils.py:290) via the HIP argmax kernel on the bf16-rounded logits (first max wins)."""
        import ctypes as C
        row = orig.reshape(-1, orig.shape[-1])[-1:].to(torch.bfloat16).contiguous()
        out = torch.zeros(1, dtype=torch.int32, device=row.device)
        L.check(self.engine.lib.vispec_argmax_rows(self.engine.h, self.engine._stream(), C.c_void_p(row.data_ptr()), row.shape[-1], 1,
                                                   row.shape[-1], C.c_void_p(out.data_ptr())))
        return out

    def forward(self, input_ids=None, attention_mask=None, past_key_values=None, output_orig=False, position_ids=None,
                inputs_embeds=None, output_real_hidden=False, **kwargs):
        """spec_model_ours.py:205-245: ONE function serving both callers of the reference —
          * utils.initialize_tree (utils.py:280-283): empty KV cache -> the PREFILL form (PyTorch-ROCm GEMMs + SDPA, K/V written in place);
          * utils.tree_decoding (utils.py:404-409): non-empty cache, `input_ids` = the T tree candidates, `position_ids` =
            tree_position_ids + n (x3, + rope_deltas for Qwen2.5-VL), tree mask installed on `base_model.model.tree_mask`
            (spec_model_ours.py:486-489) -> the VERIFY form (vispec_target_forward: HIP kernels, K/V rows appended at [n, n+T)).
        Returns (None[, logits fp32 [1,S,V]], hidden [1,S,D]) (post-final-norm hidden, modeling_llama_kv.py:1062-1066)."""
        n_past = 0
        if past_key_values is not None:
            n_past = int(past_key_values[0][0].current_length.item())  # `past_key_values[0][0].shape[2]` of modeling_llama_kv.py:957
        if n_past > 0:
            return self._forward_verify(input_ids, past_key_values, output_orig, position_ids, inputs_embeds)
        if inputs_embeds is None:
            inputs_embeds = self.base_model.get_input_embeddings()(input_ids.to(self.engine.device))
        emb = inputs_embeds.reshape(-1, inputs_embeds.shape[-1]).to(torch.bfloat16).contiguous()
        self._last_embeds = None if input_ids is not None and kwargs.get("_draft_embeds_from_ids") else emb[None]
        pos3 = position_ids if (position_ids is not None and position_ids.dim() == 3) else None
        logits, hidden = self.base_model.prefill(emb, all_logits=bool(kwargs.get("all_logits", False)),
                                                 position_ids=None if pos3 is None else pos3[:, 0].cpu())
        # device-side round state: context = the L prefilled rows (utils.initialize_tree re-issues this with the prompt ids)
        ids0 = (input_ids.reshape(-1).cpu().numpy() if input_ids is not None and input_ids.numel() == emb.shape[0]
                else np.zeros(emb.shape[0], np.int32))
        self.engine.begin_request(ids0, 1 << 20)
        if past_key_values is not None:
            for kv in past_key_values:
                kv[0].current_length.fill_(emb.shape[0])
                kv[1].current_length.fill_(emb.shape[0])
        if output_orig:
            return None, logits[None], hidden[None]
        return None, hidden[None]

    def _forward_verify(self, input_ids, past_key_values, output_orig, position_ids, inputs_embeds):
        """The verify form of forward(): S <= 64 new tokens against the committed context of the engine."""
        eng = self.engine
        if input_ids is None or inputs_embeds is not None:
            raise NotImplementedError("forward() with a non-empty KV cache takes token ids (the tree candidates); the reference's "
                                      "loop never passes inputs_embeds there (utils.py:404-409)")
        ids = input_ids.reshape(-1).cpu().numpy().astype(np.int32)
        S = int(ids.shape[0])
        if S < 1 or S > L.TREE_MAX_T:
            raise ValueError(f"forward() with a non-empty KV cache handles 1..{L.TREE_MAX_T} tokens per call (one tree), got {S}")
        st = eng.state()
        n = int(st["n_ctx"])  # authoritative context length (the host mirror in past_key_values is refreshed below)
        # relative positions = depth in the tree (utils.py:397: position_ids = tree_position_ids + input_ids.shape[1])
        if position_ids is None:
            pos_rel = np.arange(S, dtype=np.int64)
        else:
            p = position_ids
            if p.dim() == 3:  # Qwen2.5-VL: [3, 1, T], the three components are equal in the decode phase (utils.py:398-402)
                p = p[0]
            pos_rel = p.reshape(-1).cpu().numpy().astype(np.int64) - n - int(getattr(self, "_rope_delta", 0))
        if pos_rel.shape[0] != S or pos_rel.min() < 0 or pos_rel.max() >= S:
            raise ValueError("position_ids of a verify forward must be tree depths offset by the context length "
                             f"(n = {n}{', + rope_deltas' if getattr(self, '_rope_delta', 0) else ''})")
        tm = self.base_model.tree_mask
        bits = np.zeros(L.TREE_MAX_T, np.uint64)
        if tm is None:  # no tree mask installed: plain causal continuation (modeling_llama_kv.py:890-924 without the tree branch)
            for i in range(S):
                bits[i] = np.uint64((1 << (i + 1)) - 1)
        else:
            m = (tm.reshape(tm.shape[-2], tm.shape[-1]).cpu().numpy() > 0)
            if m.shape != (S, S):
                raise ValueError(f"tree_mask {m.shape} does not match the {S} tree tokens")
            for i in range(S):
                bits[i] = np.uint64(sum(1 << j for j in range(S) if m[i, j]))
        restore = None
        if S != eng.total_token:
            restore = eng.total_token
            eng.set_total_token(S)
        try:
            eng.set_tree(ids, pos_rel.astype(np.int32), bits, None)
            eng.target_forward()
            V, D = eng.tcfg.vocab_size, eng.tcfg.hidden_size
            logits = eng.buffer("logits", (64, V))[:S].float()[None]  # `.float()` of modeling_llama_kv.py:1197
            hidden = eng.buffer("hidden_new", (64, D))[:S].clone()[None]
        finally:
            if restore is not None:
                eng.set_total_token(restore)
        for kv in past_key_values:  # KVCache.cat appended S rows (kv_cache.py:40-58); update_inference_inputs resets the lengths
            kv[0].current_length.fill_(n + S)
            kv[1].current_length.fill_(n + S)
        if output_orig:
            return None, logits, hidden
        return None, hidden

    __call__ = forward

    def _merge_vision(self, input_ids, inputs_embeds, kwargs):
        """spec_model_ours.py:309-453: token embeddings, image features scattered over the placeholder tokens, and the
        image mask the draft compresses with.
        -> (inputs_embeds | None, special_image_mask | None, draft_embeds | None, position_ids [3,L] | None, rope_delta)."""
        special_image_mask = None
        arch = self.base_model.config.architectures[0]
        draft_embeds = None
        position_ids, rope_delta = None, 0
        if arch == "LlavaNextForConditionalGeneration":  # :311-378
            pixel_values = kwargs.get("pixel_values")
            image_sizes = kwargs.get("image_sizes")
            if pixel_values is not None and inputs_embeds is not None:
                raise ValueError("You cannot specify both pixel_values and inputs_embeds at the same time, and must specify either one")
            if inputs_embeds is None:
                inputs_embeds = self.base_model.get_input_embeddings()(input_ids)
            if pixel_values is not None:
                image_features = self.base_model.get_image_features(pixel_values, image_sizes)
                image_features, _ = self.base_model.pack_image_features(image_features, image_sizes)
                mask = input_ids == self.base_model.config.image_token_index
                n_tok = int(mask.sum())
                if n_tok != image_features.shape[0]:  # :363-370
                    raise ValueError(f"Image features and image tokens do not match: tokens: {n_tok}, features {image_features.shape[0]}")
                inputs_embeds = inputs_embeds.clone()
                inputs_embeds[mask] = image_features.to(inputs_embeds.dtype)
                special_image_mask = mask
            draft_embeds = inputs_embeds
        elif arch == "LlavaForConditionalGeneration":
            # LLaVA-1.5: the reference's specgenerate has NO vision branch for it: the target merges the
            # image features itself (HF forward with pixel_values), while the draft gets inputs_embeds=None / image_mask=None, i.e.
            # it embeds the ids (placeholder tokens included) with its own table and never compresses (g = 0).
            pixel_values = kwargs.get("pixel_values")
            if inputs_embeds is None:
                inputs_embeds = self.base_model.get_input_embeddings()(input_ids)
                if pixel_values is not None:
                    feats = self.base_model.get_image_features(pixel_values, kwargs.get("image_sizes"))
                    mask = input_ids == self.base_model.config.image_token_index
                    if int(mask.sum()) != feats.shape[0]:
                        raise ValueError(f"Image features and image tokens do not match: tokens: {int(mask.sum())}, features {feats.shape[0]}")
                    inputs_embeds = inputs_embeds.clone()
                    inputs_embeds[mask] = feats.to(inputs_embeds.dtype)
        elif arch == "Qwen2_5_VLForConditionalGeneration":  # :380-453
            pixel_values, grid = kwargs.get("pixel_values"), kwargs.get("image_grid_thw")
            pixel_values_videos, vgrid = kwargs.get("pixel_values_videos"), kwargs.get("video_grid_thw")
            if inputs_embeds is None:
                inputs_embeds = self.base_model.get_input_embeddings()(input_ids)
                for pv, g_, tid, what in ((pixel_values, grid, self.base_model.config.image_token_id, "Image"),
                                          (pixel_values_videos, vgrid, self.base_model.cfg.video_token_id, "Video")):
                    if pv is None:
                        continue
                    feats = self.base_model.get_image_features(pv, image_grid_thw=g_)  # the same visual tower serves both (:393-395, 426-428)
                    mask = input_ids == tid
                    if int(mask.sum()) != feats.shape[0]:  # :403-406 / :435-438
                        raise ValueError(f"{what} features and {what.lower()} tokens do not match: tokens: {int(mask.sum())}, features {feats.shape[0]}")
                    inputs_embeds = inputs_embeds.clone()
                    inputs_embeds[mask] = feats.to(inputs_embeds.dtype)
                    special_image_mask = mask  # the reference keeps the LAST mask it built (:420,453): with a video, the draft compresses
                    #                            the video runs and sees image tokens as ordinary rows
            draft_embeds = inputs_embeds
            # multimodal rotary positions of the prefill + rope_delta of the decode rounds: get_rope_index over image AND video grids,
            # video frames at floor(frame * second_per_grid_ts * tokens_per_second) (modeling_qwen2_5_vl_kv.py:1789-1975, 2157-2163)
            position_ids, rope_delta = self._qwen_rope(input_ids, grid, video_grid=vgrid, second_per_grid_ts=kwargs.get("second_per_grid_ts"))
        elif arch in ("LlamaForCausalLM", "Qwen2ForCausalLM"):
            pass  # text targets (Qwen2 = the same decoder with q/k/v bias, modeling_qwen2_kv.py): the draft embeds the ids itself (cnets_ours.py:1099-1107)
        else:
            raise NotImplementedError(f"target architecture {arch}")
        return inputs_embeds, special_image_mask, draft_embeds, position_ids, rope_delta

    def _qwen_rope(self, input_ids, grid, video_grid=None, second_per_grid_ts=None):
        """Multimodal rotary positions [3, L] + rope_delta of a Qwen2.5-VL prompt (get_rope_index: image and video grids), cached on the
        target like the reference's prefill does (modeling_qwen2_5_vl_kv.py `self.rope_deltas`; read back by utils.tree_decoding, utils.py:398-400)."""
        from ..synth import qwen_rope_index
        as_grids = lambda g: [] if g is None else [tuple(int(v) for v in g3) for g3 in (g.tolist() if torch.is_tensor(g) else g)]
        sec = None
        if second_per_grid_ts is not None:
            sec = [float(v) for v in (second_per_grid_ts.tolist() if torch.is_tensor(second_per_grid_ts) else second_per_grid_ts)]
        cfg = self.base_model.cfg
        pos3, rope_delta = qwen_rope_index(input_ids[0].cpu().numpy(), self.base_model.config.image_token_id, as_grids(grid),
                                           video_token_id=cfg.video_token_id if cfg.video_token_id >= 0 else None,
                                           video_grids=as_grids(video_grid), second_per_grid_ts=sec, tokens_per_second=cfg.tokens_per_second)
        self.base_model.rope_deltas = torch.tensor([[rope_delta]], device=input_ids.device)
        return torch.from_numpy(pos3), int(rope_delta)

    def _embed_prompt(self, input_ids, inputs_embeds, kwargs):
        """The prompt as both kinds of request start consume it: -> (ids on the device, embeddings [L, D] bf16 with the vision features merged
        in, then _merge_vision's image mask, draft embeddings, position ids and rope delta).  No side effect on the engine or the caches."""
        input_ids = input_ids.clone().to(self.engine.device)
        inputs_embeds, *rest = self._merge_vision(input_ids, inputs_embeds, kwargs)
        emb = inputs_embeds if inputs_embeds is not None else self.base_model.get_input_embeddings()(input_ids)
        return (input_ids, emb.reshape(-1, emb.shape[-1]).to(torch.bfloat16).contiguous(), *rest)

    @torch.no_grad()
    def _start_prepare(self, input_ids, inputs_embeds, kwargs, temperature=0.0, top_k=0.0, seed=0, max_new_tokens=512, is_llama3=False,
                       prefix=None, return_logprobs=False, return_prefix=False, top_logprobs=0):
        """First stage of a request start, everything before the target prefill (spec_model_ours.py:272-456): sampling config, KV reset,
        vision merge, embeddings.  Returns the state the later stages need.
        prefix (a PromptPrefix): the request's first `prefix.rows` rows are the prefix's — refused with ValueError before anything is touched
        when they are not (PromptPrefix.check_request); only the new ids are embedded, no vision kwargs are read, the vision front-end does
        not run; `position_ids` of the result are those of the new rows, `past` = prefix.rows.
        return_logprobs: the engine's rounds also log the target log-probability of every token they commit (Engine.set_logprobs).
        top_logprobs = N > 0 (with return_logprobs): ... and the N best tokens of every row they commit from (Engine.set_top_logprobs).
        return_prefix: the engine's rounds also keep the hidden row of every position they commit (Engine.set_hidden_log), and the result
        keeps the grids the prompt's positions came from — what _request_result needs to hand the finished request back as a PromptPrefix."""
        if prefix is not None:
            prefix.check_request(input_ids, self.base_model.w, self._visual_token_ids())
        self.engine.set_logprobs(return_logprobs)
        self.engine.set_top_logprobs(top_logprobs)
        self.engine.set_hidden_log(return_prefix)
        grids = None
        if return_prefix:
            grids = prefix.grids if prefix is not None else \
                {k: kwargs.get(k) for k in ("image_grid_thw", "video_grid_thw", "second_per_grid_ts") if kwargs.get(k) is not None}
        self.engine.set_sampling(temperature if temperature > 1e-5 else 0.0, seed, top_k=int(top_k) if temperature > 1e-5 else 0)
        self.spec_layer.reset_kv()  # :283
        if not hasattr(self, "past_key_values"):  # :286-307
            self.past_key_values, self.past_key_values_data, self.current_length_data = initialize_past_key_values(self.base_model)
        self.current_length_data.zero_()
        if prefix is None:
            input_ids, emb, special_image_mask, draft_embeds, position_ids, rope_delta = self._embed_prompt(input_ids, inputs_embeds, kwargs)
        else:
            input_ids, emb, special_image_mask, draft_embeds, position_ids, rope_delta = self._embed_on_prefix(input_ids, prefix)
        reset_tree_mode(self)  # :456
        # initialize_tree (:458-475) follows: prefill + first token + draft prefill with image-token compression
        return SimpleNamespace(input_ids=input_ids, emb=emb, position_ids=position_ids, rope_delta=rope_delta, draft_embeds=draft_embeds,
                               special_image_mask=special_image_mask, temperature=temperature, max_new_tokens=max_new_tokens, is_llama3=is_llama3,
                               prefix=prefix, past=0 if prefix is None else prefix.rows, return_logprobs=bool(return_logprobs),
                               top_logprobs=int(top_logprobs), return_prefix=bool(return_prefix), grids=grids)

    def _visual_token_ids(self):
        """The placeholder ids that the vision merge replaces in a prompt of this target (none for a text target)."""
        arch, cfg = self.base_model.config.architectures[0], self.base_model.cfg
        if arch in ("LlavaNextForConditionalGeneration", "LlavaForConditionalGeneration"):
            return (cfg.image_token_index,)
        if arch == "Qwen2_5_VLForConditionalGeneration":
            return (cfg.image_token_index, cfg.video_token_id)
        return ()

    def _embed_on_prefix(self, input_ids, prefix):
        """_embed_prompt for a request on a PromptPrefix: the prefix's merged embeddings followed by embed_tokens of the new ids; for
        Qwen2.5-VL the rotary index of the FULL ids over the kept grids (rope_delta is the full prompt's), of which the new rows' columns are
        returned.  -> the tuple of _embed_prompt, with position_ids [3, L - P] | None."""
        input_ids = input_ids.clone().to(self.engine.device)
        P = prefix.rows
        new_emb = self.base_model.get_input_embeddings()(input_ids[0, P:]).to(torch.bfloat16)
        pos_full, rope_delta = None, 0
        if prefix.pos3 is not None:
            g = prefix.grids
            pos_full, rope_delta = self._qwen_rope(input_ids, g.get("image_grid_thw"), video_grid=g.get("video_grid_thw"),
                                                   second_per_grid_ts=g.get("second_per_grid_ts"))
        emb, mask, pos_new = prefix.extend(input_ids, new_emb, pos_full)
        return input_ids, emb, mask, (emb if prefix.draft_emb else None), pos_new, rope_delta

    @torch.no_grad()
    def prefill_prefix(self, input_ids, prefill_chunk_rows=None, **kwargs):
        """Prefill the first P rows of a prompt ONCE — input_ids [1, P] with the vision kwargs of specgenerate (the vision front-end, the merge
        and, for Qwen2.5-VL, the rope index run here) — on this model's own cache, and keep them: -> a PromptPrefix owning a compact copy of
        K/V rows [0, P) of every layer (Engine.save_kv_rows: one copy launch, no memory shared with the cache), the hidden rows, the merged
        embeddings, the image mask, the ids and, for Qwen2.5-VL, the [3, P] positions and the grids.  prefill_chunk_rows: TargetLM.prefill's
        chunk_rows.  Any request of this model or of its cohort members whose prompt begins with these rows and has every image / video run
        inside them can then start with specgenerate*(..., prefix=...).  No request state is begun and no draft work runs: the model is
        ready for an ordinary request afterwards (every request start resets its slot)."""
        ids, emb, mask, draft_embeds, pos, _ = self._embed_prompt(input_ids, None, kwargs)
        _, hidden = self.base_model.prefill(emb, position_ids=pos, **_chunk_kw("chunk_rows", prefill_chunk_rows))
        store = self.engine.save_kv_rows(int(emb.shape[0]))
        grids = {k: kwargs.get(k) for k in ("image_grid_thw", "video_grid_thw", "second_per_grid_ts") if kwargs.get(k) is not None}
        return PromptPrefix(store, hidden, emb, draft_embeds is not None, mask, ids.cpu(), pos3=pos, grids=grids, weights=self.base_model.w)

    @torch.no_grad()
    def _start_finish(self, prep, logits, hidden):
        """Last stage of a request start, everything after the target prefill (spec_model_ours.py:458-475): first token, device round state,
        rope delta, stop token, draft prefill with image-token compression + the first tree."""
        eng, input_ids, emb = self.engine, prep.input_ids, prep.emb
        first = eng.sample_row(logits[-1]) if prep.temperature > 1e-5 else self._first_token(logits)
        eng.begin_request(input_ids[0].cpu().numpy(), prep.max_new_tokens)
        self._prompt_len = int(input_ids.shape[1])
        if prep.return_logprobs:  # the first token's value: the row that chose it, whichever prefill produced it
            eng.token_logprob_row(logits[-1], first, self._prompt_len)
        if prep.top_logprobs:  # ... and its top-N entry, from the same row
            eng.token_top_logprob_row(logits[-1], self._prompt_len)
        self._rope_delta = int(prep.rope_delta)
        if prep.rope_delta:
            eng.set_rope_delta(prep.rope_delta)
        if prep.is_llama3:  # :268-269, 540-542
            eng.set_stop_token(int(self.tokenizer.convert_tokens_to_ids("<|eot_id|>")))
        if prep.draft_embeds is None:
            ids1 = torch.cat([input_ids[0], first.long()])
            demb = torch.nn.functional.embedding(ids1[:-1], self.spec_layer.w.t["embed"]).contiguous()
        else:
            demb = emb
        mask_np = None if prep.special_image_mask is None else prep.special_image_mask.reshape(-1).cpu().numpy()
        eng.draft_prefill(hidden, demb, mask_np, first)
        self.spec_layer.stable_kv = ("device", eng)
        # return_prefix: the prompt rows as this start has them, whoever produced them (references only; nothing is kept otherwise)
        self._prompt_rows = None
        if prep.return_prefix:
            pos3 = prep.position_ids
            if pos3 is not None and prep.prefix is not None:
                pos3 = torch.cat([prep.prefix.pos3, pos3.to(prep.prefix.pos3.device, prep.prefix.pos3.dtype)], dim=1)
            self._prompt_rows = SimpleNamespace(hidden=hidden, emb=emb, draft_emb=prep.draft_embeds is not None, image_mask=prep.special_image_mask,
                                                pos3=pos3, rope_delta=int(prep.rope_delta), grids=prep.grids, weights=self.base_model.w)
        return hidden, demb, mask_np, first

    @torch.no_grad()
    def _start_request(self, input_ids, inputs_embeds, kwargs, temperature=0.0, top_k=0.0, seed=0, max_new_tokens=512, is_llama3=False,
                       prefill_chunk_rows=None, prefix=None, return_logprobs=False, return_prefix=False, top_logprobs=0):
        """Everything specgenerate does before its loop (spec_model_ours.py:272-475): sampling config, KV reset, vision merge, target
        prefill, first token, device round state, draft prefill with image-token compression + the first tree.
        Returns (hidden [L,D], draft_embeds [L,D], image_mask numpy | None, first_token int32 [1]) — what the draft prefill consumed.
        prefill_chunk_rows: TargetLM.prefill's chunk_rows (the draft prefill is unchanged: it consumes the full [L, D] hidden).
        prefix: a PromptPrefix the prompt begins with (the staged route of _start_requests)."""
        if prefix is not None:
            return _start_requests([self], [(input_ids, kwargs)], [seed], [max_new_tokens],
                                   _start_kw(temperature, top_k, is_llama3, prefill_chunk_rows, return_logprobs, return_prefix, top_logprobs),
                                   prefixes=[prefix])[0]
        prep = self._start_prepare(input_ids, inputs_embeds, kwargs, temperature=temperature, top_k=top_k, seed=seed,
                                   max_new_tokens=max_new_tokens, is_llama3=is_llama3, return_logprobs=return_logprobs,
                                   **_prefix_kw(return_prefix), **_top_kw(top_logprobs))
        # (raises before touching the KV when the prompt cannot fit)
        logits, hidden = self.base_model.prefill(prep.emb, position_ids=prep.position_ids, **_chunk_kw("chunk_rows", prefill_chunk_rows))
        return self._start_finish(prep, logits, hidden)

    # ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def specgenerate(self, input_ids, temperature=0.0, top_p=0.0, top_k=0.0, max_new_tokens=512, max_length=2048, log=False,
                     is_llama3=False, inputs_embeds=None, return_acceptance_len=False, return_decode_time=False,
                     forced_accept=None, seed=0, prefill_chunk_rows=None, prefix=None, return_logprobs=False, return_prefix=False, top_logprobs=0,
                     **kwargs):
        """spec_model_ours.py:247-582.  `forced_accept` (callable round->int, bench-only) scripts the accept length.
        return_prefix=True appends, LAST in the output tuple (behind the logprobs entry when both are asked for), the finished request as a
        PromptPrefix of every row of the returned ids — the next turn of the conversation then runs as specgenerate(next_ids, prefix=that,
        return_prefix=True), turn after turn: no vision front-end, no prefill of anything already in the cache.  Cut it with
        PromptPrefix.truncated at the EOS the returned ids keep, or at a chat-template boundary.  The entry is None, with a RuntimeWarning,
        when the generated ids contain an image / video placeholder id (no later request could be checked or positioned on it); the other
        outputs are unaffected.  Arithmetic class: the prompt rows of the returned prefix are the bytes the request started with; the
        generated rows' K/V are the cache's bytes at the finish and their hidden rows are, byte for byte, the hidden_new[sel[j]] rows the
        rounds handed to the draft (Engine.hidden_log) — all from the verify kernels (tree attention, decode GEMMs), not the prefill
        kernels, in the class of the cohort they were decoded in (solo order for up to four requests with trees of <= 32 nodes, c8 order
        for five to eight).  A turn on it is the oracle's arithmetic within the bf16 bars, not bit-identical to prefilling the whole
        conversation again.  Costs [kv_max_pos, D] bf16 per engine that ever turns it on, and the prefix holds a full K/V copy of its
        rows.  The default False leaves the call, its captured graphs and its output tuple exactly as they were.
        return_logprobs=True appends, LAST in the output tuple, a float32 tensor [1, len(ids) - L] with one value per generated token:
        logprobs[i] = log_softmax(target_logits(ids[:L + i]))[ids[L + i]], computed on the device in fp32 from the bf16 logits the rounds
        (and the prefill, for i = 0) already produced.  It is always the TARGET model's own log-probability over its RAW logits —
        temperature 1, no top-k warper — at any temperature / top_k: never that of the warped distribution a token was sampled from, nor of
        the residual distribution a bonus token is drawn from after a rejection.  The array ends exactly where the ids end (EOS, budget,
        full KV cache).  The default False leaves the call, its captured graphs and its output tuple exactly as they were.
        top_logprobs = N (1..20, only with return_logprobs=True: ValueError otherwise, before any device work) appends, directly behind the
        logprobs entry (so before the return_prefix entry), a pair (top_ids int32 [1, len(ids) - L, N], top_logprobs float32 of the same
        shape): for every generated position the N tokens with the largest RAW target logits of the row that predicted it — the row of
        logprobs[i], the target's own distribution at temperature 1 without a warper, whatever the token was sampled from — and their
        log-probabilities x - m - log sum exp(x - m) in fp32.  Order: logit descending as floats (+0.0 and -0.0 are one value), ties by
        ascending token id; a vocabulary smaller than N pads with id -1, value -inf.  The selection is exact (bf16 logits, integer
        comparisons): the ids have no tolerance, and the entry is a deterministic function of the logits row.  The values come from the
        reduction that gives logprobs[i] (same arithmetic class; the kernel that writes both replaces the logprobs kernel of the round):
        logprobs is bit-identical with and without top_logprobs, and a listed token that is ids[L + i] carries exactly logprobs[i].  The
        default 0 leaves the call, its captured graphs and its output tuple exactly as they were.
        prefix = a PromptPrefix (prefill_prefix) that input_ids begins with: its K/V rows are copied into this model's cache (one
        vispec_kv_copy_rows launch) and only the new rows are prefilled, at past_len = prefix.rows; the vision front-end does not run and
        the vision kwargs are not read.  ValueError — with every cache untouched — when the ids do not begin with the prefix's, an image /
        video token follows the prefix, the prompt is no longer than the prefix, or the prefix belongs to other weights.  Arithmetic
        class: the prefix rows are the donor prefill's bytes; the new rows run the offset kernels (bit-identical per row) and library
        GEMMs at M = the new rows, which may sum in another fp32 order — the oracle's arithmetic within the bf16 bars, not guaranteed
        bit-identical to the full prefill, but bit-identical to prefill(x[:P]) followed by prefill(x[P:], past_len=P) on one cache.  The
        default None leaves the call exactly as it was.
        prefill_chunk_rows = C: the target prefill runs in pieces of at most C rows (TargetLM.prefill's chunk_rows: bounded activation
        workspace; the oracle's arithmetic within the bf16 bars, not guaranteed bit-identical to the unchunked prefill).  A named
        parameter: **kwargs go to the vision merge.  The default None leaves the call exactly as it was.
        temperature > 1e-5 selects the sampling path (utils.py:453-493) with device-side counter-based randomness (`seed`) and the
        processor list of utils.py:39-55: temperature, then TopK when top_k > 0.  0 < top_p < 1 raises: HF's TopPLogitsWarper fails
        on the 3-D tree logits evaluate_posterior passes it, so the reference cannot run that setting either."""
        if (input_ids is None) ^ (inputs_embeds is not None):  # :263-266 (sic: exactly the reference's condition)
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        if temperature > 1e-5 and 1e-8 <= top_p < 1.0:
            raise NotImplementedError("TopPLogitsWarper (utils.py:50-51) cannot run on the tree logits (HF scatters along dim 1: "
                                      "RuntimeError in the reference as well); use temperature / top_k")
        _check_top_logprobs(top_logprobs, return_logprobs)
        eng = self.engine
        max_length = max_length - self.spec_layer.total_tokens - 10  # :270
        self._start_request(input_ids, inputs_embeds, kwargs, seed=seed, max_new_tokens=max_new_tokens, prefix=prefix,
                            **_start_kw(temperature, top_k, is_llama3, prefill_chunk_rows, return_logprobs, return_prefix, top_logprobs))
        acceptance_len = []
        if return_decode_time:
            torch.cuda.synchronize()
            start_time = time.time()
        idx = 0
        st = eng.state()  # max_length <= 0 runs no round: the reference then returns the prompt as it is (:484,555)
        for idx in range(max_length):  # :484
            fa = -1 if forced_accept is None else int(forced_accept(idx))
            eng.verify_accept(fa)   # tree_decoding + evaluate_posterior + accept half of update_inference_inputs
            eng.draft_round()       # topK_genrate half of update_inference_inputs
            st = eng.state()        # the round's single host sync
            if return_acceptance_len:
                acceptance_len.append(int(st["accept_len"]))
            if _request_ended(st, max_new_tokens):  # the next tree not fitting a KV cache: the reference raises in KVCache.cat (kv_cache.py:40-58)
                _warn_kv_full(st, "specgenerate", f" (context {st['n_ctx']} of {eng.kv_max_pos} rows); the returned sequence is truncated")
                break
        res = _request_result(self, st, idx, acceptance_len, **_prefix_kw(return_prefix))
        toks, new_token = res[:2]
        outputs = (toks,)
        if log:
            outputs += (new_token, idx)
        if return_acceptance_len:
            outputs += (acceptance_len,)
        if return_decode_time:
            torch.cuda.synchronize()
            outputs += (time.time() - start_time,)
        if return_logprobs:
            outputs += (torch.from_numpy(_result_logprobs(self, toks.shape[1]))[None].to(eng.device),)
        if top_logprobs:
            outputs += (tuple(torch.from_numpy(x)[None].to(eng.device) for x in _result_top_logprobs(self, toks.shape[1], top_logprobs)),)
        if return_prefix:
            outputs += (res[-1],)
        return outputs[0] if len(outputs) == 1 else outputs

    # ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _start_baseline(self, input_ids, inputs_embeds, kwargs, max_new_tokens, return_logprobs=False, top_logprobs=0):
        """Prefill + first token of an AR request (gen_baseline_answer_coco_caption.py:60-110); -> the prompt ids on the device."""
        eng = self.engine
        eng.set_logprobs(return_logprobs)
        eng.set_top_logprobs(top_logprobs)
        eng.set_hidden_log(False)  # (the AR step shares target_accept with the rounds: its graphs carry a null log pointer)
        eng.set_sampling(0.0, 0)
        input_ids, emb, _, _, position_ids, rope_delta = self._embed_prompt(input_ids, inputs_embeds, kwargs)
        logits, _ = self.base_model.prefill(emb, position_ids=position_ids)
        first = self._first_token(logits)
        eng.begin_request(input_ids[0].cpu().numpy(), max_new_tokens)
        self._prompt_len = int(input_ids.shape[1])
        if return_logprobs:
            eng.token_logprob_row(logits[-1], first, self._prompt_len)
        if top_logprobs:
            eng.token_top_logprob_row(logits[-1], self._prompt_len)
        if rope_delta:
            eng.set_rope_delta(rope_delta)
        eng.set_next_token(first)
        return input_ids

    def _finish_baseline(self, input_ids, n_ctx, max_new_tokens):
        toks = self.engine.tokens(n_ctx).astype(np.int64)
        eos = self.base_model.cfg.eos_token_id
        gen = toks[input_ids.shape[1]:]
        cut = np.nonzero(gen == eos)[0]
        if cut.size:
            toks = toks[: input_ids.shape[1] + int(cut[0]) + 1]
        elif len(gen) > max_new_tokens + 1:
            toks = toks[: input_ids.shape[1] + max_new_tokens + 1]
        return torch.from_numpy(toks).to(self.engine.device)[None]

    @torch.no_grad()
    def baseline_generate(self, input_ids, inputs_embeds=None, max_new_tokens=512, max_steps=2048, return_logprobs=False, top_logprobs=0,
                          **kwargs):
        """Greedy AR with the same KV cache and kernels — evaluation/gen_baseline_answer_coco_caption.py:34-133.
        return_logprobs=True: -> (ids, logprobs float32 [1, len(ids) - L]) with specgenerate's meaning (the target's own log-softmax over its
        raw logits at each generated token), from the same kernel behind every AR step's accept.
        top_logprobs = N (1..20, only with return_logprobs=True: ValueError otherwise): -> (ids, logprobs, (top_ids int32 [1, len(ids) - L, N],
        top_logprobs float32 of the same shape)), specgenerate's top_logprobs entry, from the kernel that then replaces the logprobs one."""
        _check_top_logprobs(top_logprobs, return_logprobs)
        eng = self.engine
        input_ids = self._start_baseline(input_ids, inputs_embeds, kwargs, max_new_tokens, **_logprob_kw(return_logprobs), **_top_kw(top_logprobs))
        sync_every = 16
        for n in range(1, max_steps + 1):
            eng.ar_step()
            if n % sync_every == 0 or n == max_steps:
                st = eng.state()
                if st["done"]:
                    break
        st = eng.state()
        toks = self._finish_baseline(input_ids, st["n_ctx"], max_new_tokens)
        if return_logprobs:
            out = (toks, torch.from_numpy(_result_logprobs(self, toks.shape[1]))[None].to(eng.device))
            if top_logprobs:
                out += (tuple(torch.from_numpy(x)[None].to(eng.device) for x in _result_top_logprobs(self, toks.shape[1], top_logprobs)),)
            return out
        return toks


def _chunk_kw(name, chunk_rows):
    """The chunked-prefill option as keyword arguments: nothing at all for None, so a default call passes exactly what it always passed."""
    return {} if chunk_rows is None else {name: int(chunk_rows)}


def _logprob_kw(return_logprobs):
    """The log-probability option as keyword arguments: nothing at all for False, so a default call passes exactly what it always passed."""
    return {"return_logprobs": True} if return_logprobs else {}


def _top_kw(top_logprobs):
    """The top-N option as keyword arguments: nothing at all for 0, so a default call passes exactly what it always passed."""
    return {"top_logprobs": int(top_logprobs)} if top_logprobs else {}


def _check_top_logprobs(top_logprobs, return_logprobs):
    """The refusals of top_logprobs (one N, or a list with one N per request), raised before any device work: every N an integer in
    [0, 20], and N > 0 only together with return_logprobs."""
    for n in top_logprobs if isinstance(top_logprobs, (list, tuple)) else [top_logprobs]:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= L.TOP_LOGPROBS_MAX:
            raise ValueError(f"top_logprobs must be an integer in [0, {L.TOP_LOGPROBS_MAX}], not {n!r}")
        if n and not return_logprobs:
            raise ValueError("top_logprobs needs return_logprobs=True")


def _prefix_kw(return_prefix):
    """The returned-prefix option as keyword arguments: nothing at all for False, so a default call passes exactly what it always passed."""
    return {"return_prefix": True} if return_prefix else {}


def _start_kw(temperature, top_k, is_llama3, prefill_chunk_rows, return_logprobs, return_prefix=False, top_logprobs=0):
    """The generation keywords of a request start, built once per public call: what every _start_request of the call receives besides its
    own seed and budget (and, in a cohort or stream, its own top_logprobs: _start_requests' tops)."""
    return dict(temperature=temperature, top_k=top_k, is_llama3=is_llama3, **_chunk_kw("prefill_chunk_rows", prefill_chunk_rows),
                **_logprob_kw(return_logprobs), **_prefix_kw(return_prefix), **_top_kw(top_logprobs))


def _truncate_logprobs(log, n_prompt, n_tokens):
    """The generated tokens' entries of a position-indexed log-probability log for a result of n_tokens ids (prompt included): float32
    [n_tokens - n_prompt] — the log is cut exactly where the ids were cut (EOS, budget, full KV cache)."""
    log = np.asarray(log, dtype=np.float32)
    if not 0 <= n_prompt <= n_tokens <= log.shape[0]:
        raise ValueError(f"a log of {log.shape[0]} positions cannot serve {n_tokens} tokens behind a prompt of {n_prompt}")
    return log[n_prompt:n_tokens].copy()


def _result_logprobs(model, n_tokens):
    """The log-probabilities of the generated tokens of model's current request, for a result of n_tokens ids."""
    return _truncate_logprobs(model.engine.logprobs(n_tokens), model._prompt_len, n_tokens)


def _truncate_top_logprobs(ids_log, vals_log, n_prompt, n_tokens, n_top):
    """_truncate_logprobs for the two position-indexed top-N logs ([positions, >= n_top] each): -> (int32, float32) [n_tokens - n_prompt,
    n_top], cut exactly where the ids were cut and to the n_top slots the request asked for."""
    ids_log, vals_log = np.asarray(ids_log, dtype=np.int32), np.asarray(vals_log, dtype=np.float32)
    if ids_log.ndim != 2 or ids_log.shape != vals_log.shape or not 0 <= n_top <= ids_log.shape[1]:
        raise ValueError(f"top-N logs of shapes {ids_log.shape} / {vals_log.shape} cannot serve {n_top} entries per position")
    if not 0 <= n_prompt <= n_tokens <= ids_log.shape[0]:
        raise ValueError(f"logs of {ids_log.shape[0]} positions cannot serve {n_tokens} tokens behind a prompt of {n_prompt}")
    return ids_log[n_prompt:n_tokens, :n_top].copy(), vals_log[n_prompt:n_tokens, :n_top].copy()


def _result_top_logprobs(model, n_tokens, n_top):
    """The top-N entry of the generated tokens of model's current request, for a result of n_tokens ids; n_top = 0 (a member of a cohort
    whose partners asked): empty [n_gen, 0] arrays, the engine is not asked."""
    if not n_top:
        n_gen = n_tokens - model._prompt_len
        return np.zeros((n_gen, 0), np.int32), np.zeros((n_gen, 0), np.float32)
    return _truncate_top_logprobs(*model.engine.top_logprobs(n_tokens), model._prompt_len, n_tokens, n_top)


def _sync_tree_size(models):
    """Every request of a cohort round needs the leader's tree size (the C library checks it): a member built before
    `autotune_total_token()` / `spec_layer.total_tokens = ...` changed the leader's follows it here.  Trees of 33..64 nodes take two
    activation tiles per request, so such a cohort has at most four requests (vispec_ctx_create_member / vispec_set_total_token)."""
    lead = models[0]
    T = lead.engine.total_token
    if T > 32 and len(models) > 4:
        raise ValueError(f"a cohort of {len(models)} requests with trees of {T} nodes: trees of more than 32 nodes take two activation tiles per "
                         "request, at most four requests share a weight pass")
    for m in models[1:]:
        if m.engine.total_token != T:
            m.spec_layer.total_tokens = T - 1


def _request_ended(state, budget) -> bool:
    """The stop rule of every request loop: EOS in the generated ids (spec_model_ours.py:544, done bit 1), more new tokens than the budget
    (:546), or a next round that would not fit a KV cache (done bit 4)."""
    return bool(state["done"] & 5) or state["new_token"] > budget


def _warn_kv_full(state, subject, detail=""):
    """The RuntimeWarning of a request that a full KV cache ended (done bit 4) — not when EOS (bit 1) or its budget (bit 2) ended it as well."""
    if state["done"] & 4 and not state["done"] & 3:
        warnings.warn(f"{subject} stopped after {state['new_token']} new tokens: the next round would not fit a KV cache{detail}", RuntimeWarning)


def _result_prefix(model, toks):
    """The finished request of `model` as a PromptPrefix of every row of toks [1, n_ctx] (None + RuntimeWarning: conversation_prefix): the
    prompt rows its start kept, K/V rows [0, n_ctx) of its cache (one copy launch) and the generated rows of its hidden-row log — read in
    stream order, so before anything a later request start writes to this slot."""
    eng = model.engine
    return conversation_prefix(model._prompt_rows, toks, model._visual_token_ids(), eng.save_kv_rows, eng.hidden_log,
                               model.base_model.get_input_embeddings())


def _request_result(model, state, idx, accept_lens, return_logprobs=False, return_prefix=False, top_logprobs=None):
    """What a finished request returns: (ids [1, n_ctx] int64 on the device, new_token, idx, accept lengths); the host mirror of the KV length
    follows the device's.  return_logprobs: one more entry, the float32 numpy array of the generated tokens' target log-probabilities.
    top_logprobs = N (not None): one more entry behind it, the numpy pair (top ids int32, their log-probabilities float32) [n_gen, N].
    return_prefix: one more entry, LAST, the request as a PromptPrefix of its n_ctx rows (or None: _result_prefix)."""
    n_ctx = state["n_ctx"]
    model.current_length_data.fill_(n_ctx)
    toks = torch.from_numpy(model.engine.tokens(n_ctx).astype(np.int64)).to(model.engine.device)[None]
    out = (toks, state["new_token"], idx, accept_lens)
    if return_logprobs:
        out += (_result_logprobs(model, n_ctx),)
    if top_logprobs is not None:
        out += (_result_top_logprobs(model, n_ctx, top_logprobs),)
    if return_prefix:
        out += (_result_prefix(model, toks),)
    return out


def _check_cohort(models, requests=None):
    """models = [leader, members built on it...]; with `requests`, also 2..8 models and one request each."""
    if requests is not None and (not 2 <= len(models) <= 8 or len(requests) != len(models)):
        raise ValueError("a cohort is 2..8 models (leader, members...) and one request per model")
    for m in models[1:]:
        if m.engine.leader is not models[0].engine:
            raise ValueError("models[1:] must have been built with cohort_leader=models[0]")


def _per_request(value, n):
    """A list (one entry per request) as it is, a single value n times."""
    return list(value) if isinstance(value, (list, tuple)) else [value] * n


@torch.no_grad()
def baseline_generate_cohort(models, requests, max_new_tokens=512, max_steps=2048, stats=None):
    """The AR baseline (gen_baseline_answer_coco_caption.py:34-133) for two to eight requests in LOCKSTEP on one weight pass: what
    specgenerate_cohort is to specgenerate.  models / requests as there; max_new_tokens may be a list.  Returns one [1, L + new] id tensor
    per request — for cohorts of up to four the tokens `m.baseline_generate(ids, ...)` returns for that request alone (a request that
    reaches EOS or its budget freezes on the device while the others go on).  The speed-up bench.py prints divides a cohort's
    speculative tokens/s by THIS rate: like by like (speed.py:56-97).
    Arithmetic class (round 5): cohorts of up to FOUR requests keep every row bit-identical to a run of that request alone; cohorts of
    FIVE to EIGHT run the cohort-8 GEMM (csrc/gemm_c8.h: one fp32 accumulator chain per element) and 768-key attention splits — a request's
    tokens then do not depend on WHAT shares its weight pass (any cohort of 5..8, any tile), but they are the tokens of the c8 summation
    order, which may leave the solo run's at a near tie of the logits.  The class follows len(models) of the call: a deployment that wants
    one class for every request always calls with its full slot count."""
    _check_cohort(models, requests)
    lead, budgets = models[0], _per_request(max_new_tokens, len(models))
    _sync_tree_size(models)
    prompts = [m._start_baseline(ids, None, dict(kw), mx) for m, (ids, kw), mx in zip(models, requests, budgets)]
    members = [m.engine for m in models[1:]]
    if stats is not None:
        torch.cuda.current_stream().synchronize()
        t_loop = time.time()
    sync_every, steps = 16, 0
    for steps in range(1, max_steps + 1):
        lead.engine.cohort_ar_step(members)
        if steps % sync_every == 0 or steps == max_steps:
            states = lead.engine.cohort_states(members)
            if all(st["done"] for st in states):
                break
    states = lead.engine.cohort_states(members)
    if stats is not None:
        stats.update(decode_s=time.time() - t_loop, steps=steps)
    return [m._finish_baseline(p, st["n_ctx"], mx) for m, p, st, mx in zip(models, prompts, states, budgets)]


@torch.no_grad()
def _start_requests(models, requests, seeds, budgets, start_kw, prefixes=None, batch_prefill=False, forks=None, batches=None, tops=None):
    """Start one request per model: THE place that chooses the route of a request start, for cohorts, stream fills and refills alike.
    start_kw = _start_kw(...) of the public call; prefixes[t] = the PromptPrefix request t's prompt begins with, or None for a whole prompt.
    Without a prefix list, and without batch_prefill on two or more requests, every model runs its own _start_request, in slot order.
    Otherwise the start is staged.  Order: every refusal (PromptPrefix.check_request, check_prompt_fits of the whole prompt) for every
    request before any row of any cache is written; the first stage of _start_request per model; ONE Engine.load_kv_rows per distinct
    prefix into the caches of all requests that share it (its fan-out is appended to `forks`); the target prefill of the new rows — per
    request at past_len = P, or, under batch_prefill with two or more requests, one TargetLM.prefill_batch walk for all of them (their
    number is appended to `batches`; past_lens= whenever there is a prefix list); the last stage per model on cat(prefix hidden, new
    hidden) [L, D] (first token from each engine's own sample_row / seed; the draft prefill and the first tree stay per request).
    tops[t] = request t's own top_logprobs, in place of start_kw's one value for all (None: start_kw's)."""
    n = len(models)
    batched = batch_prefill and n >= 2
    if tops is not None:
        start_kw = {k: v for k, v in start_kw.items() if k != "top_logprobs"}
    tkw = [{} if tops is None else _top_kw(tp) for tp in (tops if tops is not None else [0] * n)]
    if prefixes is None and not batched:
        return [m._start_request(ids, None, dict(kw), seed=sd, max_new_tokens=mx, **start_kw, **tk)
                for m, (ids, kw), sd, mx, tk in zip(models, requests, seeds, budgets, tkw)]
    with_past = prefixes is not None  # (prefill_batch takes past_lens= for a prefix list only, a list of None included)
    prefixes = prefixes if with_past else [None] * n
    if len(prefixes) != n or len(requests) != n:
        raise ValueError("one request and one prefix entry (a PromptPrefix or None) per model")
    prep_kw = dict(start_kw)
    ck = _chunk_kw("chunk_rows", prep_kw.pop("prefill_chunk_rows", None))
    for m, (ids, kw), pf in zip(models, requests, prefixes):
        Ln = int(ids.shape[1]) if pf is None else pf.check_request(ids, m.base_model.w, m._visual_token_ids())
        m.engine.check_prompt_fits(Ln)
    preps = [m._start_prepare(ids, None, dict(kw), seed=sd, max_new_tokens=mx, prefix=pf, **prep_kw, **tk)
             for m, (ids, kw), pf, sd, mx, tk in zip(models, requests, prefixes, seeds, budgets, tkw)]
    groups = {}
    for t, pf in enumerate(prefixes):
        if pf is not None:
            groups.setdefault(id(pf), (pf, []))[1].append(t)
    for pf, ts in groups.values():
        models[ts[0]].engine.load_kv_rows(pf.store, [models[t].engine for t in ts])
        if forks is not None:
            forks.append(len(ts))
    news = [pr.emb[pr.past:] for pr in preps]
    if batched:
        res = models[0].base_model.prefill_batch([m.engine for m in models], news, [pr.position_ids for pr in preps],
                                                  **({"past_lens": [pr.past for pr in preps]} if with_past else {}), **ck)
        if batches is not None:
            batches.append(n)
    else:
        res = [m.base_model.prefill(x, position_ids=pr.position_ids, **({"past_len": pr.past} if pr.past else {}), **ck)
               for m, pr, x in zip(models, preps, news)]
    return [m._start_finish(pr, logits, hidden if not pr.past else torch.cat([pr.prefix.hidden, hidden], dim=0))
            for m, pr, (logits, hidden) in zip(models, preps, res)]


@torch.no_grad()
def specgenerate_cohort(models, requests, temperature=0.0, top_k=0.0, max_new_tokens=512, max_length=2048, is_llama3=False, seeds=None,
                        forced_accept=None, stats=None, batch_prefill=False, prefill_chunk_rows=None, prefix=None, return_logprobs=False,
                        return_prefix=False, top_logprobs=0):
    """Two to eight independent requests through SpecModel.specgenerate's loop (spec_model_ours.py:247-582) in LOCKSTEP on one weight pass.

    models   = [leader, member, ...]  (members built with cohort_leader=leader: one vispec_ctx, KV cache, tree and round state each)
    requests = [(input_ids [1,L], specgenerate kwargs), ...] one per model; max_new_tokens may be a list (one budget per request)
    Returns one (input_ids [1, L+new], new_token, idx, acceptance_len) tuple per request — for cohorts of up to four exactly what
    `m.specgenerate(ids, log=True, return_acceptance_len=True, ...)` returns for that request alone, token for token: the prefills run
    per request, every decode round launches each GEMM once on all requests' rows (Engine.cohort_round), and a request that finishes
    first is frozen on the device while the others complete.
    Arithmetic class (round 5): cohorts of up to FOUR requests keep every row bit-identical to a run of that request alone; cohorts of
    FIVE to EIGHT run the cohort-8 GEMM (csrc/gemm_c8.h: one fp32 accumulator chain per element) and 768-key attention splits — a request's
    tokens then do not depend on WHAT shares its weight pass (any cohort of 5..8, any tile), but they are the tokens of the c8 summation
    order, which may leave the solo run's at a near tie of the logits.  The class follows len(models) of the call: a deployment that wants
    one class for every request always calls with its full slot count.  `stats` (a dict, optional) receives the wall time of the round loop
    (`decode_s`, bracketed by synchronisations like specgenerate's return_decode_time) and the number of lockstep rounds (`rounds`).
    batch_prefill=True starts the n requests through ONE target prefill (TargetLM.prefill_batch: the prompts' rows concatenated, one walk over
    the weights, varlen rotary + attention kernels) instead of n (`stats["prefill_batches"]`: [n]).  Arithmetic class of that start: the row-wise kernels and both varlen kernels
    are bit-identical to the per-request path; the library GEMMs at M = sum L may pick another solution and with it another fp32 summation
    order, so a request's prefill is the oracle's arithmetic within the bf16 bars of the single-request comparisons, not guaranteed
    bit-identical to its solo prefill.  The default False leaves the call exactly as it was.
    prefill_chunk_rows = C: every target prefill of the start runs in pieces of at most C rows — per request (TargetLM.prefill's chunk_rows)
    or, under batch_prefill, over the concatenated row stream of the batch (prefill_batch's chunk_rows).  Same arithmetic class as
    batch_prefill: within the oracle's bf16 bars, not guaranteed bit-identical.  The default None leaves the call exactly as it was.
    prefix = one PromptPrefix (SpecModel.prefill_prefix) for every request, or a list with one entry or None per request: a request on a
    prefix starts as specgenerate(prefix=) does.  The requests that share one PromptPrefix get its K/V rows through ONE copy launch
    (`stats["prefix_forks"]`: the fan-outs, in order); under batch_prefill their new rows — and the whole prompts of requests without a
    prefix — go through one walk (prefill_batch's past_lens).  Every refusal of any request is raised before any cache row of any
    request is written.  Arithmetic class: prefix rows are the donor prefill's bytes; new rows run the offset kernels (bit-identical per
    row) and library GEMMs at M = the new rows (or their sum), which may sum in another fp32 order — the oracle's arithmetic within the
    bf16 bars, not guaranteed bit-identical to the full prefill; per request it IS bit-identical to prefill(x[:P]) followed by
    prefill(x[P:], past_len=P) on one cache.  The default None leaves the call exactly as it was.
    return_logprobs=True: every request's tuple gains a fifth entry, the float32 numpy array [len(ids) - L] of specgenerate's
    return_logprobs (the target's own log-softmax over its raw logits at each generated token), a deterministic function of that request's
    logits: a request that finished and froze keeps its log untouched while the others go on.  The default False leaves the call exactly
    as it was.
    top_logprobs = N, or a list with one N per request (0..20, N > 0 only with return_logprobs=True: ValueError otherwise, before any
    device work): when any N > 0, every request's tuple gains, directly behind the logprobs entry, the numpy pair (top_ids int32,
    top_logprobs float32) [len(ids) - L, N of that request] of specgenerate's top_logprobs — like the logprobs entry a deterministic
    function of that request's logits, kept untouched by a request that finished and froze.  Requests with different N share the
    round's one launch.  The default 0 leaves the call exactly as it was.
    return_prefix=True: every request's tuple gains one more entry, LAST, specgenerate's return_prefix — that request as a PromptPrefix of
    its own n_ctx rows, or None.  A request that finished and froze keeps its cache rows and its hidden-row log untouched while the others
    go on.  Arithmetic class of the generated rows: that of this cohort (up to four requests: bit-identical to the request's solo run; five
    to eight: the c8 class, independent of what shares the weight pass).  The default False leaves the call exactly as it was."""
    _check_cohort(models, requests)
    _check_top_logprobs(top_logprobs, return_logprobs)
    n, lead = len(models), models[0]
    tops = _per_request(top_logprobs, n)
    if len(tops) != n:
        raise ValueError("one top_logprobs entry per request")
    seeds = seeds or [0] * n
    _sync_tree_size(models)
    budgets = _per_request(max_new_tokens, n)
    prefix_forks, prefill_batches = [], []
    _start_requests(models, requests, seeds, budgets, _start_kw(temperature, top_k, is_llama3, prefill_chunk_rows, return_logprobs, return_prefix),
                    prefixes=None if prefix is None else _per_request(prefix, n), batch_prefill=batch_prefill, forks=prefix_forks,
                    batches=prefill_batches, **({"tops": tops} if any(tops) else {}))
    rounds_cap = max_length - lead.spec_layer.total_tokens - 10  # :270
    alive = [True] * n
    final = [m.engine.state() for m in models]
    idxs, accs = [0] * n, [[] for _ in range(n)]
    member_engines = [m.engine for m in models[1:]]
    if stats is not None:
        torch.cuda.current_stream().synchronize()
        t_loop = time.time()
    for idx in range(rounds_cap):
        fa = -1 if forced_accept is None else int(forced_accept(idx))
        lead.engine.cohort_round(member_engines, fa)
        states = lead.engine.cohort_states(member_engines)  # the round's ONE host synchronisation
        for t, m in enumerate(models):
            if not alive[t]:
                continue
            st = states[t]
            final[t], idxs[t] = st, idx
            accs[t].append(int(st["accept_len"]))
            if _request_ended(st, budgets[t]):
                _warn_kv_full(st, f"cohort request {t}")
                alive[t] = False
        if not any(alive):
            break
    if stats is not None:
        torch.cuda.current_stream().synchronize()
        stats.update(decode_s=time.time() - t_loop, rounds=idx + 1)
        if batch_prefill:
            stats["prefill_batches"] = prefill_batches
        if prefix is not None:
            stats["prefix_forks"] = prefix_forks
    return [_request_result(m, final[t], idxs[t], accs[t], **_logprob_kw(return_logprobs), **_prefix_kw(return_prefix),
                            **({"top_logprobs": tops[t]} if any(tops) else {})) for t, m in enumerate(models)]


def specgenerate_stream(models, requests, temperature=0.0, top_k=0.0, max_new_tokens=512, max_length=2048, is_llama3=False, seeds=None,
                        stats=None, batch_prefill=False, prefill_chunk_rows=None, prefix=None, return_logprobs=False, return_prefix=False,
                        top_logprobs=0):
    """Any number of independent requests through the request SLOTS of one cohort (continuous batching): `models` = [leader, member, ...]
    as for specgenerate_cohort, `requests` = [(input_ids [1,L], specgenerate kwargs), ...] in arrival order.  The first len(models)
    requests start together; every lockstep round serves all slots on one weight pass, and the moment a request finishes (EOS, its
    token budget, a full KV cache) its slot takes the next request of the queue — prefill, first token and draft prefill of that request
    on the same stream, then it simply joins the following rounds (the other slots' state is device-resident and waits).  A cohort run
    request by request (specgenerate_cohort) executes max(rounds of its requests) lockstep rounds; the stream executes ≈ mean(rounds).
    Every request keeps the reference's batch-1 semantics: with up to four slots it returns exactly the (input_ids, new_token, idx,
    acceptance_len) tuple of `m.specgenerate(ids, log=True, return_acceptance_len=True, ...)` run alone (spec_model_ours.py:247-582), in
    request order; with five to eight slots the tuple of the c8 arithmetic class (see specgenerate_cohort) — independent of what shares the
    slots.  When len(requests) <= len(models) the call falls back to plain cohorts of len(group) requests, so the class then follows the
    number of requests that arrive together (4 or fewer: solo arithmetic; 5 or more: c8).
    `stats` (dict, optional): `rounds` = lockstep rounds executed, `request_rounds` = rounds summed over the requests.
    batch_prefill=True: the initial fill of all slots is ONE batched target prefill (specgenerate_cohort's batch_prefill: same arithmetic
    class — within the oracle's bf16 bars, not guaranteed bit-identical to a solo prefill), and refills whose slots are harvested in the same
    pass over the states start together as one batch; a single refill goes through the unchanged per-request path.  `stats` then also
    receives `prefill_batches`: the sizes of the batched starts, in order.  The default False leaves the call exactly as it was.
    prefill_chunk_rows = C: every target prefill of the call — initial fills and refills, batched or not — runs in pieces of at most C rows
    (specgenerate_cohort's prefill_chunk_rows).  The default None leaves the call exactly as it was.
    prefix = one PromptPrefix for every request, or a list with one entry or None per request, in arrival order (specgenerate_cohort's
    prefix: same refusals, same arithmetic class).  Initial fills and refills take the same route: the requests that start together and
    share a PromptPrefix get its rows through one copy launch, and `stats` receives `prefix_forks`, the fan-outs of those launches in
    order (their sum = the requests that started on a prefix).  The default None leaves the call exactly as it was.
    return_logprobs=True: every request's tuple gains the fifth entry of specgenerate_cohort's return_logprobs; a slot's log is cleared when
    its next request begins, so a re-used slot returns its own request's values only.  The default False leaves the call exactly as it was.
    top_logprobs = N, or a list with one N per request in arrival order (specgenerate_cohort's top_logprobs: same refusals): when any
    N > 0, every request's tuple gains that entry directly behind the logprobs entry; a slot's top-N logs are cleared with its
    log-probability log when its next request begins.  The default 0 leaves the call exactly as it was.
    return_prefix=True: every request's tuple gains one more entry, LAST, specgenerate_cohort's return_prefix; it is taken when the request
    finishes, in stream order before the slot's next request writes the cache.  The default False leaves the call exactly as it was."""
    _check_top_logprobs(top_logprobs, return_logprobs)
    start_kw = _start_kw(temperature, top_k, is_llama3, prefill_chunk_rows, return_logprobs, return_prefix)
    lk = {**_logprob_kw(return_logprobs), **_prefix_kw(return_prefix)}
    n, R = len(models), len(requests)
    tops = _per_request(top_logprobs, R)
    if len(tops) != R:
        raise ValueError("one top_logprobs entry per request")
    with_top = any(tops)  # every tuple then carries the entry (a request with N = 0: [n_gen, 0] arrays)
    prefixes = None if prefix is None else _per_request(prefix, R)
    if prefixes is not None and len(prefixes) != R:
        raise ValueError("one prefix entry (a PromptPrefix or None) per request")
    prefix_forks, prefill_batches = [], []
    seeds = list(seeds) if seeds is not None else [0] * R
    budgets = _per_request(max_new_tokens, R)
    if len(seeds) != R or len(budgets) != R:
        raise ValueError("one seed and one token budget per request")
    lead = models[0]
    rounds_cap = max_length - lead.spec_layer.total_tokens - 10  # :270
    if R <= n or n < 2 or rounds_cap < 1:  # nothing to refill: the plain cohort (or single-request) loops
        outs, st_all = [], dict(rounds=0, request_rounds=0)
        for lo in range(0, R, max(n, 1)):
            grp = list(range(lo, min(R, lo + max(n, 1))))
            if len(grp) >= 2 and n >= 2:
                st = {}
                got = specgenerate_cohort(models[:len(grp)], [requests[i] for i in grp], max_new_tokens=[budgets[i] for i in grp],
                                          max_length=max_length, seeds=[seeds[i] for i in grp], stats=st, batch_prefill=batch_prefill,
                                          prefix=None if prefixes is None else [prefixes[i] for i in grp],
                                          **({"top_logprobs": [tops[i] for i in grp]} if with_top else {}), **start_kw)
                if with_top and not any(tops[i] for i in grp):  # (a group that asked for none: the entry all the same)
                    got = [g[:5] + (_result_top_logprobs(m, g[0].shape[1], 0),) + g[5:] for g, m in zip(got, models)]
                st_all["rounds"] += st["rounds"]
                prefix_forks += st.get("prefix_forks", [])
                prefill_batches += st.get("prefill_batches", [])
            else:
                got = []
                for i in grp:
                    ids, kw = requests[i]
                    pf = None if prefixes is None else prefixes[i]
                    one = lead.specgenerate(ids, max_new_tokens=budgets[i], max_length=max_length, log=True, return_acceptance_len=True,
                                            seed=seeds[i], prefix=pf, **start_kw, **_top_kw(tops[i]), **kw)
                    k = 4 + bool(return_logprobs) + bool(tops[i])  # the entries behind the first four that arrive as device tensors
                    top = (tuple(x[0].cpu().numpy() for x in one[k - 1]),) if tops[i] else \
                        ((_result_top_logprobs(lead, one[0].shape[1], 0),) if with_top else ())
                    got.append(one[:4] + ((one[4][0].cpu().numpy(),) if return_logprobs else ()) + top + one[k:])
                    prefix_forks += [1] if pf is not None else []
                st_all["rounds"] += sum(g[2] + 1 for g in got)
            st_all["request_rounds"] += sum(g[2] + 1 for g in got)
            outs += got
        if stats is not None:
            stats.update(st_all)
            if prefill_batches:
                stats["prefill_batches"] = prefill_batches
            if prefixes is not None:
                stats["prefix_forks"] = prefix_forks
        return outs
    _check_cohort(models)
    _sync_tree_size(models)
    member_engines = [m.engine for m in models[1:]]
    outs = [None] * R
    slot = [None] * n  # request index a slot is working on
    rnd, accs = [0] * n, [[] for _ in range(n)]
    nxt = 0

    def start(ts):  # the next len(ts) requests of the queue on slots ts
        nonlocal nxt
        idx = list(range(nxt, nxt + len(ts)))
        nxt += len(ts)
        _start_requests([models[t] for t in ts], [requests[i] for i in idx], [seeds[i] for i in idx], [budgets[i] for i in idx], start_kw,
                        prefixes=None if prefixes is None else [prefixes[i] for i in idx], batch_prefill=batch_prefill, forks=prefix_forks,
                        batches=prefill_batches, **({"tops": [tops[i] for i in idx]} if with_top else {}))
        for t, i in zip(ts, idx):
            slot[t], rnd[t], accs[t] = i, 0, []

    # One round of LOOKAHEAD (round 4; VISPEC_STREAM_LOOKAHEAD=0 restores the lockstep loop): round k + 1 is launched before round k's states are
    # read, so the stream never waits for the host between rounds (state snapshots travel through two pinned slots in stream order:
    # Engine.cohort_states_enqueue / _wait).  A request that finished in round k is frozen on the device (EOS, budget and cache limits are
    # decided there: tree_kernels.h), so the round already in flight leaves it untouched; its slot rides along idle for that one round and the
    # refill joins from the round after.  valid_from[t] = the first launched round whose snapshot describes slot t's CURRENT request.
    lookahead = os.environ.get("VISPEC_STREAM_LOOKAHEAD", "1") != "0"
    valid_from = [0] * n
    k_enq = k_done = 0

    def launch():
        nonlocal k_enq
        lead.engine.cohort_round(member_engines, -1)
        lead.engine.cohort_states_enqueue(member_engines, k_enq & 1)
        k_enq += 1

    start(list(range(n)))
    lockstep = request_rounds = 0
    launch()
    while any(i is not None for i in slot):
        if lookahead and k_enq - k_done < 2:
            launch()
        states = lead.engine.cohort_states_wait(member_engines, k_done & 1)  # waits for that round's snapshot only
        k, k_done = k_done, k_done + 1
        lockstep += 1
        for t in range(n):
            if slot[t] is None or k < valid_from[t]:
                continue  # an idle slot (the queue is empty / its new request joins a later round): its frozen rows ride along
            st = states[t]
            rnd[t] += 1
            request_rounds += 1
            accs[t].append(int(st["accept_len"]))
            if _request_ended(st, budgets[slot[t]]) or rnd[t] >= rounds_cap:  # (the cap, :484, is the host's alone)
                _warn_kv_full(st, f"request {slot[t]}")
                outs[slot[t]] = _request_result(models[t], st, rnd[t] - 1, accs[t], **lk, **({"top_logprobs": tops[slot[t]]} if with_top else {}))
                slot[t] = None
        free = [t for t in range(n) if slot[t] is None][:R - nxt]  # the slots this pass refills, in slot order
        if free:
            start(free)
        for t in free:
            valid_from[t] = k_enq  # it is part of the rounds launched from now on
        if k_enq == k_done and any(i is not None for i in slot):
            launch()
    # the round launched ahead of the last snapshot (lookahead) is still in flight: wait for its snapshot too, so that nothing of this call is
    # running on the stream when it returns.  (A request ended by the HOST-only rule `rnd >= rounds_cap` (:484) is not frozen on the device: the
    # round in flight may advance it once more — harmless, its tokens were taken up to the snapshot's n_ctx, which that round does not
    # rewrite, and the slot's next _start_request resets the device state in stream order.)
    while k_done < k_enq:
        lead.engine.cohort_states_wait(member_engines, k_done & 1)
        k_done += 1
    if stats is not None:
        stats.update(rounds=lockstep, request_rounds=request_rounds)
        if batch_prefill:
            stats["prefill_batches"] = prefill_batches
        if prefixes is not None:
            stats["prefix_forks"] = prefix_forks
    return outs
