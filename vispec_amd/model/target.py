"""Target VLM wrapper (`base_model` of the reference's SpecModel).

What lives where (BASELINE.json north_star): vision tower / projector and the PREFILL forward stay on PyTorch-ROCm
(plain torch ops below: hipBLASLt GEMMs + SDPA), writing K/V straight into the engine's KV buffer; every forward
that happens inside the draft-and-verify loop (tree verify, AR decode step) runs as HIP kernels via the Engine.
This module owns its Llama decode path instead of subclassing HF (transformers 5.x no longer lets
`language_model` be swapped — SURVEY.md §7.2); reference semantics followed: modeling_llama_kv.py:527-653
(attention), :104-133 (RMSNorm), :927-1080 (model), lm_head + .float() (:1190-1197)."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

import ctypes as C
import os

from .. import lib as L
from ..engine import Engine, TargetConfig, TargetWeights
from ..prefill_plan import plan_prefill_pieces


_p = lambda t: C.c_void_p(t.data_ptr())
_gemm_lock = __import__("threading").Lock()
_gemm_state = {"mode": None}
# Recorded GEMM solutions of the prefill shapes (torch's TunableOp CSV: one line per (transposition, M, N, K, leading dims) with the library
# solution that won an offline tuning run, preceded by validator lines: PyTorch / ROCm / hipBLASLt / rocBLAS versions and the GPU arch).
# Written by tools/tune_prefill.py on an MI355X; TunableOp ignores the file when a validator does not match the running stack.
PREFILL_GEMM_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tunable", "prefill_gemms_gfx950.csv")


def prefill_gemm_selection():
    """Which library kernel runs the prefill's GEMMs is decided HERE, once per process and identically on every rank and lane — not by a
    timing taken at the first prompt (rounds 2-3 padded the gate|up weight with zero rows until hipBLASLt's heuristic left a slow
    stream-K kernel: a second copy of every gate|up matrix, chosen by whichever lane got there first, gone with the next ROCm).

      VISPEC_PREFILL_GEMMS=recorded (default)  torch's TunableOp in LOOKUP-ONLY mode over the committed table PREFILL_GEMM_FILE (or
                                               $VISPEC_PREFILL_GEMM_FILE): a shape in the table runs the recorded rocBLAS / hipBLASLt solution,
                                               any other shape — and every shape when the table's validators do not match this PyTorch /
                                               ROCm / GPU — runs the libraries' own default.  Deterministic; nothing is timed at run time.
                                               (TunableOp is a process-wide switch of torch: in this mode every torch GEMM of the process does
                                               one table lookup; shapes outside the table are untouched.  A host application that minds sets
                                               VISPEC_PREFILL_GEMMS=default.)
      VISPEC_PREFILL_GEMMS=default             TunableOp stays off.
      VISPEC_PREFILL_GEMMS=tune                tuning on, results written to the file (tools/tune_prefill.py: offline, one process, idle GPU)."""
    if _gemm_state["mode"] is not None:
        return _gemm_state["mode"]
    with _gemm_lock:
        if _gemm_state["mode"] is not None:
            return _gemm_state["mode"]
        mode = os.environ.get("VISPEC_PREFILL_GEMMS", "recorded")
        path = os.environ.get("VISPEC_PREFILL_GEMM_FILE", PREFILL_GEMM_FILE)
        if mode not in ("recorded", "default", "tune"):
            raise ValueError("VISPEC_PREFILL_GEMMS must be recorded, default or tune")
        if mode != "default":
            try:
                import torch.cuda.tunable as tn
                if mode == "tune":
                    tn.enable(True)
                    tn.tuning_enable(True)
                    tn.set_filename(path)
                elif os.path.exists(path):
                    tn.enable(True)
                    tn.tuning_enable(False)
                    tn.set_filename(path)
                    if not tn.read_file(path):  # validators of another stack: the libraries' defaults, and say so once
                        tn.enable(False)
                        # (no warning at import time of a host application — round-4 advice; the mode string says it, bench.py prints it in
                        #  its line's config and VISPEC_PREFILL_GEMMS_STRICT=1 makes it an error)
                        mode = "default (the recorded table does not match this PyTorch / ROCm / GPU: re-run tools/tune_prefill.py)"
                        if os.environ.get("VISPEC_PREFILL_GEMMS_STRICT") == "1":
                            raise RuntimeError(f"{path}: recorded prefill GEMM solutions do not match this PyTorch / ROCm / GPU (VISPEC_PREFILL_GEMMS_STRICT=1)")
                else:
                    mode = "default (no recorded table)"
            except RuntimeError as e:
                if "VISPEC_PREFILL_GEMMS_STRICT" in str(e):
                    raise
                mode = f"default (TunableOp unavailable: {type(e).__name__})"
            except Exception as e:  # TunableOp is an optimisation: never lose a run to it
                mode = f"default (TunableOp unavailable: {type(e).__name__})"
        _gemm_state["mode"] = mode
        return mode


_sdpa_lock = __import__("threading").Lock()
_sdpa_ready = set()


def _sdpa(q, k, v, gqa):
    """Causal SDPA for the prefill.  PyTorch-ROCm's flash backend initialises its per-device kernel table lazily and not
    thread-safely (concurrent first calls from several lanes were seen to fail with "Accelerated SDPA only supports ..."), so the
    first call per device is serialised; if the accelerated backend is unavailable the math backend is used (still PyTorch)."""
    dev = q.device.index
    if dev not in _sdpa_ready:
        with _sdpa_lock:
            out = _sdpa_try(q, k, v, gqa)
            torch.cuda.synchronize(q.device)
            _sdpa_ready.add(dev)
            return out
    return _sdpa_try(q, k, v, gqa)


def _sdpa_try(q, k, v, gqa):
    try:
        return F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=gqa)
    except RuntimeError as e:
        import warnings
        from torch.nn.attention import SDPBackend, sdpa_kernel
        warnings.warn(f"accelerated SDPA unavailable ({str(e)[:120]}); prefill attention falls back to the math backend")
        with sdpa_kernel([SDPBackend.MATH]):
            return F.scaled_dot_product_attention(q, k, v, is_causal=True, enable_gqa=gqa)


def scaled_linear(x, w, b=None, scale=None, q8=None):
    """nn.Linear on a row-major weight.  scale != None: `w` holds fp8 (e4m3) codes as bf16 and `scale` their per-output-channel factors —
    bf16( (x . w^T) * scale + b ) on an fp32 accumulator, the rounding points of the library's W8A16 GEMMs (kernels.h epilogues).
    q8 != None (W8A8, target_weight_dtype "fp8a8"): the same codes as a row-major uint8 tensor; the activations are quantised row by row
    (vispec_quant_rows_e4m3: the decode path's kernel) and the product runs on the fp8 MFMA through the library's fp8 x fp8 GEMM
    (torch._scaled_mm, row-wise scales): bf16( (q_x . q_w^T) * sx[m] * scale[n] + b ) — oracle: Ops.linear(a8=True)."""
    if scale is None:
        return F.linear(x, w, b)
    x2 = x.reshape(-1, x.shape[-1])
    if q8 is not None:
        lib = L.load()
        M, K = x2.shape
        x2 = x2.contiguous()
        qx = torch.empty(M, K, dtype=torch.uint8, device=x2.device)
        sx = torch.empty(M, 1, dtype=torch.float32, device=x2.device)
        L.check(lib.vispec_quant_rows_e4m3(None, C.c_void_p(torch.cuda.current_stream(x2.device).cuda_stream), C.c_void_p(x2.data_ptr()), K,
                                           C.c_void_p(qx.data_ptr()), K, C.c_void_p(sx.data_ptr()), M, K))
        out = torch._scaled_mm(qx.view(torch.float8_e4m3fn), q8.view(torch.float8_e4m3fn).t(), scale_a=sx, scale_b=scale.reshape(1, -1).float(),
                               bias=None if b is None else b.to(torch.bfloat16), out_dtype=torch.bfloat16)
        return out.reshape(*x.shape[:-1], q8.shape[0])
    acc = torch.mm(x2, w.t(), out_dtype=torch.float32)
    N = w.shape[0]
    if acc.is_cuda and N % 8 == 0 and x.dtype == torch.bfloat16:  # scale, bias and the bf16 rounding in one pass (vispec_scale_bias_cast)
        lib = L.load()
        out = torch.empty(acc.shape[0], N, dtype=torch.bfloat16, device=acc.device)
        sc = scale.reshape(-1).float().contiguous()
        bb = None if b is None else b.to(torch.bfloat16).contiguous()
        L.check(lib.vispec_scale_bias_cast(None, C.c_void_p(torch.cuda.current_stream(acc.device).cuda_stream), C.c_void_p(acc.data_ptr()), N,
                                           C.c_void_p(sc.data_ptr()), None if bb is None else C.c_void_p(bb.data_ptr()), C.c_void_p(out.data_ptr()), N,
                                           acc.shape[0], N))
        return out.reshape(*x.shape[:-1], N)
    y = acc * scale
    if b is not None:
        y = y + b.float()
    return y.to(x.dtype).reshape(*x.shape[:-1], N)


class _Head:
    """stand-in for nn.Linear lm_head: the reference passes `base_model.lm_head` into topK_genrate (utils.py:300)."""

    def __init__(self, weights):
        self._w = weights  # the Engine may quantise the head in place after this object exists: read weight / scale at call time

    @property
    def weight(self):
        return self._w.lm_head

    def __call__(self, x):
        return scaled_linear(x, self._w.lm_head, None, getattr(self._w, "lm_head_scale", None))


class SyntheticVision:
    """Vision front-end used when no vision tower weights exist on the box (no network): deterministic features
    with the statistics of SURVEY.md §8(d) — N(0,1)*0.05 — one row per image placeholder token."""

    def __init__(self, hidden_size: int, std: float = 0.05):
        self.hidden_size, self.std = hidden_size, std

    def features(self, n_tokens: int, seed: int, device, dtype):
        g = torch.Generator(device="cpu").manual_seed(1000 + int(seed))
        return (torch.randn(n_tokens, self.hidden_size, generator=g) * self.std).to(device=device, dtype=dtype)


class TargetLM:
    """`base_model`: config + weights + PyTorch prefill + handles the reference code touches."""

    def __init__(self, cfg: TargetConfig, weights: TargetWeights, vision=None):
        self.cfg, self.w = cfg, weights
        self.device, self.dtype = weights.device, torch.bfloat16
        self.config = SimpleNamespace(
            architectures=list(cfg.architectures), num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.num_heads,
            num_key_value_heads=cfg.num_kv_heads, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
            vocab_size=cfg.vocab_size, max_position_embeddings=cfg.max_position_embeddings, rms_norm_eps=cfg.rms_norm_eps,
            image_token_index=cfg.image_token_index, image_token_id=cfg.image_token_index, video_token_id=cfg.video_token_id,
            eos_token_id=cfg.eos_token_id,
            vision_feature_layer=-2, vision_feature_select_strategy="default")
        self.lm_head = _Head(weights)
        self.vision = vision or SyntheticVision(cfg.hidden_size)
        self.engine: Optional[Engine] = None  # attached by SpecModel
        self.tree_mask = None  # reference stores it on base_model.model (spec_model_ours.py:486-489); kept for API parity
        self.model = self  # `base_model.model.tree_mask = ...` (utils.py:334)

    # ---- handles used by spec_model_ours.py:339-376 -------------------------------------------------
    def get_input_embeddings(self):
        return lambda ids: F.embedding(ids, self.w.embed)

    def get_image_features(self, pixel_values, image_sizes=None, image_grid_thw=None, **kw):
        """-> packed image features [n_image_tokens, D] in prompt order.
        A ready [N, D] tensor is passed through (bench / tests keep the request's features resident in HBM); with a real
        checkpoint (`self.vision` is an HFVisionFrontEnd) `pixel_values` are the processor's pixels and the HF vision tower +
        projector (+ anyres packing) run on PyTorch-ROCm, as in the reference (spec_model_ours.py:341-356); the synthetic
        front-end takes (n_image_tokens, seed)."""
        if (torch.is_tensor(pixel_values) and pixel_values.dim() == 2 and pixel_values.shape[-1] == self.cfg.hidden_size
                and not hasattr(self.vision, "tower")):
            return pixel_values.to(self.device, self.dtype)
        if hasattr(self.vision, "tower"):
            kw = {k: v for k, v in kw.items() if k in ("vision_feature_layer", "vision_feature_select_strategy") and v is not None}
            return self.vision.features(pixel_values, image_sizes=image_sizes, image_grid_thw=image_grid_thw, **kw).to(self.device, self.dtype)
        n, seed = pixel_values
        return self.vision.features(int(n), int(seed), self.device, self.dtype)

    def pack_image_features(self, image_features, image_sizes=None, **kw):
        return image_features, torch.tensor([image_features.shape[0]])

    image_newline = None

    # ---- PyTorch prefill -----------------------------------------------------------------------------
    def mrope_cos_sin(self, pos3: torch.Tensor):
        """cos/sin [L, hd] for 3-component positions [3, L] (modeling_qwen2_5_vl_kv.py rotary + apply_multimodal_rotary_pos_emb):
        fp32 angles per component, chunk i of sizes mrope_section*2 takes component i % 3, then cast to the model dtype."""
        c = self.cfg
        hd = c.head_dim
        inv_freq = 1.0 / (c.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))
        freqs = pos3.float().cpu()[:, :, None] * inv_freq[None, None, :]
        emb = torch.cat((freqs, freqs), dim=-1)
        cos3, sin3 = emb.cos(), emb.sin()
        sec = list(c.mrope_section) * 2
        cos = torch.cat([m[i % 3] for i, m in enumerate(cos3.split(sec, dim=-1))], dim=-1)
        sin = torch.cat([m[i % 3] for i, m in enumerate(sin3.split(sec, dim=-1))], dim=-1)
        return cos.to(self.dtype).to(self.device), sin.to(self.dtype).to(self.device)

    @torch.no_grad()
    def prefill(self, inputs_embeds: torch.Tensor, all_logits: bool = False, position_ids: Optional[torch.Tensor] = None,
                chunk_rows: Optional[int] = None, past_len: int = 0):
        """inputs_embeds [L, D] bf16 -> (logits fp32 [L or 1, V], hidden [L, D] post-final-norm); K/V rows [0, L)
        of every layer are written into the engine's KV buffer (KVCache.cat semantics, modeling_llama_kv.py:583-594).
        position_ids: None (0..L-1) or [3, L] multimodal rotary positions (Qwen2.5-VL).

        The prefill is MFMA-bound: its GEMMs (hipBLASLt) stay PyTorch ops; its attention is the library's causal kernel
        (vispec_prefill_attention, round 3: 185 us per layer at L = 2704 where torch's flash SDPA takes 296 us); the element-wise
        steps between them — RMSNorm, rotary + KV append, SwiGLU — run as the library's kernels (one launch each instead of ~6 / ~12 / 2 torch ops,
        same rounding points as the decode path): 11 launches per layer instead of ~35, which also keeps the host thread of a lane
        from holding the interpreter while other lanes wait to issue their rounds.

        past_len = P > 0: the L rows are positions [P, P + L) of a sequence whose cache rows [0, P) are live (an earlier prefill wrote them);
        position_ids, when given, is [3, L] for THESE rows.  K/V rows [P, P + L) are written, the rows attend over [0, P + L), and logits /
        hidden are returned for the L rows only.  The prompt is checked against the cache as P + L rows before any row is written.
        chunk_rows = C (any positive integer): the prompt runs as ceil(L / C) consecutive past_len pieces, each a full walk over the layers on
        at most C rows, so the activation workspace (the gate|up output [rows, 2 I] above all) is that of C rows instead of L.  The hidden
        rows go into one [L, D] buffer; the lm_head runs on the last row, or piece by piece under all_logits.  Shapes and dtypes returned are
        those of the unchunked call.  C >= L (or None) with past_len = 0 is the unchunked call: the same library calls, names, order, arguments.
        Both forms run the offset kernels (vispec_rope_append_varlen_at, vispec_prefill_attention_varlen_at: head_dim 128 only — other head
        sizes are refused with VispecError).

        Arithmetic class of a chunked / offset prefill: the row-wise kernels (RMSNorm, residual add, SwiGLU, row quantisation, scale/cast) and
        both offset kernels are bit-identical, row for row, to the unchunked path.  The library GEMMs run at M = the piece's rows and may sum
        in another fp32 order than at M = L.  A chunked prefill is therefore the oracle's arithmetic within the bf16 bars of the
        single-request comparisons — not guaranteed bit-identical to the unchunked prefill."""
        c, eng = self.cfg, self.engine
        if (chunk_rows is not None and int(chunk_rows) < 1) or int(past_len) < 0:
            raise ValueError("prefill: chunk_rows must be a positive integer (or None) and past_len >= 0")
        if int(past_len) > 0 or (chunk_rows is not None and int(chunk_rows) < int(inputs_embeds.shape[0])):
            return self._prefill_pieces(inputs_embeds, all_logits, position_ids, chunk_rows, int(past_len))
        eng.check_prompt_fits(int(inputs_embeds.shape[0]))  # before the first KV row is written
        lib, st = eng.lib, eng._stream()
        x = inputs_embeds.to(self.dtype).contiguous()
        Ln = x.shape[0]
        H, Hk, hd = c.num_heads, c.num_kv_heads, c.head_dim
        QKV = (H + 2 * Hk) * hd
        if position_ids is not None and position_ids.dim() == 2:
            cos, sin = self.mrope_cos_sin(position_ids)  # per-request tables [L, hd]: row m is the rotary of prompt position m
            cos, sin = cos.contiguous(), sin.contiguous()
        else:
            cos, sin = eng.t_cos, eng.t_sin
        kv = eng.target_kv
        S = kv.shape[3]

        def seq_step(i, qkv):
            # rotary at position m (bf16 rounding points of the reference) on q in place; k (rotated) and v -> cache rows [0, L)
            L.check(lib.vispec_rope_append(eng.h, st, _p(qkv), Ln, H, Hk, hd, _p(cos), _p(sin), None, None, _p(kv[2 * i]), _p(kv[2 * i + 1]), S, None))
            if hd == 128:  # causal attention of the L rows over the cache rows just written: the library's kernel (no [H, L, L] tensor,
                # the reference's eager score arithmetic for LLaVA — the decode kernel's — instead of a flash kernel's)
                a = torch.empty(Ln, H * hd, dtype=self.dtype, device=x.device)
                L.check(lib.vispec_prefill_attention(eng.h, st, _p(qkv), QKV, _p(kv[2 * i]), _p(kv[2 * i + 1]), S, H, Hk, Ln, _p(a), H * hd,
                                                     int(c.attn_impl == "eager")))
                return a
            q = qkv[:, : H * hd].view(Ln, H, hd).transpose(0, 1)  # (other head sizes: torch's SDPA)
            return _sdpa(q[None], kv[2 * i, :, :, :Ln], kv[2 * i + 1, :, :, :Ln], H != Hk)[0].transpose(0, 1).reshape(Ln, H * hd)

        x = x.clone() if x.data_ptr() == inputs_embeds.data_ptr() else x  # the residual stream is updated in place
        hidden = self._walk_layers(eng, x, seq_step)
        logits = scaled_linear(hidden if all_logits else hidden[-1:], self.w.lm_head, None, getattr(self.w, "lm_head_scale", None)).float()
        return logits, hidden.contiguous()

    def _lm_head(self, hidden):
        return scaled_linear(hidden, self.w.lm_head, None, getattr(self.w, "lm_head_scale", None)).float()

    def _prefill_pieces(self, inputs_embeds, all_logits, position_ids, chunk_rows, past_len):
        """prefill() at an offset and / or in pieces: rows [lo, hi) of the prompt are one segment at pos0 = past_len + lo."""
        c, eng = self.cfg, self.engine
        if c.head_dim != 128:
            raise L.VispecError(f"prefill: head_dim {c.head_dim} is not served by the offset kernels (head_dim 128 only); "
                                "run the unchunked prefill (chunk_rows=None, past_len=0)")
        x = inputs_embeds.to(self.dtype).reshape(-1, c.hidden_size)
        Ln = int(x.shape[0])
        eng.check_prompt_fits(past_len + Ln)  # before the first KV row is written
        tabs = None
        if position_ids is not None and position_ids.dim() == 2:
            if position_ids.shape[-1] != Ln:
                raise ValueError("prefill: position_ids is None or [3, L] for the L rows of this call")
            tabs = self.mrope_cos_sin(position_ids)  # [L, hd] each, once for all pieces
        C_ = Ln if chunk_rows is None else int(chunk_rows)
        hidden = torch.empty(Ln, c.hidden_size, dtype=self.dtype, device=x.device)
        parts = []
        for lo in range(0, Ln, C_):
            hi = min(Ln, lo + C_)
            h = self._walk_piece([eng], x[lo:hi].clone(), [(0, 0, past_len + lo, hi - lo)], None if tabs is None else (tabs[0][lo:hi], tabs[1][lo:hi]))
            hidden[lo:hi] = h
            if all_logits:
                parts.append(self._lm_head(h))
        logits = (parts[0] if len(parts) == 1 else torch.cat(parts)) if all_logits else self._lm_head(hidden[-1:])
        return logits, hidden

    def _walk_piece(self, engines, x, plan, tables, at=True):
        """One varlen walk (a piece of a chunked prefill, or a sub-batch of whole prompts): the layer walk on x [rows, D] (a buffer of the
        caller's: updated in place) whose segments are plan = [(request, row0, pos0, len), ...] (plan_prefill_pieces): rows
        [row0, row0 + len) are positions [pos0, pos0 + len) of engines[request]'s sequence.  tables: None = the shared rotary table indexed by
        position, or (cos, sin) [rows, hd] covering exactly this walk's rows (M-RoPE).  at: the offset entries on PrefillSegAt; False (every
        pos0 is 0): the `_varlen` entries on PrefillSeg.  The only place that fills a segment table and issues the two calls.
        -> hidden [rows, D]."""
        c, eng = self.cfg, engines[plan[0][0]]
        lib, st = eng.lib, eng._stream()
        H, Hk, hd = c.num_heads, c.num_kv_heads, c.head_dim
        QKV = (H + 2 * Hk) * hd
        S = eng.target_kv.shape[3]
        rows = x.shape[0]
        if tables is None:
            shared = max(engines, key=lambda e: e.t_cos.shape[0])
            cos, sin, table_global = shared.t_cos, shared.t_sin, 0
        else:
            cos, sin, table_global = tables[0].contiguous(), tables[1].contiguous(), 1
        n = len(plan)
        if at:
            Seg, rope, attn = L.PrefillSegAt, lib.vispec_rope_append_varlen_at, lib.vispec_prefill_attention_varlen_at
        else:
            Seg, rope, attn = L.PrefillSeg, lib.vispec_rope_append_varlen, lib.vispec_prefill_attention_varlen
        assert at or not any(pos0 for _, _, pos0, _ in plan), "the _varlen entries take whole prompts (pos0 = 0)"
        segs = (Seg * n)()

        def seq_step(i, qkv):
            for s_, (r, row0, pos0, ln) in enumerate(plan):
                kv = engines[r].target_kv[2 * i].data_ptr(), engines[r].target_kv[2 * i + 1].data_ptr()
                segs[s_] = Seg(row0, ln, pos0, 0, *kv) if at else Seg(row0, ln, *kv)
            L.check(rope(eng.h, st, _p(qkv), H, Hk, hd, _p(cos), _p(sin), table_global, segs, n, S))
            a = torch.empty(rows, H * hd, dtype=self.dtype, device=x.device)
            L.check(attn(eng.h, st, _p(qkv), QKV, segs, n, S, H, Hk, _p(a), H * hd, int(c.attn_impl == "eager")))
            return a

        return self._walk_layers(eng, x, seq_step)

    def _walk_layers(self, eng, x, seq_step):
        """The layer walk of both prefills: x [rows, D], the residual stream (updated in place) -> hidden [rows, D] post-final-norm.
        seq_step(i, qkv) is the one step in which a single sequence and a varlen batch differ: rotary + KV append + causal attention of layer i
        on the q|k|v rows [rows, QKV] (q rotated in place), returning the attention output [rows, H hd]."""
        c, lib, st = self.cfg, eng.lib, eng._stream()
        Ln = x.shape[0]
        prefill_gemm_selection()

        def rmsnorm(t, w):
            out = torch.empty_like(t)
            L.check(lib.vispec_rmsnorm(eng.h, st, _p(t), _p(w), _p(out), Ln, c.hidden_size, c.rms_norm_eps))
            return out

        def add_rmsnorm(t, r, w):  # t <- t + r (in place), returns RMSNorm(t) * w: one launch instead of a torch add + the norm
            out = torch.empty_like(t)
            L.check(lib.vispec_add_rmsnorm(eng.h, st, _p(t), _p(r), _p(w), _p(out), Ln, c.hidden_size, c.rms_norm_eps))
            return out

        y = None  # the previous layer's down_proj output, added to the residual stream by the next norm's launch
        # W8A8 (fp8a8): the q|k|v, gate|up and down inputs are quantised row by row like the decode forwards' and multiplied on the fp8 MFMA
        a8 = getattr(eng, "target_weight_dtype", "bf16") == "fp8a8" and hasattr(self.w, "codes8")
        for i, lw in enumerate(self.w.layers):
            c8 = self.w.codes8[i] if a8 else {}
            h = rmsnorm(x, lw["ln1"]) if y is None else add_rmsnorm(x, y, lw["ln1"])
            qkv = scaled_linear(h, lw["wqkv"], lw["bqkv"], lw.get("wqkv_scale"), c8.get("wqkv"))  # [rows, QKV]
            a = seq_step(i, qkv)
            h = add_rmsnorm(x, scaled_linear(a, lw["wo"], None, lw.get("wo_scale")), lw["ln2"])
            gu = scaled_linear(h, lw["wgu"], None, lw.get("wgu_scale"), c8.get("wgu"))  # [rows, 2I]
            act = torch.empty(Ln, c.intermediate_size, dtype=self.dtype, device=x.device)
            L.check(lib.vispec_silu_mul(eng.h, st, _p(gu), gu.shape[1], _p(act), c.intermediate_size, Ln, c.intermediate_size))
            y = scaled_linear(act, lw["wdown"], None, lw.get("wdown_scale"), c8.get("wdown"))
        return rmsnorm(x, self.w.norm) if y is None else add_rmsnorm(x, y, self.w.norm)

    # widest activation of a prefill: the gate|up GEMM's output [rows, 2 I] (fp32 accumulators under W8A16, bf16 otherwise)
    PREFILL_BATCH_ACT_BYTES = 4 << 30

    def prefill_batch_max_rows(self, target_weight_dtype: str = "bf16") -> int:
        """Default `max_rows` of prefill_batch: the rows whose gate|up output stays within PREFILL_BATCH_ACT_BYTES (4 GiB), a multiple of 128,
        at most 131 072 (the varlen attention launch takes 1536 row blocks)."""
        per_row = 2 * self.cfg.intermediate_size * (4 if target_weight_dtype == "fp8" else 2)
        return max(128, min(131072, self.PREFILL_BATCH_ACT_BYTES // per_row // 128 * 128))

    @torch.no_grad()
    def prefill_batch(self, engines, embeds_list, position_ids_list=None, all_logits: bool = False, max_rows: Optional[int] = None,
                      chunk_rows: Optional[int] = None, past_lens=None):
        """prefill() for up to eight requests of one leader group on ONE walk over the weights: embeds_list[i] [L_i, D] bf16 is the prompt of
        engines[i]; returns [(logits fp32 [L_i or 1, V], hidden [L_i, D])] in request order, the shapes and dtypes of prefill().  K/V rows
        [0, L_i) of every layer go to engines[i].target_kv.  position_ids_list[i]: None or [3, L_i] (Qwen2.5-VL M-RoPE), as prefill().

        The prompts' rows are concatenated (sum L rows): the row-wise kernels and the GEMMs run once per layer on all of them, the rotary + KV
        append and the attention through the library's varlen entries (vispec_rope_append_varlen, vispec_prefill_attention_varlen: one launch
        per layer, every sequence on its own cache, M-RoPE tables concatenated like the rows).  The lm_head runs per request.
        Every prompt is checked against its cache BEFORE any KV row of any request is written: a prompt that cannot fit raises VispecError and
        leaves every cache untouched.  Engines of two leader groups (other weights, device, stream or cache size) raise ValueError.  The varlen
        kernels are head_dim 128 only: other head sizes are refused here (prefill() per request serves them through SDPA).

        max_rows: a batch of more rows is split into consecutive sub-batches of at most max_rows rows each (a single longer prompt runs alone).
        Default prefill_batch_max_rows(): the gate|up output — the widest activation, [rows, 2 I] — within 4 GiB: 97 536 rows for LLaVA-7B
        (8 x 2704 rows take 0.95 GB there), 56 576 for Qwen2.5-VL-7B in bf16 / W8A8, 28 288 under W8A16 (fp32 accumulators).

        Arithmetic class: the row-wise kernels (RMSNorm, residual add, SwiGLU, row quantisation, scale/cast) and both varlen kernels are
        bit-identical, row for row, to the per-request path.  The library GEMMs run at M = sum L: those shapes are not in the recorded
        TunableOp table (prefill_gemm_selection), so they run the library's default solution, which may sum in another fp32 order than the
        solution of the request's own M.  A request's batched prefill is therefore the oracle's arithmetic within the bf16 bars of the
        single-request comparisons — not guaranteed bit-identical to its solo prefill.

        chunk_rows = C (any positive integer below sum L; None or more leaves the call as it is): the concatenated row stream of the batch is
        cut into consecutive pieces of at most min(C, max_rows) rows (plan_prefill_pieces): a piece may hold the tail of one prompt, whole
        prompts and the head of the next — up to eight segments, each at its pos0 — and is one walk over the layers through the offset varlen
        entries (vispec_rope_append_varlen_at, vispec_prefill_attention_varlen_at), so the activation workspace is that of C rows.  Same
        arithmetic class: the row-wise kernels and both offset kernels are bit-identical per row, the library GEMMs run at M = the piece's
        rows and may sum in another fp32 order — the oracle's arithmetic within the bf16 bars, not guaranteed bit-identical to the
        unchunked call.

        past_lens = [P_i, ...] (one per engine; the default None is today's calls, byte for byte): embeds_list[i] holds the rows BEHIND P_i
        cache rows of engines[i] that are already live (a shared prompt prefix put there by Engine.load_kv_rows; P_i = 0: a whole prompt),
        position_ids_list[i] is [3, L_i] for those rows, and request i is one segment (i, row0, P_i, L_i) of the walk — always the offset
        varlen entries, in pieces of at most min(chunk_rows, max_rows) rows and eight segments.  K/V rows [P_i, P_i + L_i) are written, logits
        and hidden cover the L_i new rows; every prompt is checked as P_i + L_i rows before any row is written.  Arithmetic class as chunk_rows:
        a request's rows are bit-identical per row in the offset kernels, its GEMMs run at M = the piece's rows."""
        c = self.cfg
        n = len(engines)
        if past_lens is not None and (len(past_lens) != n or any(int(p_) < 0 for p_ in past_lens)):
            raise ValueError("prefill_batch: one non-negative past length per engine")
        past = None if past_lens is None else [int(p_) for p_ in past_lens]
        if n < 1 or len(embeds_list) != n or (position_ids_list is not None and len(position_ids_list) != n):
            raise ValueError("prefill_batch: one prompt (and one position_ids entry) per engine")
        eng0 = engines[0]
        root = eng0.leader or eng0
        for e in engines:
            if (e.leader or e) is not root or e.device != eng0.device or e.target_kv.shape != eng0.target_kv.shape:
                raise ValueError("prefill_batch: the engines must belong to one leader group (same weights, device, stream and cache size)")
        if len(set(id(e) for e in engines)) != n:
            raise ValueError("prefill_batch: an engine appears twice (one request per KV cache)")
        if self.engine is None or (self.engine.leader or self.engine) is not root:
            raise ValueError("prefill_batch: the engines do not run this model's weights")
        if c.head_dim != 128:
            raise L.VispecError(f"prefill_batch: head_dim {c.head_dim} is not served by the varlen kernels (head_dim 128 only); "
                                "run prefill() per request")
        xs = [e_.to(self.dtype).reshape(-1, c.hidden_size) for e_ in embeds_list]
        lens = [int(x.shape[0]) for x in xs]
        for i, (e, ln) in enumerate(zip(engines, lens)):  # every prompt, before the first KV row of any request is written
            e.check_prompt_fits(ln if past is None else past[i] + ln)
        pos = list(position_ids_list) if position_ids_list is not None else [None] * n
        for i, pz in enumerate(pos):
            if pz is not None and (pz.dim() != 2 or pz.shape[-1] != lens[i]):
                raise ValueError("prefill_batch: position_ids entries are None or [3, L_i]")
        if max_rows is None:
            max_rows = self.prefill_batch_max_rows(getattr(eng0, "target_weight_dtype", "bf16"))
        if chunk_rows is not None:
            if int(chunk_rows) < 1:
                raise ValueError("prefill_batch: chunk_rows must be a positive integer (or None)")
            if past is not None or int(chunk_rows) < sum(lens):
                return self._prefill_batch_pieces(engines, xs, pos, all_logits, max(1, min(int(chunk_rows), int(max_rows))), past)
        if past is not None:
            return self._prefill_batch_pieces(engines, xs, pos, all_logits, max(1, int(max_rows)), past)
        out, lo = [], 0
        while lo < n:  # consecutive sub-batches of at most max_rows rows and eight requests
            hi, rows = lo + 1, lens[lo]
            while hi < n and hi - lo < 8 and rows + lens[hi] <= max_rows:
                rows += lens[hi]
                hi += 1
            out += self._prefill_rows(engines[lo:hi], xs[lo:hi], pos[lo:hi], all_logits)
            lo = hi
        return out

    def _prefill_batch_pieces(self, engines, xs, pos, all_logits, chunk_rows, past=None):
        """prefill_batch in pieces of at most chunk_rows rows of the concatenated row stream; past[r] live cache rows precede xs[r] (None: 0)."""
        c = self.cfg
        lens = [int(x.shape[0]) for x in xs]
        past = [0] * len(xs) if past is None else past
        tabs = None
        if any(pz is not None for pz in pos):  # per-request M-RoPE tables; a text-only prompt among them uses the plain table's rows
            shared = max(engines, key=lambda e: e.t_cos.shape[0])
            tabs = [self.mrope_cos_sin(pz) if pz is not None else (shared.t_cos[P:P + ln], shared.t_sin[P:P + ln]) for pz, ln, P in zip(pos, lens, past)]
        hiddens = [torch.empty(ln, c.hidden_size, dtype=self.dtype, device=xs[0].device) for ln in lens]
        for piece in plan_prefill_pieces(lens, chunk_rows, 8, past_lens=past):
            own = [(r, pos0 - past[r], ln) for r, _, pos0, ln in piece]  # (request, first row within xs[request], rows)
            x = torch.cat([xs[r][p0:p0 + ln] for r, p0, ln in own], dim=0).contiguous()  # (a copy: the residual stream is updated in place)
            if len(piece) == 1 and x.data_ptr() == xs[own[0][0]][own[0][1]:].data_ptr():
                x = x.clone()
            tables = None if tabs is None else tuple(torch.cat([tabs[r][k][p0:p0 + ln] for r, p0, ln in own]).contiguous() for k in (0, 1))
            h = self._walk_piece(engines, x, piece, tables)
            for (r, p0, ln), (_, row0, _, _) in zip(own, piece):
                hiddens[r][p0:p0 + ln] = h[row0:row0 + ln]
        return [(self._lm_head(hs if all_logits else hs[-1:]), hs) for hs in hiddens]  # the lm_head per request, at prefill()'s own shapes

    def _prefill_rows(self, engines, xs, pos, all_logits):
        """One sub-batch of prefill_batch: whole prompts, request i the segment (i, row0_i, 0, L_i) of one walk on the concatenated rows."""
        lens = [int(x.shape[0]) for x in xs]
        row0 = [0]
        for ln in lens[:-1]:
            row0.append(row0[-1] + ln)
        x = torch.cat(xs, dim=0).contiguous()  # (a copy: the residual stream is updated in place)
        if len(xs) == 1 and x.data_ptr() == xs[0].data_ptr():
            x = x.clone()
        tables = None
        if any(pz is not None for pz in pos):  # per-request M-RoPE tables, concatenated like the rows: table row = global row
            shared = max(engines, key=lambda e: e.t_cos.shape[0])
            tabs = [self.mrope_cos_sin(pz) if pz is not None else (shared.t_cos[:ln], shared.t_sin[:ln]) for pz, ln in zip(pos, lens)]
            tables = torch.cat([t[0] for t in tabs]), torch.cat([t[1] for t in tabs])
        hidden = self._walk_piece(engines, x, [(i, r0, 0, ln) for i, (r0, ln) in enumerate(zip(row0, lens))], tables, at=False)
        out = []
        for r0, ln in zip(row0, lens):  # the lm_head per request, at prefill()'s own shapes
            hs = hidden[r0:r0 + ln]
            out.append((self._lm_head(hs if all_logits else hs[-1:]), hs.clone() if len(lens) > 1 else hs.contiguous()))
        return out

    def eval(self):
        return self
