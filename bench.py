#!/usr/bin/env python3
"""bench.py — accepted output tokens/s of the ViSpec draft-and-verify path on MI355X.

Workload (BASELINE.json configs[1]): LLaVA-v1.6-vicuna-7B-shaped target + ViSpec draft, bf16, one request =
48 template tokens + one image run of 2144 image tokens + 512 text tokens (L = 2704), up to 512 new tokens, temperature 0,
total_token 30 / depth 3 / top_k 8 / num_q 2.  A "step" = one whole specgenerate() request (prefill + all rounds), exactly what
the reference harness brackets with its wall clock (gen_spec_answer_coco_caption.py:221-232), on every request slot of the GPU:
--lanes (4) concurrent streams x --cohort (8) requests per lane that share each pass over the weights (every request keeps the
reference's batch-1 semantics; cohorts of up to four keep its exact single-request arithmetic, cohorts of five to eight run the
cohort-8 GEMM whose fp32 summation order differs — csrc/gemm_c8.h).  Inputs/weights are resident in HBM when the timed region starts.

No checkpoints exist on the box (no network), so weights are synthetic: random N(0,0.02) layers with a successor structure on
embed/lm_head (vispec_amd/synth_gpu.py) that makes the draft agree with the target on ~88.5 % of the tokens.  Acceptance is
therefore MEASURED by the real verify/accept kernels (tau lands near the reference's published 2.98), not scripted; the
weight-value-independent rounds/s is reported next to it.

    python bench.py [--gpus N] [--steps K] [--warmup W]
    torchrun --nnodes=1 --nproc-per-node N bench.py --gpus N ...      (one rank per GPU, replicas only)
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

# Four lanes need four hardware queues of their own next to the default stream's: the ROCm runtime maps streams onto
# GPU_MAX_HW_QUEUES (default 4) queues and two lanes sharing one queue serialise (883 vs 1011 tok/s measured).  Must be in the
# environment before the HIP runtime initialises, i.e. before torch is imported.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from vispec_amd.evaluation.bench_launch import host_usage, pin_to_gpu_numa_node, request_plan, run_lanes, self_launch  # noqa: E402,F401
from vispec_amd.evaluation.bench_vision import InLoopFrontEnd, VisionInput, build_front_end  # noqa: E402,F401

N_PRE, N_IMG, N_POST = 48, 2144, 512
MAX_NEW = 512
# Acceptance is measured on a synthetic successor pair whose draft disagrees with the target on a fraction rho of the vocabulary.
# rho is chosen per model so that the measured mean accept length lands near the reference's published one (README.md:186-195 of
# the reference, T=0 averages): tau = p + p^2 + p^3 + p^4 with p ~ 1 - 0.91 rho at depth 3.
TAU_PUBLISHED = {"tiny": 2.98, "llava7b": 2.98, "llava13b": 2.89, "qwen7b": 2.24, "qwen7b-hires": 2.24, "qwen7b-fp8": 2.24, "qwen7b-fp8a8": 2.24}
RHO = {"tiny": 0.115, "llava7b": 0.115, "llava13b": 0.125, "qwen7b": 0.24, "qwen7b-hires": 0.24, "qwen7b-fp8": 0.24, "qwen7b-fp8a8": 0.24}
TREE = dict(total_token=30, depth=3, top_k=8, num_q=2)
# --model selects the BASELINE.json config; the default (configs[1]) is the headline line, the others are extra coverage runs
MODELS = {
    # TEST-ONLY (tests/test_world8_gpu.py: eight ranks of the N > 1 control flow on ONE GPU): a LLaVA-shaped target an eighth of the width, four
    # layers — the same request shape, launch sequence and kernels (head_dim 128), 0.3 GB of weights per rank.  Never a bench line.
    "tiny": dict(name="LLaVA-shaped TEST model (hidden 1024, 4 layers; control-flow tests only)",
                 desc="1 image (2144 image tokens) + 512 text + 48 template tokens per request (L=2704)"),
    "llava7b": dict(name="LLaVA-v1.6-vicuna-7B", desc="1 image (2144 image tokens) + 512 text + 48 template tokens per request (L=2704)"),
    "llava13b": dict(name="LLaVA-v1.6-vicuna-13B", desc="1 image (2144 image tokens) + 512 text + 48 template tokens per request (L=2704)"),
    "qwen7b": dict(name="Qwen2.5-VL-7B-Instruct", desc="4 images of 32x32 patches (256 merged tokens each) in a multi-turn prompt + 512 text tokens (L=1584)"),
    "qwen7b-hires": dict(name="Qwen2.5-VL-7B-Instruct", desc="one 1280x960 image = 68x92 patches (1564 merged tokens) + 512 text tokens (L=2124), bf16 weights"),
    "qwen7b-fp8": dict(name="Qwen2.5-VL-7B-Instruct (fp8 e4m3 target weights, W8A16)",
                       desc="one 1280x960 image = 68x92 patches (1564 merged tokens) + 512 text tokens (L=2124)"),
    "qwen7b-fp8a8": dict(name="Qwen2.5-VL-7B-Instruct (fp8 e4m3 target weights AND activations: the fp8 MFMA, W8A8)",
                         desc="one 1280x960 image = 68x92 patches (1564 merged tokens) + 512 text tokens (L=2124)"),
}
MODEL = "llava7b"
# On the command line the name a reader tries first for BASELINE config 5 ("Qwen2.5-VL-7B fp8 weights (CDNA4 fp8 MFMA)") runs the line that
# config is: W8A8 on v_mfma_scale_f32_32x32x64_f8f6f4.  The W8A16 sibling keeps a labelled name.  (Inside the module — tests, tools — the
# keys of MODELS keep their round-4 meaning: "qwen7b-fp8" = W8A16, "qwen7b-fp8a8" = W8A8.)
CLI_MODEL_ALIASES = {"qwen7b-fp8": "qwen7b-fp8a8", "qwen7b-fp8-w8a16": "qwen7b-fp8"}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# Real checkpoints: when $VISPEC_WEIGHTS (or --weights-dir) holds the published pair under its hub names — or
# --base-model-path / --spec-model-path (the reference harness's own flags, gen_spec_answer_coco_caption.py:292-300) name the directories —
# the weights come from SpecModel.from_pretrained (spec_model_ours.py:147-166) and tau is what those weights accept on the synthetic prompts.
HUB_NAMES = {"llava7b": ("llava-hf/llava-v1.6-vicuna-7b-hf", "JLKang/ViSpec-llava-v1.6-vicuna-7b-hf"),
             "llava13b": ("llava-hf/llava-v1.6-vicuna-13b-hf", "JLKang/ViSpec-llava-v1.6-vicuna-13b-hf"),
             "qwen7b": ("Qwen/Qwen2.5-VL-7B-Instruct", "JLKang/ViSpec-Qwen2.5-VL-7B-Instruct")}
REAL_WEIGHTS = None  # (base_model_path, spec_model_path) once resolved


def resolve_weights(args):
    base, spec = args.base_model_path, args.spec_model_path
    root = args.weights_dir or os.environ.get("VISPEC_WEIGHTS")
    if not (base and spec) and root:
        names = HUB_NAMES.get(MODEL.split("-")[0])  # ("qwen7b-fp8a8", "qwen7b-hires" ... share the bf16 checkpoint pair)
        if names:
            cand = [os.path.join(root, n) for n in names]
            cand_flat = [os.path.join(root, n.split("/")[-1]) for n in names]
            for b_, s_ in (cand, cand_flat):
                if os.path.isdir(b_) and os.path.isdir(s_):
                    base, spec = base or b_, spec or s_
                    break
    if bool(base) != bool(spec):
        raise SystemExit("error: --base-model-path and --spec-model-path go together")
    if base and not (os.path.isdir(base) and os.path.isdir(spec)):
        raise SystemExit(f"error: checkpoint directories not found: {base} / {spec}")
    return (base, spec) if base else None


REFILL = True  # --no-refill: cohort by cohort
WIDE_RB = -1  # --wide-row-blocks: -1 = automatic (one lane: 0 = two row blocks where four cannot fill the GPU; several lanes: 84 = eight for bf16 weights and for W8A8, four for fp8 weights with bf16 activations)


def model_configs():
    """-> (TargetConfig, DraftConfig) of bench.MODEL at the published sizes."""
    from vispec_amd.engine import LLAVA_16_7B, LLAVA_16_13B, QWEN25_VL_7B, DraftConfig, TargetConfig
    if MODEL == "tiny":
        tcfg = TargetConfig(hidden_size=1024, num_heads=8, num_kv_heads=8, intermediate_size=2816, vocab_size=32064, num_layers=4, max_position_embeddings=4096)
        dcfg = DraftConfig(hidden_size=1024, num_heads=8, intermediate_size=2816, vocab_size=32064, max_position_embeddings=4096)
    elif MODEL == "llava13b":
        tcfg = TargetConfig(**LLAVA_16_13B)
        dcfg = DraftConfig(hidden_size=5120, num_heads=40, intermediate_size=13824, vocab_size=32064, max_position_embeddings=4096)
    elif MODEL.startswith("qwen7b"):
        tcfg = TargetConfig(**QWEN25_VL_7B)
        dcfg = DraftConfig(hidden_size=3584, num_heads=28, intermediate_size=18944, vocab_size=152064, max_position_embeddings=8192,
                           rms_norm_eps=1e-6, rope_theta=1e6, qkv_bias=True)  # vispec/train/qwen2.5_vl_7B_config.json
    else:
        tcfg = TargetConfig(**LLAVA_16_7B)
        dcfg = DraftConfig(hidden_size=4096, num_heads=32, intermediate_size=11008, vocab_size=32064, max_position_embeddings=4096)
    return tcfg, dcfg


def synth_pair(device, seed, structured=True):
    """The synthetic weight pair of bench.MODEL on the device -> (tcfg, dcfg, TargetWeights, DraftWeightsDev) (also tests/ckpt_writer.py)."""
    from vispec_amd import synth_gpu
    tcfg, dcfg = model_configs()
    tw, dw = synth_gpu.make_pair(tcfg, dcfg, device, seed=seed, structured=structured, num_q=TREE["num_q"], rho=RHO[MODEL],
                                 succ_hi=min(tcfg.vocab_size, 151640 if MODEL.startswith("qwen") else 32000))
    return tcfg, dcfg, tw, dw


def build_models(device, seed, rank, world, lanes, cohort=1, structured=True):
    """`lanes` SpecModels (one vispec_ctx + KV cache + stream each) sharing ONE copy of the weights on this GPU; with cohort = 2..4 every lane
    also gets cohort members (further request contexts on the same weight pass): returns [leader, member, ...] lists then.
    structured=False (tests/test_unstructured_gpu.py only): plain random matrices, flat logits — never the bench workload."""
    from vispec_amd import parallel
    from vispec_amd.model import SpecModel
    from vispec_amd.model.cnets_ours import Model
    from vispec_amd.model.target import TargetLM
    tcfg, dcfg = model_configs()
    real = REAL_WEIGHTS is not None
    if real:  # every rank reads the checkpoint itself (no collective needed); the lanes share that one copy
        first = SpecModel.from_pretrained(base_model_path=REAL_WEIGHTS[0], spec_model_path=REAL_WEIGHTS[1], device=str(device), **TREE)
        tcfg, dcfg = first.base_model.cfg, first.spec_layer.config
        tw, dw = first.engine.tw, first.engine.dw
        first.engine.close()
        del first
    else:  # rank 0 creates the weights; the others allocate same-shaped buffers (different seed) and receive rank 0's over RCCL
        _, _, tw, dw = synth_pair(device, seed if rank == 0 else seed + 1000 + rank, structured)
    t_rep = 0.0
    if world > 1 and not real:
        import torch.distributed as dist
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.time()
        try:
            nbytes = parallel.replicate_weights(list(tw.tensors()) + list(dw.tensors()), src=0)
            torch.cuda.synchronize()
            same = parallel.all_equal(parallel.checksum(list(tw.tensors()) + list(dw.tensors())))
        except Exception as e:  # never lose the run to the start-up collective: rebuild rank 0's weights locally (same seed)
            log(f"[rank {rank}] weight replication failed ({e}); regenerating rank 0's weights locally")
            same, nbytes = False, 0
        t_rep = time.time() - t0
        if not same:
            del tw, dw
            torch.cuda.empty_cache()
            _, _, tw, dw = synth_pair(device, seed, structured)
        log(f"[rank {rank}] replicated {nbytes / 1e9:.2f} GB of weights over {'RCCL' if dist.get_backend() == 'nccl' else dist.get_backend()} "
            f"in {t_rep:.2f} s, checksums {'equal' if same else 'differ: weights regenerated locally'}")
    sms = []
    for _ in range(lanes):
        base = TargetLM(tcfg, tw)
        draft = Model(dcfg, dw, total_tokens=TREE["total_token"], depth=TREE["depth"], top_k=TREE["top_k"], num_q=TREE["num_q"])
        lead = SpecModel(base, draft, target_weight_dtype="fp8a8" if MODEL.endswith("fp8a8") else ("fp8" if MODEL.endswith("fp8") else "bf16"), **TREE)
        # one lane has the GPU to itself: smaller workgroups where the large ones cannot fill it; several lanes: every launch costs CU-time
        # in proportion to the bytes its workgroups ingest, so the bf16 GEMMs take eight row blocks per workgroup (same-box A/Bs in
        # profiles/README.md, round 4: +4 % on the LLaVA / Qwen bf16 lines; fp8 weights stay on four)
        lead.engine.set_wide_row_blocks(WIDE_RB if WIDE_RB >= 0 else (0 if lanes == 1 else 84))
        sms.append([lead] + [lead.make_cohort_member() for _ in range(cohort - 1)] if cohort >= 2 else lead)
    return sms, tcfg, t_rep


def make_request(tcfg, req_id, device):
    """-> (input_ids [1,L] on the device, specgenerate kwargs).  The vision tower is not on the path (it stays PyTorch in a
    deployment): its output — the projected image features, N(0,1)*0.05 per SURVEY §8(d) — is part of the request and, like
    the ids, is resident in HBM before the timed region starts."""
    ids, kw = _make_request(tcfg, req_id, device)
    n, seed = kw["pixel_values"]
    from vispec_amd.model.target import SyntheticVision
    kw["pixel_values"] = SyntheticVision(tcfg.hidden_size).features(int(n), int(seed), device, torch.bfloat16)
    if FRONT_END is not None:  # the front-end runs inside specgenerate: the request carries its pixels as well
        pixels, sizes = FRONT_END.pixels(req_id)
        kw["pixel_values"] = VisionInput(pixels, kw["pixel_values"], sizes)
    return ids, kw


def _make_request(tcfg, req_id, device):
    from vispec_amd import synth_gpu
    if MODEL == "qwen7b":  # 4 image runs of 256 merged tokens, text in between (multi-turn), 512 text tokens in total
        g = torch.Generator().manual_seed(1000 + req_id)
        parts, grids = [], []
        for seg in (48, 96, 96, 96):
            parts += [torch.randint(3, 151640, (seg,), generator=g), torch.full((256,), tcfg.image_token_index)]
            grids.append((1, 32, 32))
        parts.append(torch.randint(3, 151640, (224,), generator=g))
        ids = torch.cat(parts)
        return ids[None].to(device), dict(pixel_values=(4 * 256, req_id), image_grid_thw=torch.tensor(grids))
    if MODEL in ("qwen7b-hires", "qwen7b-fp8", "qwen7b-fp8a8"):
        g = torch.Generator().manual_seed(1000 + req_id)
        ids = torch.cat([torch.randint(3, 151640, (48,), generator=g), torch.full((34 * 46,), tcfg.image_token_index),
                         torch.randint(3, 151640, (512,), generator=g)])
        return ids[None].to(device), dict(pixel_values=(34 * 46, req_id), image_grid_thw=torch.tensor([(1, 68, 92)]))
    ids = synth_gpu.make_request_ids(32000, N_PRE, N_IMG, N_POST, req_id, tcfg.image_token_index)
    return ids[None].to(device), dict(pixel_values=(N_IMG, req_id))


def algorithmic_bytes_per_round(tcfg, n_ctx, n_c, fp8=False):
    """B_round = B_target + (1+d)(B_draft_layer + B_lmhead) + KV_t(n) + (1+d) KV_d(n_c).
    fp8 (config 5): the streamed target GEMM weights and lm_head (which is also the draft's head) are 1 byte per element; the
    draft layer, activations and both KV caches stay bf16."""
    D, I, V, NL, d = tcfg.hidden_size, tcfg.intermediate_size, tcfg.vocab_size, tcfg.num_layers, TREE["depth"]
    kvd = tcfg.num_kv_heads * tcfg.head_dim
    wb = 1 if fp8 else 2
    b_target = wb * (NL * (2 * D * D + 2 * D * kvd + 3 * D * I) + V * D)
    b_draft_layer = 2 * (2 * 2 * D * D + 4 * D * D + 3 * D * I)
    b_lm = wb * V * D
    return b_target + (1 + d) * (b_draft_layer + b_lm) + 2 * NL * kvd * 2 * n_ctx + (1 + d) * 2 * D * 2 * n_c


def algorithmic_bytes_per_ar_step(tcfg, n_ctx, fp8=False):
    D, I, V, NL = tcfg.hidden_size, tcfg.intermediate_size, tcfg.vocab_size, tcfg.num_layers
    kvd = tcfg.num_kv_heads * tcfg.head_dim
    return (1 if fp8 else 2) * (NL * (2 * D * D + 2 * D * kvd + 3 * D * I) + V * D) + 2 * NL * kvd * 2 * n_ctx


CPU_THREADS = 16  # torch's CPU GEMMs at M <= 30 are memory-bound and get SLOWER with more threads on the 256-core GPU box
                  # (tools/cpu_probe.py, [30,4096]x[11008,4096]: 6.0 ms at 16 threads, 26 ms at 64, 261 ms at 256)


def cpu_models(sm, tcfg):
    """The oracle's PyTorch-CPU restatement (oracle/torch_cpu.py) over the GPU's own weight pair, copied to the host and de-fused to the
    reference's state-dict names — built once, used by both CPU legs.  Checker-side code only.  -> (target, draft, cores, seconds) or a string
    saying why not."""
    from oracle import torch_cpu as tc
    from oracle import vispec_oracle as vo
    avail_gb = 0.0
    try:
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable"):
                avail_gb = int(ln.split()[1]) / 1e6
    except OSError:
        pass
    n_par = sum(t.numel() for t in sm.engine.tw.tensors()) + sum(t.numel() for t in sm.engine.dw.tensors())
    need_gb = n_par * 4 * 1.6 / 1e9  # fp32 copies + transients
    if avail_gb and avail_gb < need_gb + 16:
        return f"skipped: {avail_gb:.0f} GB of host memory available, {need_gb:.0f} GB needed"
    cores = min(CPU_THREADS, os.cpu_count())
    torch.set_num_threads(cores)
    eng = sm.engine
    t0 = time.time()
    ot = vo.TargetLlama(vo.TargetConfig(tcfg.hidden_size, tcfg.num_heads, tcfg.num_kv_heads, tcfg.intermediate_size, tcfg.vocab_size, tcfg.num_layers,
                                        tcfg.max_position_embeddings, rms_norm_eps=tcfg.rms_norm_eps, rope_theta=tcfg.rope_theta,
                                        attn_impl=tcfg.attn_impl, mrope_section=tcfg.mrope_section), tc.split_fused_target(eng.tw, tcfg))
    dcfg = eng.dcfg
    od = vo.DraftModel(vo.DraftConfig(dcfg.hidden_size, dcfg.num_heads, dcfg.intermediate_size, dcfg.vocab_size, max(eng.kv_max_pos, eng.draft_max_pos),
                                      rms_norm_eps=dcfg.rms_norm_eps, rope_theta=dcfg.rope_theta, num_q=eng.num_q, total_token=eng.total_token,
                                      depth=eng.depth, top_k=eng.top_k), tc.split_fused_draft(eng.dw))
    ot.ops, od.ops = tc.TorchOps(), tc.TorchOps()
    return ot, od, cores, time.time() - t0


def cpu_baseline_leg(sm, tcfg, req, host, rounds=6, ar_steps=4, budget_s=20.0):
    """The reference's CPU path in spirit: the oracle's restatement on its PyTorch-CPU back end
    (oracle/torch_cpu.py: torch ops, fp32, torch.set_num_threads) runs the decode part of ONE request of the bench workload on the
    host — the very weights the GPU streams (copied to the host, de-fused to the reference's state-dict names), the same prompt at its
    real length: the draft prefill with image-token compression, then a bounded number (and a bounded time) of draft-and-verify rounds
    with MEASURED accept lengths and of plain AR steps on the same cores.  The 2704-token TARGET prefill (36 TFLOP: minutes on host
    cores) is not repeated on the CPU: its outputs — KV rows, hidden states, last logits — are copied from the GPU's prefill, which is
    how the CPU rounds start from the real context.  tokens/s = (tau + 1) / seconds per round, steady state.  Checker-side code only:
    nothing here is on the product path."""
    from oracle import torch_cpu as tc
    if isinstance(host, str):
        return dict(value=None, unit="tokens/s", cores=os.cpu_count(), kind="port", sample=host)
    ot, od, cores, t_copy = host
    eng = sm.engine
    ids, pix = req
    emb_in, mask, _, pos3, rope_delta = sm._merge_vision(ids.clone(), None, dict(pix))
    emb = emb_in.reshape(-1, emb_in.shape[-1]).float().cpu().numpy()
    mask_np = None if mask is None else mask.reshape(-1).cpu().numpy().astype(bool)
    L = emb.shape[0]
    # the GPU's target prefill of this prompt: KV rows [0, L) of every layer, post-norm hidden states, last logits row
    logits_g, hidden_g = sm.base_model.prefill(emb_in.reshape(-1, emb_in.shape[-1]).to(torch.bfloat16).contiguous(), position_ids=pos3)
    torch.cuda.synchronize()
    kv_g = eng.target_kv[:, 0, :, :L].float().cpu().numpy()
    r = tc.timed_request(ot, od, ids[0].cpu().numpy(), emb, mask_np, rounds=rounds, ar_steps=ar_steps, max_pos=L + 64 * (rounds + 2),
                         position_ids=None if pos3 is None else pos3.numpy(), rope_delta=int(rope_delta),
                         prefilled=(kv_g, hidden_g.float().cpu().numpy(), logits_g[-1].float().cpu().numpy()), budget_s=budget_s)
    rounds = len(r["verify_s"])
    t_round = (sum(r["verify_s"]) + sum(r["draft_s"])) / rounds
    tau = float(np.mean(r["accept_lengths"]))
    t_ar = float(np.mean(r["ar_s"]))
    return dict(value=round((tau + 1) / t_round, 3), unit=f"tokens/s ({cores} threads of {os.cpu_count()} host cores)", cores=cores, kind="port",
                ar_tokens_per_s=round(1.0 / t_ar, 3), speedup_vs_ar=round((tau + 1) / t_round * t_ar, 3), tau_measured=round(tau, 3),
                seconds_per_round=round(t_round, 3), verify_s=round(float(np.mean(r["verify_s"])), 3), draft_s=round(float(np.mean(r["draft_s"])), 3),
                draft_prefill_s=round(r["draft_prefill_s"], 2), host_cores=os.cpu_count(),
                sample=(f"the oracle on its PyTorch-CPU back end (torch {torch.__version__}, fp32, {cores} threads of {os.cpu_count()} host cores: more "
                        f"threads slow torch's M<=30 GEMMs down here): the decode part of one bench request on the host — target prefill of L={L} taken "
                        f"from the GPU (KV rows, hidden states), draft prefill with compression on the CPU ({r['draft_prefill_s']:.1f}s, outside the "
                        f"quoted rate), then {rounds} full draft-and-verify rounds at context {L}..{r['context']} (all {tcfg.num_layers} target layers + "
                        f"lm_head on T={eng.total_token} tree nodes {np.mean(r['verify_s']):.2f}s + draft round {np.mean(r['draft_s']):.2f}s per round) with the "
                        f"GPU's own weight pair (measured tau {tau:.2f}) and {ar_steps} AR steps ({t_ar:.2f}s each) on the same cores; host copy and "
                        f"de-fusing of the weights {t_copy:.0f}s (not timed)"))


def cpu_config0_leg(sm, tcfg, host, rounds=6, ar_steps=2, budget_s=8.0):
    """BASELINE.json configs[0] — "the reference's own CPU-runnable case" (SURVEY.md §8d cfg 1): one LLaVA-1.5-7B-shaped request END TO
    END on the host cores, target prefill included: L = 576 image + 32 + 35 text tokens, LLaVA-1.5 semantics (the draft sees token ids, no
    image-token compression: SURVEY.md fact 0.7), the oracle on its PyTorch-CPU back end with the weight pair the GPU benchmark uses
    (LLaVA-1.5-7B and v1.6-vicuna-7B share every dimension).  In the default line in a bounded form (~7 s of prefill + <= 8 s of rounds +
    2 AR steps, the host models shared with cpu_baseline_leg); --no-cpu-config0 drops it.  Checker-side code only."""
    from oracle import torch_cpu as tc
    if isinstance(host, str):
        return host
    ot, od, cores, _ = host
    n_pre, n_img, n_post = 35, 576, 32
    from vispec_amd import synth
    ids, emb, mask = synth.make_request(tcfg.vocab_size, tcfg.hidden_size, n_pre, n_img, n_post, seed=9000, image_token_id=tcfg.image_token_index,
                                        embed=ot.w["model.embed_tokens.weight"])
    L = len(ids)
    r = tc.timed_request(ot, od, ids, emb, None, rounds=rounds, ar_steps=ar_steps, max_pos=L + 64 * (rounds + 2), budget_s=budget_s,
                         draft_sees_embeds=False)
    n_rounds = len(r["verify_s"])
    new_tok = int(sum(a + 1 for a in r["accept_lengths"]))
    t_dec = sum(r["verify_s"]) + sum(r["draft_s"])
    wall = r["prefill_s"] + r["draft_prefill_s"] + t_dec
    t_ar = float(np.mean(r["ar_s"]))
    return dict(workload=f"LLaVA-1.5-7B-shaped request, L={L} (576 image + 67 text tokens), no image-token compression, whole request on {cores} host threads",
                prefill_s=round(r["prefill_s"], 2), draft_prefill_s=round(r["draft_prefill_s"], 2), rounds=n_rounds, new_tokens=new_tok,
                seconds_per_round=round(t_dec / n_rounds, 3), tau_measured=round(float(np.mean(r["accept_lengths"])), 3),
                tokens_per_s_decode=round(new_tok / t_dec, 3), tokens_per_s_end_to_end=round(new_tok / wall, 3),
                ar_tokens_per_s=round(1.0 / t_ar, 3), speedup_vs_ar_decode=round(new_tok / t_dec * t_ar, 3), cores=cores)


FRONT_END = None  # main(): the InLoopFrontEnd when HF's modules can be built (then every timed specgenerate call includes it)


def vision_tower_leg(tcfg, device, n_img, iters=5):
    """Seconds per image set of the front-end ALONE on the GPU (information: with FRONT_END it is already inside every wall clock of the line;
    without, `speedpy_comparable.with_vision_tower` adds it to both walls).  -> (seconds, description)"""
    fe, what, pixels = (FRONT_END.fe, FRONT_END.what, FRONT_END.pixels) if FRONT_END is not None else build_front_end(MODEL, tcfg, device, n_img)
    pix, sizes = pixels(0)
    grids = None
    if MODEL.startswith("qwen"):
        grids = torch.tensor([(1, 32, 32)] * 4 if MODEL == "qwen7b" else [(1, 68, 92)], device=device)
    call = lambda: fe.features(pix, image_sizes=sizes, image_grid_thw=grids)
    for _ in range(2):
        f = call()
    if f.shape[0] != n_img:
        raise ValueError(f"vision front-end produced {f.shape[0]} tokens, the request has {n_img}")
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(iters):
        call()
    torch.cuda.synchronize()
    return (time.time() - t0) / iters, what


def dominant_kernel_on_all_lanes(sms, streams, tcfg, CO, fp8, device, iters=24):
    """The dominant kernel the way the timed configuration runs it: gate|up + SwiGLU for CO requests, launched on EVERY lane's stream at once
    through the library's own cohort GEMM entry (vispec_gemm_cohort, the launch shape of the timed region), each launch on another layer's
    weights so that they stream from HBM.  The `roofline` object above times this kernel ALONE on the GPU, where the multi-lane launch shape
    (fewer, larger workgroups) fills a third of the CUs by design; here all lanes' launches share the chip as they do in the timed region:
    achieved = (launches x weight bytes) / wall time, HIP events on the launching streams."""
    import ctypes as C
    from vispec_amd import lib as L
    lib = L.load()
    R = len(sms)
    D, I = tcfg.hidden_size, tcfg.intermediate_size
    tw = sms[0].engine.tw
    layers = tw.packed8 if fp8 else tw.packed
    X = [torch.randn(32 * CO, D, device=device, dtype=torch.bfloat16) for _ in range(R)]
    Y = [torch.empty(32 * CO, I, device=device, dtype=torch.bfloat16) for _ in range(R)]
    p = lambda t: C.c_void_p(t.data_ptr())

    def launch(lane, it):
        li = (it * R + lane) % len(layers)
        sc = tw.scales8[li]["wgu"] if fp8 else None
        L.check(lib.vispec_gemm_cohort(sms[lane].engine.h, C.c_void_p(streams[lane].cuda_stream), p(X[lane]), D, p(layers[li]["wgu"]), None if sc is None else p(sc),
                                       None, p(Y[lane]), I, None, 0, CO, TREE["total_token"], I, D, 2))

    for it in range(3):
        for lane in range(R):
            launch(lane, it)
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(R)]
    e0.record()
    for st in streams:
        st.wait_event(e0)
    for it in range(iters):
        for lane in range(R):
            launch(lane, it)
    for lane in range(R):
        ends[lane].record(streams[lane])
    torch.cuda.synchronize()
    wall_ms = max(e0.elapsed_time(e) for e in ends)
    nbytes = 2 * I * D * (1 if fp8 else 2)
    ach = iters * R * nbytes / (wall_ms * 1e-3) / 1e9
    a8_note = (" — NOTE: this model's timed region runs the W8A8 instantiation (e4m3 activations + its quantisation pass); this leg launches the W8A16 "
               "kernel on the same weights (bf16 activations): not the timed region's kernel") if MODEL.endswith("fp8a8") else ""
    return dict(what=f"gate|up + SwiGLU for {CO} requests launched on all {R} lanes' streams at once (vispec_gemm_cohort, the timed region's launch shape; every "
                     f"launch on another layer's weights), {iters} launches per lane" + a8_note, streams=R, launches=iters * R,
                us_per_launch_per_stream=round(1e3 * wall_ms / iters, 2), achieved=round(ach, 1), unit="GB/s", frac=round(ach / 8000.0, 4))


def prefill_gemm_mode():
    """Which library kernels ran the prefill GEMMs: "recorded" = the committed TunableOp table matched this PyTorch / ROCm / GPU; anything else
    names why the libraries' defaults ran (+10 % prefill time, measured in round 4)."""
    from vispec_amd.model.target import prefill_gemm_selection
    return prefill_gemm_selection()


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, returned, suffix=""):
    """--dump-outputs: the (input_ids, new_token, idx, acceptance_len) tuples specgenerate returned to the requests of the last timed step, one
    row per request in request-id order, as float64 .npy files (ids and lengths are exact in float64); ragged rows are padded with -1.  Rows
    beyond DUMP_MAX_BYTES in all are dropped to a fixed seeded sample of requests."""
    rid = sorted(returned)
    seqs = [returned[i][0][0].cpu().numpy() for i in rid]
    accs = [returned[i][3] for i in rid]
    width = max((len(s) for s in seqs), default=0) + max((len(a) for a in accs), default=0) + 3
    keep_n = max(1, DUMP_MAX_BYTES // (8 * width))
    rows = range(len(rid)) if len(rid) <= keep_n else sorted(np.random.default_rng(0).choice(len(rid), keep_n, replace=False))

    def padded(xs):
        a = np.full((len(rows), max((len(xs[r]) for r in rows), default=1)), -1.0)
        for j, r in enumerate(rows):
            a[j, :len(xs[r])] = xs[r]
        return a

    arrays = {"request_ids": np.array([rid[r] for r in rows], dtype=np.float64), "output_ids": padded(seqs),
              "new_token": np.array([returned[rid[r]][1] for r in rows], dtype=np.float64),
              "idx": np.array([returned[rid[r]][2] for r in rows], dtype=np.float64), "acceptance_len": padded(accs)}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), a)
    log(f"--dump-outputs: {len(rows)} of {len(rid)} last-step requests -> {out_dir} ({sum(a.nbytes for a in arrays.values()) / 1e6:.2f} MB)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-cpu-config0", action="store_true",
                    help="drop BASELINE configs[0] (one LLaVA-1.5-7B-shaped request, L=643, end to end on the host cores, ~20 s) from the cpu_baseline object")
    ap.add_argument("--cpu-config0", action="store_true", help=argparse.SUPPRESS)  # (round 2-3 spelling: the leg is on by default now)
    ap.add_argument("--no-ar", action="store_true")
    ap.add_argument("--ar-batch1-lanes", action="store_true",
                    help="also time R lanes of batch-1 AR requests (one request per weight pass): information only, never the denominator of speedup_vs_ar")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--model", default="llava7b", choices=sorted(set(MODELS) | set(CLI_MODEL_ALIASES)),
                    help="BASELINE config; `qwen7b-fp8` (config 5, 'CDNA4 fp8 MFMA') = fp8 weights AND activations (W8A8, = qwen7b-fp8a8); "
                         "`qwen7b-fp8-w8a16` = fp8 weights with bf16 activations")
    ap.add_argument("--n-img", type=int, default=0, help="image tokens per request of the llava workloads (default 2144; SURVEY §8d also names 2928)")
    ap.add_argument("--temperature", type=float, default=0.0, help="> 0: sampling path (README T=1 rows); 0 = greedy (headline)")
    ap.add_argument("--lanes", type=int, default=0, help="concurrent request lanes (stream + host thread + cohort) per GPU sharing one copy of the weights; "
                                                         "0 = 4 (3 for llava13b: 32 request slots of its 6.7 GB KV caches do not fit 288 GB next to the weights)")
    ap.add_argument("--cohort", type=int, default=8, choices=(1, 2, 3, 4, 5, 6, 7, 8),
                    help="requests per lane that run their rounds in lockstep on ONE weight pass (n = every GEMM of a round serves n "
                         "independent batch-1 requests; up to 4: the tokens of each request are bit for bit those of a run on its own; 5..8: the "
                         "cohort-8 summation order — independent of what shares the pass, but not bit-identical to a solo run)")
    ap.add_argument("--wide-row-blocks", type=int, default=-1, choices=(-1, 0, 2, 3, 4, 8, 84),
                    help="weight row blocks per workgroup of a 3-4 request cohort's GEMMs (vispec_set_wide_row_blocks); -1 = 0 with one lane, "
                         "84 (eight for bf16 weights and W8A8, four for W8A16) with several")
    ap.add_argument("--no-vision-in-loop", action="store_true",
                    help="start every request from its projected image features (rounds 1-4) instead of running the HF vision front-end inside the timed "
                         "specgenerate call")
    ap.add_argument("--no-refill", action="store_true",
                    help="run a lane's requests cohort by cohort (every cohort waits for its slowest request) instead of refilling a finished "
                         "request's slot at once (continuous batching, the default)")
    ap.add_argument("--max-new-tokens", type=int, default=512,
                    help="experiments only (what the prompt prefill costs the line): the BASELINE workload is 512 new tokens per request")
    ap.add_argument("--requests", type=int, default=0,
                    help="BASELINE config 4 mode: a step = this many independent (image, prompt) requests sharded round-robin over the "
                         "replicas (request i -> GPU i mod N, then over that GPU's lanes); 0 = one request per lane per step (weak scaling)")
    ap.add_argument("--weights-dir", default=None, help="directory holding the published checkpoints under their hub names (default: $VISPEC_WEIGHTS)")
    ap.add_argument("--base-model-path", default=None, help="target checkpoint directory (the reference harness's flag)")
    ap.add_argument("--spec-model-path", default=None, help="ViSpec draft checkpoint directory (the reference harness's flag)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step's requests returned (token ids, new-token counts, last round "
                         "index, accept lengths) as DIR/<name>.npy (float64), for output-for-output comparison of two builds")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    global MODEL, N_IMG, WIDE_RB, REFILL, MAX_NEW, REAL_WEIGHTS
    MAX_NEW = args.max_new_tokens
    REFILL = not args.no_refill
    MODEL = CLI_MODEL_ALIASES.get(args.model, args.model)
    WIDE_RB = args.wide_row_blocks
    if args.n_img:
        N_IMG = args.n_img
        for k in ("llava7b", "llava13b"):
            MODELS[k]["desc"] = f"1 image ({N_IMG} image tokens) + 512 text + 48 template tokens per request (L={N_PRE + N_IMG + N_POST})"
    REAL_WEIGHTS = resolve_weights(args)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        self_launch(args.gpus, __file__)  # does not return
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    if os.environ.get("VISPEC_FORCE_DEVICE"):  # dry run of the N > 1 control flow on a 1-GPU box
        local = int(os.environ["VISPEC_FORCE_DEVICE"])
    if world != args.gpus:
        log(f"error: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks; refusing to print a line whose n_gpus is not the job's")
        sys.exit(2)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    affinity = pin_to_gpu_numa_node(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("VISPEC_DIST_BACKEND", "nccl")  # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    R = args.lanes if args.lanes > 0 else (3 if MODEL == "llava13b" and args.cohort > 6 else 4)
    fp8 = "fp8" in MODEL
    CO = args.cohort
    t_start = time.time()
    sms, tcfg, t_rep = build_models(device, args.seed, rank, world, R, CO)
    torch.cuda.synchronize()
    t_build = time.time() - t_start  # weight synthesis (or checkpoint load) + W32 packing + replication + contexts / KV caches of every lane
    pairs = sms if CO >= 2 else None
    global FRONT_END
    vision_note = "not in the timed region (--no-vision-in-loop): the requests start from projected image features resident in HBM"
    if not args.no_vision_in_loop:
        try:  # the vision front-end inside every timed specgenerate call, like the reference harness's wall clock (gen_spec_answer_coco_caption.py:221-232)
            n_img_model = {"qwen7b": 1024, "qwen7b-hires": 1564, "qwen7b-fp8": 1564, "qwen7b-fp8a8": 1564}.get(MODEL, N_IMG)
            FRONT_END = InLoopFrontEnd(*build_front_end(MODEL, tcfg, device, n_img_model))
            for grp in (sms if CO >= 2 else [[m] for m in sms]):
                for m in grp:
                    m.base_model.vision = FRONT_END
            vision_note = "IN the timed region, once per request: " + FRONT_END.what + "; its output enters as 0 x (the embeddings are the request's synthetic features)"
        except Exception as e:
            FRONT_END = None
            vision_note = f"not in the timed region (HF vision modules could not be built: {type(e).__name__}: {e})"[:300]
    sms = [p[0] for p in sms] if CO >= 2 else sms  # the leaders double as the single-request models of the annotation legs
    sm = sms[0]
    eng = sm.engine
    K, W = args.steps, args.warmup
    streams = [torch.cuda.Stream(device) for _ in range(R)]
    from vispec_amd import parallel
    from vispec_amd.model.spec_model_ours import baseline_generate_cohort, specgenerate_cohort, specgenerate_stream
    plan, scaling = request_plan(args.requests, rank, world, R, CO, W + K)
    req_cache = {}

    def get_req(i):
        if i not in req_cache:
            req_cache[i] = make_request(tcfg, i, device)
        return req_cache[i]

    for lane in range(R):  # every request tensor is resident in HBM before the timed region
        for step in plan[lane]:
            for i in step:
                get_req(i)
    torch.cuda.synchronize()

    lock = [0] * R  # lockstep rounds a lane executed in continuous-batching mode (slot utilisation = request-rounds / (CO x this))
    # --dump-outputs: what the requests of the last timed step returned, by request id (references only: every returned tensor is a fresh one)
    last_step = {i for lane in plan for i in lane[W + K - 1]} if args.dump_outputs else set()
    returned = {}

    def keep(i, o, new_token, idx, acc):
        if i in last_step:
            returned[i] = (o, int(new_token), int(idx), list(acc))

    def lane_fn(lane, lo_, hi, ar=False, ar_new=None):
        ar_new = MAX_NEW if ar_new is None else ar_new  # (the AR legs' graph-capturing pre-run decodes a few tokens only)

        def f():
            lo = lo_
            tok = rnd = 0
            accs = []
            t_lane = time.time()
            torch.cuda.set_device(device)  # HIP's current device is per host thread; a new thread starts on device 0
            with torch.cuda.stream(streams[lane]):
                if REFILL and CO >= 2 and not ar and sum(len(plan[lane][s_]) for s_ in range(lo, hi)) > CO:
                    # continuous batching over the lane's CO request slots: the moment a request finishes, its slot takes the lane's next one
                    mine = [i for s_ in range(lo, hi) for i in plan[lane][s_]]
                    st_s = {}
                    outs = specgenerate_stream(pairs[lane], [get_req(i) for i in mine], max_new_tokens=MAX_NEW, temperature=args.temperature,
                                               seeds=mine, stats=st_s)
                    for i, (o, new_token, idx, acc) in zip(mine, outs):
                        tok += int(new_token)
                        rnd += idx + 1
                        accs += acc
                        keep(i, o, new_token, idx, acc)
                    lock[lane] += st_s["rounds"]
                    lo = hi  # nothing left for the step-by-step loop below
                for s_ in range(lo, hi):
                    todo = list(plan[lane][s_])
                    while CO >= 2 and not ar and len(todo) >= 2:  # up to CO requests per weight pass
                        now, todo = todo[:CO], todo[CO:]
                        outs = specgenerate_cohort(pairs[lane][:len(now)], [get_req(i) for i in now], max_new_tokens=MAX_NEW,
                                                   temperature=args.temperature, seeds=now)
                        for i, (o, new_token, idx, acc) in zip(now, outs):
                            tok += int(new_token)
                            rnd += idx + 1
                            accs += acc
                            keep(i, o, new_token, idx, acc)
                    while CO >= 2 and ar == "cohort" and len(todo) >= 2:  # the AR baseline at the same batching: CO requests per weight pass
                        now, todo = todo[:CO], todo[CO:]
                        outs = baseline_generate_cohort(pairs[lane][:len(now)], [get_req(i) for i in now], max_new_tokens=ar_new, max_steps=ar_new + 1)
                        for o, i in zip(outs, now):
                            tok += o.shape[1] - get_req(i)[0].shape[1]
                    for i in todo:
                        ids, pix = get_req(i)
                        if ar:
                            o = sms[lane].baseline_generate(ids, max_new_tokens=ar_new, max_steps=ar_new + 1, **pix)
                            tok += o.shape[1] - ids.shape[1]
                        else:
                            o, new_token, idx, acc = sms[lane].specgenerate(ids, max_new_tokens=MAX_NEW, log=True, return_acceptance_len=True,
                                                                            temperature=args.temperature, seed=i, **pix)
                            tok += int(new_token)
                            rnd += idx + 1
                            accs += acc
                            keep(i, o, new_token, idx, acc)
                streams[lane].synchronize()
            if os.environ.get("VISPEC_BENCH_DEBUG"):
                log(f"[rank {rank} lane {lane}] steps {lo_}..{hi}: {time.time() - t_lane:.2f} s, {tok} tokens, {rnd} rounds")
            return tok, rnd, accs
        return f

    t_w0 = time.time()
    run_lanes([lane_fn(l, 0, W) for l in range(R)])
    t_warm = time.time() - t_w0  # the W warm-up steps: every hipGraph of the timed region is captured here, the TunableOp table is read
    startup = dict(build_models_s=round(t_build, 2), weight_replication_s=round(t_rep, 2), warmup_steps_s=round(t_warm, 2),
                   note="per rank, before the timed region: weight synthesis / load + W32 packing + contexts and KV caches; then the warm-up steps (graph capture)")
    log(f"[rank {rank}] start-up: build_models {t_build:.1f} s (replication {t_rep:.1f} s), {W} warm-up step(s) {t_warm:.1f} s")
    lock[:] = [0] * R
    barrier()
    cpu0, _ = host_usage()
    t0 = time.time()
    res = run_lanes([lane_fn(l, W, W + K) for l in range(R)])
    barrier()
    dt = time.time() - t0
    cpu1, rss_gb = host_usage()
    if os.environ.get("VISPEC_BENCH_MARK") and rank == 0:  # tools/mem_activity.py: wall-clock bounds of the timed region (epoch seconds)
        with open(os.environ["VISPEC_BENCH_MARK"], "w") as f:
            json.dump(dict(t0=t0, t1=t0 + dt), f)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, returned, "" if world == 1 else f"_rank{rank}")
    host_cpu_s, rank_wall_s = cpu1 - cpu0, dt  # what this rank's host side cost during the timed region (lane threads + launches + event waits)
    tokens = sum(r[0] for r in res)
    rounds = sum(r[1] for r in res)
    accs = [a for r in res for a in r[2]]
    if os.environ.get("VISPEC_BENCH_RANKLOG"):  # what THIS rank did (tools/dryrun_world2.sh, tests/test_world2_gpu.py check the N > 1 control flow with it)
        os.makedirs(os.environ["VISPEC_BENCH_RANKLOG"], exist_ok=True)
        ck = parallel.checksum(list(eng.tw.tensors()) + list(eng.dw.tensors()))
        with open(os.path.join(os.environ["VISPEC_BENCH_RANKLOG"], f"rank{rank}.json"), "w") as f:
            json.dump(dict(rank=rank, world=world, device=str(device), weights_checksum=int(ck.item()), replicate_s=round(t_rep, 3),
                           replicate_mode=os.environ.get("VISPEC_REPLICATE", "broadcast"),
                           backend=None if dist is None else dist.get_backend(), timed_request_ids=sorted(i for lane in plan for st_ in lane[W:W + K] for i in st_),
                           warmup_request_ids=sorted(i for lane in plan for st_ in lane[:W] for i in st_), tokens=int(tokens), rounds=int(rounds),
                           wall_s=round(dt, 4), host_cpu_s=round(host_cpu_s, 3), host_cpu_per_wall=round(host_cpu_s / dt, 3), peak_rss_GB=round(rss_gb, 2),
                           affinity=affinity, lanes=R, startup=startup), f)
    stats = torch.tensor([dt, tokens, rounds, sum(accs)], dtype=torch.float64, device=device)
    host_mx = torch.tensor([host_cpu_s / rank_wall_s, rss_gb], dtype=torch.float64, device=device)
    if dist is not None:
        dist.all_reduce(host_mx, op=dist.ReduceOp.MAX)
    if dist is not None:
        mx = stats.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        sm_ = stats.clone()
        dist.all_reduce(sm_, op=dist.ReduceOp.SUM)
        dt, tokens, rounds, acc_sum = float(mx[0]), float(sm_[1]), float(sm_[2]), float(sm_[3])
    else:
        acc_sum = float(sum(accs))
    value = tokens / dt
    if dist is not None:
        # The job's measurement is complete: every rank leaves the process group NOW.  Rank 0's annotation legs below take minutes (single-request
        # roofline legs, the AR baseline at equal batching); ranks 1..N-1 used to sit in a final dist.barrier() under RCCL's watchdog meanwhile.
        dist.barrier()
        dist.destroy_process_group()
        dist = None

    extra = {}
    if rank == 0:
        try:  # the legs below only annotate the line: a failure in one of them must not lose the measured value
            n_img = None
            # ---- the reference's own metric (speed.py:56-97): ONE batch-1 request stream, whole-request wall clock, spec vs AR
            ids, pix = get_req(plan[0][W][0])
            n_img = int((ids == tcfg.image_token_index).sum())
            torch.cuda.synchronize()
            t1 = time.time()
            with torch.cuda.stream(streams[0]):
                out, new_token, idx, acc, t_dec_clean = sm.specgenerate(ids, max_new_tokens=MAX_NEW, log=True, return_acceptance_len=True,
                                                                        return_decode_time=True, temperature=args.temperature, seed=7, **pix)
            torch.cuda.synchronize()
            t_req = time.time() - t1
            st = eng.state()
            n_rounds = idx + 1
            ms_round = 1e3 * t_dec_clean / n_rounds
            n_mid = (ids.shape[1] + st["n_ctx"]) // 2
            m_img = (ids[0] == tcfg.image_token_index).cpu().numpy()
            n_runs = int(m_img[0]) + int(((~m_img[:-1]) & m_img[1:]).sum())  # every image run is compressed to num_q - 1 draft rows
            n_c_mid = n_mid - n_img + n_runs * (eng.num_q - 1)
            b_round = algorithmic_bytes_per_round(tcfg, n_mid, n_c_mid, fp8)
            spc = dict(what="one batch-1 request stream on one GPU, wall clock around the whole specgenerate call (prefill included) — the "
                            "quantity the reference's speed.py divides by its AR counterpart",
                       tokens_per_s=round(int(new_token) / t_req, 2), new_tokens=int(new_token), wall_s=round(t_req, 4),
                       prefill_s=round(t_req - t_dec_clean, 4), decode_s=round(t_dec_clean, 4), rounds=n_rounds,
                       ms_per_round=round(ms_round, 3), tau=round(float(np.mean(acc)), 3),
                       algorithmic_GB_per_round=round(b_round / 1e9, 2),
                       round_GBps=round(b_round / (ms_round * 1e-3) / 1e9, 1),
                       round_roofline_frac_of_8TBps=round(b_round / (ms_round * 1e-3) / 8e12, 4))
            extra["speedpy_comparable"] = spc
            # ---- roofline legs: per-kernel device timestamps around every skinny-GEMM / attention launch (hipExtLaunchKernel events on the
            #      launch stream), (1) of one more single request, (2) with cohorts, of one cohort of the timed region's size: the kernels the
            #      timed region actually runs (each GEMM launch then serves CO requests with ONE pass over the weight)
            def price(rep, n_req):
                """-> (prefill MFMA record, priced kernels, dominant key).  Priced = every launch kind with algorithmic bytes: the GEMMs (the weight
                once per launch, recorded by the library) and the tree attention's partial kernel (K/V rows of its requests once per launch: the
                context length lives on the device, so the mid-request context prices it).  DOMINANT = the kind with the largest TOTAL device time
                (launches x average duration) in this instrumented leg — what a rocprofv3 summary of the same cohort ranks first."""
                pf_ = rep.pop("gemm_prefill_mfma", None)
                priced = {k: dict(v) for k, v in rep.items() if k.startswith("gemm") and v["bytes"] > 0}
                if "attn_partial" in rep:
                    a = dict(rep["attn_partial"])
                    a["bytes"] = a["launches"] * n_req * 2.0 * tcfg.num_kv_heads * tcfg.head_dim * 2 * n_mid
                    priced["attn_partial"] = a
                dom_ = max(priced, key=lambda k: priced[k]["ms"])
                return pf_, priced, dom_

            def flops_of(kind, v, n_req):
                """MFMA work of a priced kind: GEMM = 2 x (32 rows per request tile x requests) x N x K (N x K = weight elements = bytes / element size);
                attention = Q K^T + P V over one 32-row query tile per head: 32 G flops per K/V byte (G = query heads per KV head)."""
                if kind == "attn_partial":
                    return 32.0 * (tcfg.num_heads // tcfg.num_kv_heads) * v["bytes"]
                return 2.0 * 32 * n_req * v["bytes"] / (1 if fp8 else 2)

            def kernel_line(kind, v, n_req):
                t = v["ms"] * 1e-3
                hbm, mf = v["bytes"] / t / 8e12, flops_of(kind, v, n_req) / t / 2.5e15
                return dict(launches=int(v["launches"]), avg_launch_us=round(1e3 * v["ms"] / v["launches"], 2), total_ms=round(v["ms"], 3),
                            GBps=round(v["bytes"] / t / 1e9, 1), frac=round(hbm, 4), mfma_frac=round(mf, 4),
                            cus_occupied=round(min(1.0, v.get("workgroups", 0.0) / v["launches"] / 256.0), 3) if v.get("workgroups") else None)

            def roofline_of(rep, priced, dom_, keys, note, n_req):
                d = priced[dom_]
                line = kernel_line(dom_, d, n_req)
                gemm_ = {k: v for k, v in priced.items() if k.startswith("gemm")}
                all_b = sum(v["bytes"] for v in gemm_.values())
                all_ms = sum(v["ms"] for v in gemm_.values())
                # HBM traffic of that kernel from the PMC pass kept under profiles/ (rocprofv3 --pmc FETCH_SIZE in its own run;
                # FETCH_SIZE is KB and counts half of a wide coalesced stream on gfx950 -> x2, MI355X_MICROARCH.md §HBM)
                traffic = traffic_source = None
                try:
                    import glob  # (one committed pass per model that has one: profiles/rNN_pmc_fetch_size[_<model>].json)
                    pmc_file = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_fetch_size" + ("" if MODEL == "llava7b" else "_" + MODEL.replace("-", ""))
                                                             + ".json")))[-1]
                    pmc = json.load(open(pmc_file))
                    key = keys.get(dom_)
                    for k, v in pmc.items():
                        if key and key in k:
                            traffic = int(2 * 1024 * v["fetch_size_kb_per_launch"])
                            traffic_source = (f"profiles/{os.path.basename(pmc_file)} (a separate `rocprofv3 --pmc FETCH_SIZE` pass of this kernel, committed with "
                                              f"the tree: NOT measured by this run; x2 = the guide's gfx950 correction)")
                except Exception:
                    pass
                # the same kernel as the committed rocprofv3 summary has it (in-graph replay of one cohort-8 / single-request lane: the durations the
                # timed region's launches have; see `timing`): looked up, NOT measured by this run
                in_graph = None
                try:
                    import csv
                    import glob
                    tag = "1lane_cohort8" if n_req >= 5 else ("1lane_cohort1" if n_req == 1 else None)
                    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_kernel_stats_{tag}.csv"))) if tag and MODEL == "llava7b" else []
                    key = keys.get(dom_)
                    if files and key:
                        for row in csv.DictReader(open(files[-1])):
                            if key.replace(", ", ",") in row["Name"].replace(", ", ","):
                                us = float(row["AverageNs"]) / 1e3
                                b_l = d["bytes"] / d["launches"]
                                in_graph = dict(source=f"profiles/{os.path.basename(files[-1])} (rocprofv3 --kernel-trace --stats of `bench.py --lanes 1 --cohort "
                                                       f"{8 if n_req >= 5 else 1}`, committed with the tree)", avg_launch_us=round(us, 2),
                                                hbm_frac=round(b_l / (us * 1e-6) / 8e12, 4),
                                                mfma_frac=round(flops_of(dom_, d, n_req) / d["launches"] / (us * 1e-6) / 2.5e15, 4))
                                break
                except Exception:
                    in_graph = None
                # the roof that binds: the larger of the two fractions.  A cohort GEMM occupies `cus_occupied` of the chip by design (CU-time is
                # what it costs): per occupied CU its matrix pipe is mfma_frac / cus_occupied busy.
                bound = "mfma" if line["mfma_frac"] > line["frac"] else "hbm"
                ach, peak, unit = ((flops_of(dom_, d, n_req) / (d["ms"] * 1e-3) / 1e12, 2500.0, "TFLOP/s") if bound == "mfma"
                                   else (d["bytes"] / (d["ms"] * 1e-3) / 1e9, 8000.0, "GB/s"))
                by_bytes = max(gemm_, key=lambda k: gemm_[k]["bytes"])
                return dict(bound=bound, achieved=round(ach, 1), peak=peak, unit=unit, frac=round(ach / peak, 4),
                            hbm_frac=line["frac"], hbm_GBps=line["GBps"], mfma_frac=line["mfma_frac"], cus_occupied=line["cus_occupied"],
                            mfma_frac_of_occupied_cus=(round(line["mfma_frac"] / line["cus_occupied"], 4) if line["cus_occupied"] else None),
                            traffic=traffic, traffic_source=traffic_source, in_graph=in_graph,
                            kernel=f"{dom_} ({keys.get(dom_, '?')})",
                            dominant_by="largest total device time (launches x average duration) among the priced kernels of this instrumented leg",
                            what=note, launches=int(d["launches"]), avg_launch_us=line["avg_launch_us"],
                            algorithmic_bytes_per_launch=int(d["bytes"] / d["launches"]),
                            timing="device begin/end timestamps of each dispatch (hipExtLaunchKernel events) on the launch stream, launches un-graphed "
                                   "(an event pair per launch needs the direct path): the GPU idles between them, and the same kernels replayed back to "
                                   "back from the hipGraph of the timed region measure 6-14 % longer in the rocprofv3 summaries under profiles/ "
                                   "(c8 q|k|v 95.0 vs 87.1 us, gate|up 81.4 vs 76.8, split-K partials 44.4 vs 38.8: profiles/r06_kernel_stats_1lane_cohort8.csv)",
                            all_gemm_GBps=round(all_b / (all_ms * 1e-3) / 1e9, 1),
                            largest_bytes_gemm=dict(kernel=f"{by_bytes} ({keys.get(by_bytes, '?')})", **kernel_line(by_bytes, gemm_[by_bytes], n_req)),
                            by_kernel={k: kernel_line(k, v, n_req) for k, v in priced.items()})

            torch.cuda.synchronize()
            eng.prof_enable(True)
            out_p, new_token_p, idx_p, acc_p, t_dec = sm.specgenerate(ids, max_new_tokens=MAX_NEW, log=True, return_acceptance_len=True,
                                                                      return_decode_time=True, temperature=args.temperature, seed=7, **pix)
            rep = eng.prof_report()
            eng.prof_enable(False)
            # the draft prefill's big-M GEMM is MFMA-bound: the library records its FLOPs, reported on their own below
            pf, gemm, dom = price(rep, 1)
            single_roof = roofline_of(rep, gemm, dom, PROF_KERNEL_KEYS, "one request per launch (the instrumented single-request leg)", 1)
            if pf:
                single_roof["prefill_gemm_mfma"] = dict(launches=int(pf["launches"]), avg_launch_us=round(1e3 * pf["ms"] / pf["launches"], 2),
                                                        TFLOPs=round(pf["bytes"] / (pf["ms"] * 1e-3) / 1e12, 1), peak=2500.0,
                                                        frac=round(pf["bytes"] / (pf["ms"] * 1e-3) / 2.5e15, 4),
                                                        note="draft prefill (image K/V projection, text fusion GEMMs): once per request, outside the round loop")
            if CO >= 2:
                now = list(plan[0][W])[:CO]
                st_c = {}
                eng.prof_enable(True)
                with torch.cuda.stream(streams[0]):
                    specgenerate_cohort(pairs[0][:len(now)], [get_req(i) for i in now], max_new_tokens=MAX_NEW, temperature=args.temperature,
                                        seeds=now, stats=st_c)
                rep_c = eng.prof_report()
                eng.prof_enable(False)
                rep_c.pop("gemm_prefill_mfma", None)
                _, gemm_c, dom_c = price(rep_c, len(now))
                rb_timed = WIDE_RB if WIDE_RB >= 0 else (0 if R == 1 else 84)
                wide8 = 3 <= CO <= 4 and (rb_timed == 8 or (rb_timed == 84 and (not fp8 or "a8" in MODEL)))  # (vispec_set_wide_row_blocks(84): W8A16 stays on four)
                keys_c = PROF_KERNEL_KEYS_C8 if CO >= 5 else ((PROF_KERNEL_KEYS_WIDE8 if wide8 else PROF_KERNEL_KEYS_WIDE) if CO >= 3 else PROF_KERNEL_KEYS_PAIRED)
                extra["roofline"] = roofline_of(rep_c, gemm_c, dom_c, keys_c,
                                                f"{CO} requests per launch (one cohort of the timed region, un-graphed for the timestamps, ALONE on the GPU): "
                                                f"algorithmic bytes = the weight once, whatever the number of requests it serves"
                                                + ("; the launch shape is the multi-lane one (eight weight row blocks per workgroup: half the workgroups, half "
                                                   "the activation traffic) — alone it fills about a third of the CUs, each at the CU's ingest cap; `deployed` "
                                                   "times the same kernel the way the timed region runs it" if wide8 else ""), len(now))
                extra["roofline"]["cohort_round_ms_instrumented"] = round(1e3 * st_c["decode_s"] / st_c["rounds"], 3)
                # one launch serves CO requests with ONE pass over the weight: `achieved` counts those bytes once (the roofline the kernel is held to);
                # what the CO requests would have streamed one by one is CO times that — the figure to compare across cohort sizes
                extra["roofline"]["requests_per_launch"] = CO
                extra["roofline"]["weight_bytes_delivered_to_requests_GBps"] = round(CO * extra["roofline"]["largest_bytes_gemm"]["GBps"], 1)  # (of the gate|up launch)
                extra["roofline"]["wide_row_blocks"] = rb_timed
                if CO >= 3 and R >= 2:
                    try:
                        extra["roofline"]["deployed"] = dominant_kernel_on_all_lanes(sms, streams, tcfg, CO, fp8, device)
                    except Exception as e:
                        extra["roofline"]["deployed"] = f"not measured: {type(e).__name__}: {e}"[:200]
                if 3 <= CO <= 4 and rb_timed != 0:
                    # The instrumented cohort runs ALONE on the GPU with the launch shapes of the timed configuration, which are chosen for R lanes
                    # sharing the GPU (fewer, larger workgroups: a launch costs CU-time in proportion to the bytes it ingests).  The same cohort with
                    # the shapes a single lane would pick (vispec_set_wide_row_blocks(0)) shows what each kernel does when it has the GPU to itself.
                    eng.set_wide_row_blocks(0)
                    try:
                        eng.prof_enable(True)
                        st_1 = {}
                        with torch.cuda.stream(streams[0]):
                            specgenerate_cohort(pairs[0][:len(now)], [get_req(i) for i in now], max_new_tokens=min(MAX_NEW, 128), temperature=args.temperature,
                                                seeds=now, stats=st_1)
                        rep_1 = eng.prof_report()
                        eng.prof_enable(False)
                        rep_1.pop("gemm_prefill_mfma", None)
                        extra["roofline"]["by_kernel_single_lane_shapes"] = dict(
                            note="the same instrumented cohort with the launch shapes of ONE lane per GPU (--wide-row-blocks 0): not the timed configuration",
                            cohort_round_ms=round(1e3 * st_1["decode_s"] / st_1["rounds"], 3),
                            **{k: dict(avg_launch_us=round(1e3 * v["ms"] / v["launches"], 2), GBps=round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1),
                                       frac=round(v["bytes"] / (v["ms"] * 1e-3) / 8e12, 4)) for k, v in rep_1.items() if v["bytes"] > 0 and k.startswith("gemm")})
                    finally:
                        eng.prof_enable(False)
                        eng.set_wide_row_blocks(rb_timed)
                extra["roofline_single_request"] = single_roof
            else:
                extra["roofline"] = single_roof
            extra["round"] = dict(rounds_per_s=round(rounds / dt, 2), kernel_ms_per_round={k: round(v["ms"] / (idx_p + 1), 4) for k, v in rep.items()},
                                  note="kernel_ms_per_round comes from the instrumented (un-graphed) request and only splits the round by kernel; "
                                       "the round's own time and roofline fraction are speedpy_comparable.ms_per_round / round_roofline_frac_of_8TBps")
            # aggregate over all lanes: the lanes share ONE copy of the weights but each streams it on its own
            # (with a cohort the weight bytes of a round are SHARED by its two requests: bytes per request-round = weights / 2 + its own KV)
            b_kv = b_round - algorithmic_bytes_per_round(tcfg, 0, 0, fp8)
            b_req_round = (b_round - b_kv) / CO + b_kv
            extra["aggregate"] = dict(lanes=R, cohort=CO, request_rounds_per_s_per_gpu=round(rounds / world / dt, 2),
                                      algorithmic_GB_per_request_round=round(b_req_round / 1e9, 2),
                                      streamed_GBps_per_gpu=round(b_req_round * rounds / world / dt / 1e9, 1),
                                      frac_of_8TBps=round(b_req_round * rounds / world / dt / 8e12, 4))
            if isinstance(extra.get("roofline"), dict):  # the line's roofline object also describes the TIMED REGION, not only one kernel alone
                extra["roofline"].update(
                    achieved_region=extra["aggregate"]["streamed_GBps_per_gpu"], frac_region=extra["aggregate"]["frac_of_8TBps"],
                    request_rounds_per_s_per_gpu=extra["aggregate"]["request_rounds_per_s_per_gpu"],
                    region_note="achieved_region / frac_region = algorithmic bytes of the whole timed region (weights / cohort + own KV per request-round) "
                                "per second per GPU over 8 TB/s; `achieved` / `frac` above = the dominant kernel (largest total device time) of one cohort ALONE on "
                                "the GPU, on the roof that binds it (`bound`); `hbm_frac` / `mfma_frac` = both of its fractions")
                bk = extra["roofline"].get("by_kernel", {})
                tot = {k: v["launches"] * v["avg_launch_us"] for k, v in bk.items() if k.startswith("gemm")}
                if tot:
                    kmax = max(tot, key=tot.get)
                    extra["roofline"]["largest_total_time_gemm"] = dict(kernel=kmax, share_of_gemm_time=round(tot[kmax] / sum(tot.values()), 3), **bk[kmax])
            if sum(lock):  # continuous batching: share of the (lockstep round x slot) grid that carried a live request (rank 0's lanes)
                extra["aggregate"]["slot_utilisation"] = round(sum(r[1] for r in res) / (CO * sum(lock)), 4)
            # ---- AR baseline legs (gen_baseline_answer_coco_caption.py): same requests, same kernels at T=1, whole-request wall time;
            #      once on a single lane (latency) and once with the same lane concurrency as the timed region (throughput)
            if not args.no_ar:
                torch.cuda.synchronize()
                t1 = time.time()
                with torch.cuda.stream(streams[0]):
                    ar = sm.baseline_generate(ids, inputs_embeds=None, max_new_tokens=MAX_NEW, max_steps=MAX_NEW + 1, **pix)
                torch.cuda.synchronize()
                t_ar = time.time() - t1
                n_ar = ar.shape[1] - ids.shape[1]
                b_ar = algorithmic_bytes_per_ar_step(tcfg, n_mid, fp8)
                spc.update(ar_tokens_per_s=round(n_ar / t_ar, 2), speedup_vs_ar=round(spc["tokens_per_s"] / (n_ar / t_ar), 3),
                           published_speedup=None, ar_roofline_frac_of_8TBps=round(b_ar * (n_ar / t_ar) / 8e12, 4))
                try:  # the reference's wall clock also holds the vision tower, in both runs (see vision_tower_leg)
                    t_vis, vis_what = vision_tower_leg(tcfg, device, n_img)
                    if FRONT_END is not None:  # already inside t_req and t_ar (and inside every request of the timed region)
                        spc["with_vision_tower"] = dict(vision_s=round(t_vis, 4), front_end=vis_what, in_the_walls_above=True,
                                                        tokens_per_s=spc["tokens_per_s"], ar_tokens_per_s=spc["ar_tokens_per_s"], speedup_vs_ar=spc["speedup_vs_ar"])
                    else:
                        spc["with_vision_tower"] = dict(vision_s=round(t_vis, 4), front_end=vis_what, in_the_walls_above=False,
                                                        tokens_per_s=round(int(new_token) / (t_req + t_vis), 2), ar_tokens_per_s=round(n_ar / (t_ar + t_vis), 2),
                                                        speedup_vs_ar=round((int(new_token) / (t_req + t_vis)) / (n_ar / (t_ar + t_vis)), 3))
                except Exception as e:
                    spc["with_vision_tower"] = f"not measured: {type(e).__name__}: {e}"[:200]
                # greedy invariance at full size: speculative tokens == AR tokens of the same target
                if args.temperature <= 1e-5:
                    nmin = min(ar.shape[1], out.shape[1])
                    extra["spec_equals_ar_prefix"] = int((ar[0, :nmin] == out[0, :nmin]).long().cumprod(0).sum().item()) - ids.shape[1]
                # the speed-up of the LINE divides like by like (speed.py:56-97): the same lanes x cohorts, the requests of one timed step,
                # decoded autoregressively with CO requests per weight pass (vispec_cohortn_ar_step)
                def ar_leg(mode, ar_new=None):
                    torch.cuda.synchronize()
                    t1_ = time.time()
                    res_ = run_lanes([lane_fn(l, W, W + 1, ar=mode, ar_new=ar_new) for l in range(R)])
                    torch.cuda.synchronize()
                    dt_ = time.time() - t1_
                    n_ = sum(r[0] for r in res_)
                    return n_ / dt_, n_, dt_
                if CO >= 2:
                    ar_leg("cohort", ar_new=24)  # (captures the AR cohort graphs outside the timed leg: a few steps are enough)
                    ar_rate, ar_n, ar_dt = ar_leg("cohort")
                    extra["ar_baseline"] = dict(tokens_per_s=round(ar_rate, 2), lanes=R, cohort=CO, new_tokens=int(ar_n), wall_s=round(ar_dt, 3),
                                                what=f"greedy AR of the same requests at the SAME batching as the timed region: {R} lanes x {CO} requests per weight pass")
                    extra["speedup_vs_ar"] = round((tokens / world / dt) / ar_rate, 3)
                    if args.ar_batch1_lanes:  # (off by default since round 6: 26 s of a leg that is not the denominator of any figure of the line)
                        b1_rate, b1_n, b1_dt = ar_leg(True)
                        extra["ar_baseline_batch1_lanes"] = dict(
                            tokens_per_s=round(b1_rate, 2), lanes=R, cohort=1, new_tokens=int(b1_n), wall_s=round(b1_dt, 3),
                            what=f"{R} lanes of batch-1 AR requests (one request per weight pass): NOT the denominator of speedup_vs_ar — against it the "
                                 f"line is {round((tokens / world / dt) / b1_rate, 3)}x, most of which is batching, not speculation")
                else:
                    ar_rate, ar_n, ar_dt = ar_leg(True)
                    extra["ar_baseline"] = dict(tokens_per_s=round(ar_rate, 2), lanes=R, cohort=1, new_tokens=int(ar_n), wall_s=round(ar_dt, 3))
                    extra["speedup_vs_ar"] = round((tokens / world / dt) / ar_rate, 3)
        except Exception as e:
            extra["extra_legs_error"] = f"{type(e).__name__}: {e}"[:300]
            try:
                eng.prof_enable(False)
            except Exception:
                pass
        if world == 1 and not args.no_cpu_baseline:
            try:
                host = cpu_models(sm, tcfg)
                extra["cpu_baseline"] = cpu_baseline_leg(sm, tcfg, get_req(plan[0][W][0]), host)
            except Exception as e:  # never lose the GPU line to the CPU leg
                host = f"failed: {type(e).__name__}: {e}"[:300]
                extra["cpu_baseline"] = dict(value=None, unit="tokens/s", cores=os.cpu_count(), kind="port", sample=host)
            if not args.no_cpu_config0 and MODEL == "llava7b" and not REAL_WEIGHTS:  # BASELINE configs[0]: LLaVA-1.5-7B shares LLaVA-v1.6-7B's dimensions
                try:
                    extra["cpu_baseline"]["config0_end_to_end"] = cpu_config0_leg(sm, tcfg, host)
                except Exception as e:
                    extra["cpu_baseline"]["config0_end_to_end"] = f"failed: {type(e).__name__}: {e}"[:300]
        per_step = (f"{args.requests} independent requests sharded round-robin over the {world} replica(s) and their lanes" if args.requests
                    else f"{CO} request{'s' if CO > 1 else ''} on each of {R} concurrent lanes per GPU")
        if CO >= 2:
            per_step += (f" (every lane runs its {CO} batch-1 requests in lockstep on one weight pass: each GEMM of a round is launched once "
                         f"for all of them" + ("; a lane keeps its request slots full — the slot of a finished request takes the lane's next "
                                               "request at once (continuous batching over the K steps' requests)" if REFILL and K * CO > CO else "") + ")")
        line = {
            "metric": f"accepted output tokens/sec (ViSpec speculative decoding, {MODELS[MODEL]['name']} + ViSpec draft, T={args.temperature:g})",
            "value": round(value, 2), "unit": "tokens/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": round(1e3 * dt / K, 2), "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "fp8-w8a8" if MODEL.endswith("fp8a8") else ("fp8-w8a16" if fp8 else "bf16"), "data": "synthetic",
            "config": {"workload": f"{MODELS[MODEL]['name']}-shaped target + ViSpec draft, {MODELS[MODEL]['desc']}, "
                                   f"max_new_tokens={MAX_NEW}, temperature={args.temperature:g}, total_token=30 depth=3 top_k=8 num_q=2; "
                                   f"a step = {per_step} (replicas share one weight copy per GPU)",
                       "weights": (f"real checkpoints: {REAL_WEIGHTS[0]} + {REAL_WEIGHTS[1]} (SpecModel.from_pretrained); prompts and image features "
                                   f"are synthetic, so tau is what these weights accept on random prompts (published on COCO captions etc.: {TAU_PUBLISHED[MODEL]})"
                                   if REAL_WEIGHTS else
                                   f"synthetic: N(0,0.02) layers + successor-structured embed/lm_head (rho={RHO[MODEL]}: measured tau vs the "
                                   f"reference's published {TAU_PUBLISHED[MODEL]} for this model, README T=0 average)"),
                       "parallelism": f"dp{world} x {R} lanes/GPU x cohort {CO} (independent requests, one-time RCCL weight replication {t_rep:.2f}s)",
                       "prefill_gemms": prefill_gemm_mode(), "vision_front_end": vision_note},
            # what one rank costs the HOST during the timed region (max over ranks): R lane threads issuing one hipGraph launch per phase and one
            # event wait per round.  host_cpu_per_wall = busy host cores per rank; x 8 ranks must stay well below the node's cores.
            "host": {"cpu_s_per_wall_s": round(float(host_mx[0]), 3), "rank0_cpu_s": round(host_cpu_s, 2), "rank0_wall_s": round(rank_wall_s, 3),
                     "peak_rss_GB": round(float(host_mx[1]), 2), "lane_threads": R, "host_cores": os.cpu_count(), "affinity": affinity},
            "mean_accept_length_tau": round(acc_sum / max(1.0, rounds), 3), "tokens_per_round": round(tokens / max(1.0, rounds), 3),
        }
        line["startup"] = startup
        line.update(extra)
        print(json.dumps(line), flush=True)


# library profiling kinds -> the kernel instantiation they time (names as they appear in the rocprofv3 summaries under profiles/)
PROF_KERNEL_KEYS_WIDE = {"gemm_none": "gemm_w32_wide_kernel<0,", "gemm_residual": "gemm_w32_wide_kernel<1,", "gemm_swiglu": "gemm_w32_wide_kernel<2,",
                         "gemm_splitk_partial": "gemm_w32_wide_kernel<3,", "gemm_qkv_rope": "gemm_w32_wide_kernel<4,",
                         "attn_partial": "tree_attn2_partial_kernel", "attn_reduce": "tree_attn_reduce_kernel"}
PROF_KERNEL_KEYS_WIDE8 = {"gemm_none": "gemm_w32_wide8_kernel<0,", "gemm_residual": "gemm_w32_wide8_kernel<1,", "gemm_swiglu": "gemm_w32_wide8_kernel<2,",
                          "gemm_splitk_partial": "gemm_w32_wide8_kernel<3,", "gemm_qkv_rope": "gemm_w32_wide8_kernel<4,",
                          "attn_partial": "tree_attn2_partial_kernel", "attn_reduce": "tree_attn_reduce_kernel"}
PROF_KERNEL_KEYS_C8 = {"gemm_none": "gemm_w32_c8_kernel<0,", "gemm_residual": "gemm_w32_c8_kernel<1,", "gemm_swiglu": "gemm_w32_c8_kernel<2,",
                       "gemm_splitk_partial": "gemm_w32_c8_kernel<3,", "gemm_qkv_rope": "gemm_w32_c8_kernel<4,",
                       "attn_partial": "tree_attn2_partial_kernel", "attn_reduce": "tree_attn_reduce_kernel"}
PROF_KERNEL_KEYS_PAIRED = {"gemm_none": "gemm_w32_kernel<2, 0,", "gemm_residual": "gemm_w32_kernel<2, 1,", "gemm_swiglu": "gemm_w32_kernel<2, 2,",
                           "gemm_splitk_partial": "gemm_w32_kernel<2, 3,", "gemm_qkv_rope": "gemm_w32_kernel<2, 4,",
                           "attn_partial": "tree_attn2_partial_kernel", "attn_reduce": "tree_attn_reduce_kernel"}
PROF_KERNEL_KEYS = {"gemm_none": "gemm_w32_kernel<1, 0,", "gemm_residual": "gemm_w32_kernel<1, 1,", "gemm_swiglu": "gemm_w32_kernel<1, 2,",
                    "gemm_splitk_partial": "gemm_w32_kernel<1, 3,", "gemm_qkv_rope": "gemm_w32_kernel<1, 4,",
                    "attn_partial": "tree_attn2_partial_kernel", "attn_reduce": "tree_attn_reduce_kernel"}


if __name__ == "__main__":
    main()
