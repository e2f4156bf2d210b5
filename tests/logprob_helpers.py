"""Shared pieces of the token log-probability tests (tests/test_logprobs_cpu.py, tests/test_logprobs_gpu.py): the float64 reference, the
derived error bars and the oracle's teacher-forced log-probabilities."""
import math

import numpy as np

from helpers import T, vo

LOGPROB_THREADS = 1024  # csrc/tree_kernels.h: the one block size of token_logprob_kernel / token_logprob_row_kernel
U = 2.0 ** -24          # unit round-off of fp32


def bf16_round(x):
    """float32 values rounded to the nearest-even bf16, returned as float32 (what a bf16 tensor holds)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def ref_token_logprob(row, tok):
    """log_softmax(row)[tok] in float64 of a row of (bf16-valued) logits: the reference of the kernel test."""
    x = np.asarray(row, np.float64)
    m = x.max()
    return float(x[tok] - m - math.log(np.exp(x - m).sum()))


def kernel_bar(V, max_abs):
    """Absolute error bound of the kernel's fp32 value against ref_token_logprob on the SAME bf16 logits, derived from its summation shape
    (not tuned).  The kernel is a one-pass (running max, rescaled sum-exp) reduction, so the shape differs from a two-pass sum:
      per thread   steps = ceil(ceil(V / 8) / threads) vector steps + 1 tail step.  A step adds 8 positive terms (8 roundings, 8u relative
                   on the running sum) and may rescale the sum once by expf(m_old - m_new): expf is within 1 ulp = 2u, its argument (a
                   difference of two bf16 values) adds at most 1u, the multiply 1u -> 4u.  12u per step.  Each term itself: expf 2u +
                   argument 1u = 3u, once.
      merges       6 xor-butterfly levels inside the wave, then 15 serial merges of the 16 wave pairs through LDS.  A merge rescales both
                   sides (4u each, on disjoint terms -> 4u on the result) and adds once (1u): 5u per merge, 21 merges.
      => relative error of Z <= (12 * steps + 5 * 21 + 3) u, the same absolute error in log Z;
      logf is within 1 ulp: 2u * |log Z| <= 2u * ln V (Z is in [1, V] after the max is taken out);
      the two subtractions x[tok] - m - log Z round once each: 2u * (2 * max|x| + ln V) at most."""
    steps = math.ceil(math.ceil(V / 8) / LOGPROB_THREADS) + 1
    rel_z = (12 * steps + 5 * (6 + LOGPROB_THREADS // 64 - 1) + 3) * U
    return rel_z + 2 * U * math.log(V) + 2 * U * (2 * max_abs + math.log(V))


def oracle_logprobs(ot, toks, n_prompt):
    """(float64 [len(toks) - n_prompt], max|logits|): the oracle target's teacher-forced log-probability of every generated token of
    `toks` — ONE forward over toks[:-1], log-softmax of row n_prompt - 1 + i at toks[n_prompt + i] — and the scale of those logits."""
    toks = np.asarray(toks, np.int64)
    pkv, _, _ = vo.initialize_past_key_values(T["NL"], T["H"], T["max_pos"], T["D"] // T["H"])
    ot.tree_mask = None
    lg, _ = ot.forward(pkv, input_ids=toks[:-1])
    lg = np.asarray(lg, np.float64)
    out = np.array([ref_token_logprob(lg[n_prompt - 1 + i], toks[n_prompt + i]) for i in range(len(toks) - n_prompt)])
    return out, float(np.abs(lg[n_prompt - 1:]).max())


def loop_bar(max_abs_logits):
    """Device-vs-oracle bar of a log-probability: the project's logits bar (2^-6 * max|logits|, tests/test_loop_gpu.py) moves x[tok] by at
    most that much and log-sum-exp is 1-Lipschitz in the sup norm: twice the logits bar."""
    return 2.0 * 2.0 ** -6 * max_abs_logits
