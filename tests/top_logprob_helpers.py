"""Shared pieces of the top-N log-probability tests (tests/test_top_logprobs_cpu.py, tests/test_top_logprobs_gpu.py): the float64
reference of one row.  The value bar is logprob_helpers.kernel_bar: the kernel takes (m, log Z) from the very reduction that bar was
derived for and adds one more x - m - log Z per listed token, the two roundings the bar already counts."""
import math

import numpy as np

TOP_MAX = 20  # include/vispec_hip.h: VISPEC_TOP_LOGPROBS_MAX


def ref_top(row, N):
    """(ids int32 [N], values float64 [N]) of a row of (bf16-valued) logits: the N largest by lexicographic (-value, id) — -0.0 counts as
    +0.0, so the two zeros tie and the lower id goes first — with log_softmax(row)[id] in float64; a row shorter than N is padded with
    id -1, value -inf."""
    x = np.asarray(row, np.float64) + 0.0  # (-0.0 + 0.0 = +0.0: one zero)
    order = np.lexsort((np.arange(len(x)), -x))[:N]
    m = x.max()
    lz = math.log(np.exp(x - m).sum())
    ids = np.full(N, -1, np.int32)
    vals = np.full(N, -np.inf, np.float64)
    ids[:len(order)] = order
    vals[:len(order)] = x[order] - m - lz
    return ids, vals
