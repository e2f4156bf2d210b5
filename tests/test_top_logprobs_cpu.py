"""Host-side pieces of top_logprobs= that need no GPU: the float64 reference of the kernel test (against torch.topk + log_softmax and on
hand-written tie / zero / padding rows), the option's refusals, how it travels to a request start, the truncation helper, and the
ctypes prototypes against the header."""
import os
import re

import numpy as np
import pytest
import torch

from logprob_helpers import bf16_round
from top_logprob_helpers import TOP_MAX, ref_top
from vispec_amd import lib as L
from vispec_amd.model.spec_model_ours import _check_top_logprobs, _logprob_kw, _start_kw, _top_kw, _truncate_top_logprobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("V", [7, 1000, 32064])
@pytest.mark.parametrize("N", [1, 5, 20])
def test_reference_against_torch_topk_and_float64_log_softmax_on_rows_without_ties(V, N):
    rng = np.random.default_rng(V + N)
    pos = np.arange(0x0080, 0x4300, dtype=np.uint32)  # every positive normal bf16 below 128, and their negatives: distinct values
    row = (rng.choice(np.concatenate([pos, pos | 0x8000]), V, replace=False) << 16).astype(np.uint32).view(np.float32)
    assert len(np.unique(row)) == V and np.array_equal(bf16_round(row), row)
    ids, vals = ref_top(row, N)
    k = min(N, len(row))
    t = torch.from_numpy(row).double()
    want_v, want_i = torch.topk(t, k)
    np.testing.assert_array_equal(ids[:k], want_i.numpy())
    lsm = torch.log_softmax(t, dim=0).numpy()
    assert np.abs(vals[:k] - lsm[ids[:k]]).max() <= 1e-12
    assert ids.dtype == np.int32 and ids.shape == vals.shape == (N,)
    assert np.all(ids[k:] == -1) and np.all(np.isneginf(vals[k:]))
    assert np.all(np.diff(vals[:k]) <= 0)


def test_reference_tie_zero_and_padding_rules_on_hand_written_rows():
    # ties: value descending, then the LOWER id
    ids, vals = ref_top(np.array([1.0, 3.0, 2.0, 3.0, 2.0, 3.0, 0.5], np.float32), 5)
    np.testing.assert_array_equal(ids, [1, 3, 5, 2, 4])
    assert vals[0] == vals[1] == vals[2] and vals[3] == vals[4] < vals[0]
    # all equal: ids 0 .. N-1, each -ln V
    ids, vals = ref_top(np.full(9, -2.5, np.float32), 4)
    np.testing.assert_array_equal(ids, [0, 1, 2, 3])
    assert np.abs(vals + np.log(9)).max() <= 1e-12
    # +0.0 and -0.0 are ONE value: the ids decide, whatever the sign
    row = np.array([-1.0, -0.0, 0.0, 0.5, -0.0, 0.0, -3.0], np.float32)
    assert np.signbit(row[1]) and not np.signbit(row[2])
    ids, vals = ref_top(row, 4)
    np.testing.assert_array_equal(ids, [3, 1, 2, 4])
    assert vals[1] == vals[2] == vals[3]
    # the N-th place inside a run of equal values: the lowest ids of the run
    ids, _ = ref_top(np.array([0.0, 7.0, 1.0, 1.0, 9.0, 1.0, 1.0], np.float32), 4)
    np.testing.assert_array_equal(ids, [4, 1, 2, 3])
    # V < N: the tail is id -1, value -inf; the head a full log-softmax (it sums to one)
    ids, vals = ref_top(np.array([0.25, -1.0, 2.0], np.float32), 5)
    np.testing.assert_array_equal(ids, [2, 0, 1, -1, -1])
    assert np.all(np.isneginf(vals[3:])) and abs(np.exp(vals[:3]).sum() - 1.0) <= 1e-12
    # an all-negative row
    ids, vals = ref_top(np.array([-5.0, -4.0, -6.0], np.float32), 2)
    np.testing.assert_array_equal(ids, [1, 0])
    assert np.all(vals < 0)


# ---------------------------------------------------------------------------------------------------------------- the option
def test_the_option_travels_as_nothing_when_off_and_beside_the_logprob_flag_when_on():
    assert _top_kw(0) == {} and _top_kw(5) == {"top_logprobs": 5}
    assert _logprob_kw(True) == {"return_logprobs": True}  # the flag's own keywords are what they were
    off = _start_kw(0.0, 0, False, None, False)
    assert "top_logprobs" not in off and "return_logprobs" not in off
    assert _start_kw(0.0, 0, False, None, True) == {**off, "return_logprobs": True}
    assert _start_kw(0.0, 0, False, None, True, False, 7) == {**off, "return_logprobs": True, "top_logprobs": 7}


def test_refusals_come_from_the_arguments_alone():
    _check_top_logprobs(0, False)
    _check_top_logprobs(0, True)
    _check_top_logprobs(20, True)
    _check_top_logprobs([0, 3, 20], True)
    _check_top_logprobs([0, 0], False)
    for bad in (21, -1, 2.5, True, [1, 21], "3"):
        with pytest.raises(ValueError):
            _check_top_logprobs(bad, True)
    for n in (3, [0, 3]):
        with pytest.raises(ValueError, match="return_logprobs"):
            _check_top_logprobs(n, False)


def test_entry_points_refuse_before_any_device_work():
    """ValueError from the public calls with objects that have no engine at all: nothing of the model is touched first."""
    from vispec_amd.model import SpecModel
    from vispec_amd.model.spec_model_ours import specgenerate_cohort, specgenerate_stream
    sm = SpecModel.__new__(SpecModel)  # no engine, no weights: any device work would raise AttributeError instead
    ids = torch.zeros(1, 4, dtype=torch.long)
    for kw in (dict(top_logprobs=3), dict(top_logprobs=21, return_logprobs=True), dict(top_logprobs=-1, return_logprobs=True)):
        with pytest.raises(ValueError):
            sm.specgenerate(ids, **kw)
        with pytest.raises(ValueError):
            sm.baseline_generate(ids, **kw)
        with pytest.raises(ValueError):
            specgenerate_stream([sm, sm], [(ids, {})] * 3, **kw)
    with pytest.raises(ValueError):
        specgenerate_stream([sm, sm], [(ids, {})] * 3, return_logprobs=True, top_logprobs=[1, 2])  # not one entry per request


# ---------------------------------------------------------------------------------------------------------------- truncation
def test_truncation_follows_the_token_array_and_the_requested_width():
    ids_log = np.zeros((40, TOP_MAX), np.int32)
    vals_log = np.zeros((40, TOP_MAX), np.float32)
    ids_log[7:20, :5] = np.arange(13 * 5).reshape(13, 5) + 100  # a prompt of 7, 13 positions written with N = 5
    vals_log[7:20, :5] = -np.arange(13 * 5, dtype=np.float32).reshape(13, 5) - 1
    got_i, got_v = _truncate_top_logprobs(ids_log, vals_log, 7, 19, 5)
    assert got_i.dtype == np.int32 and got_v.dtype == np.float32 and got_i.shape == got_v.shape == (12, 5)
    np.testing.assert_array_equal(got_i, ids_log[7:19, :5])
    np.testing.assert_array_equal(got_v, vals_log[7:19, :5])
    got_i[0, 0] = -7
    assert ids_log[7, 0] == 100  # copies
    assert _truncate_top_logprobs(ids_log, vals_log, 7, 7, 5)[0].shape == (0, 5)   # no round ran
    assert _truncate_top_logprobs(ids_log, vals_log, 7, 19, 0)[1].shape == (12, 0)  # a cohort member that asked for none
    for bad in ((7, 41, 5), (8, 7, 5), (-1, 5, 5), (7, 19, 21), (7, 19, -1)):
        with pytest.raises(ValueError):
            _truncate_top_logprobs(ids_log, vals_log, *bad)
    with pytest.raises(ValueError):
        _truncate_top_logprobs(ids_log, vals_log[:, :10], 7, 19, 5)


# ---------------------------------------------------------------------------------------------------------------- the boundary
def header_prototypes():
    src = open(os.path.join(ROOT, "include", "vispec_hip.h")).read()
    macro = re.search(r"#define\s+VISPEC_TOP_LOGPROBS_MAX\s+(\d+)", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {name: [a.strip() for a in args.split(",")] for name, args in re.findall(r"\bint\s+(vispec_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src)}
    return protos, int(macro.group(1))


def ctype_of(arg):
    if "*" in arg:
        return L.P
    assert re.match(r"(const\s+)?int\b", arg), arg
    return L.c_int


def test_ctypes_prototypes_match_the_header():
    protos, width = header_prototypes()
    assert width == L.TOP_LOGPROBS_MAX == TOP_MAX == 20
    for name in ("vispec_set_top_logprobs", "vispec_token_top_logprob_row", "vispec_get_top_logprobs_host"):
        res, args = L.SIGNATURES[name]
        assert res is L.c_int
        assert args == [ctype_of(a) for a in protos[name]], (name, protos[name])
    # ... by the same reading that reproduces the neighbouring, long-standing entries
    for name in ("vispec_set_logprobs", "vispec_token_logprob_row", "vispec_get_logprobs_host"):
        assert L.SIGNATURES[name][1] == [ctype_of(a) for a in protos[name]], name
