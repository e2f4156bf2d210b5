"""Host-side pieces of return_logprobs that need no GPU: the result truncation helper and the float64 reference of the kernel test."""
import numpy as np
import pytest
import torch

from logprob_helpers import bf16_round, kernel_bar, ref_token_logprob
from vispec_amd.model.spec_model_ours import _logprob_kw, _truncate_logprobs


def test_truncation_follows_the_token_array():
    """The log is indexed by token position; a result of n_tokens ids behind a prompt of L keeps entries [L, n_tokens) — wherever the ids
    were cut (EOS, budget, full KV cache), including a value already written for a token behind the cut."""
    log = np.zeros(40, np.float32)
    log[7:20] = -np.arange(1, 14, dtype=np.float32)  # prompt of 7, 13 values written (one of them for the not yet committed next token)
    toks = np.arange(19)                              # ... of which the result keeps 12
    got = _truncate_logprobs(log, 7, len(toks))
    assert got.dtype == np.float32 and got.shape == (12,)
    np.testing.assert_array_equal(got, -np.arange(1, 13, dtype=np.float32))
    got[0] = 5.0
    assert log[7] == -1.0  # a copy: the caller's array is not a view of the log
    assert _truncate_logprobs(log, 7, 7).shape == (0,)  # no round ran (max_length <= 0): the prompt as it is, no values
    assert _truncate_logprobs(log.astype(np.float64), 7, 9).dtype == np.float32
    for bad in ((7, 41), (8, 7), (-1, 5)):
        with pytest.raises(ValueError):
            _truncate_logprobs(log, *bad)


def test_the_option_travels_as_nothing_when_off():
    assert _logprob_kw(False) == {} and _logprob_kw(True) == {"return_logprobs": True}


@pytest.mark.parametrize("V", [7, 1000, 32000])
def test_float64_reference_against_torch_log_softmax(V):
    rng = np.random.default_rng(V)
    row = bf16_round(rng.standard_normal(V).astype(np.float32) * 4.0)
    assert np.array_equal(torch.from_numpy(row).to(torch.bfloat16).float().numpy(), row)  # bf16_round == torch's rounding
    want = torch.log_softmax(torch.from_numpy(row).double(), dim=0).numpy()
    for t in (0, V // 2, V - 1, int(np.argmax(row))):
        assert abs(ref_token_logprob(row, t) - want[t]) <= 1e-12
    assert abs(ref_token_logprob(np.full(V, 1.5), 3) + np.log(V)) <= 1e-12
    # the derived kernel bar stays far below anything a misplaced value could hide in
    assert kernel_bar(152064, 40.0) < 1e-4 and kernel_bar(7, 1.0) > 0
