"""Malformed weight lists for the GPU tests of the weighted operators: each corruption would
stay in bounds even if the operator did not check it (the replacement is never smaller than
the tensor it stands in for), so a missing check shows as a test failure, not as a fault."""
import re

import pytest
import torch


def corruptions(w, i):
    """[(what, list)]: copies of ``w`` whose bf16 tensor i is replaced by a float32 tensor of the
    same element count, by a longer tensor, and by a non-contiguous view into a larger one."""
    t = w[i]
    assert t.dtype == torch.bfloat16 and t.numel() > 0
    n = t.numel()
    bad = {"float32": t.float(),
           "longer": torch.cat([t.reshape(-1), t.new_zeros(8)]),
           "strided": t.new_zeros(2 * n)[::2]}
    return [(k, w[:i] + [v] + w[i + 1:]) for k, v in bad.items()]


def assert_refused(call, w, i, field):
    """``call(list)`` raises for every corruption of slot i, naming the slot and its field."""
    for what, bad in corruptions(list(w), i):
        with pytest.raises(RuntimeError, match=re.escape(f"weights[{i}] ({field})")):
            call(bad)
            pytest.fail(f"the {what} tensor in weights[{i}] ({field}) was accepted")
