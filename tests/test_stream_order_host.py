"""Host: the parts of tests/stream_order.py that need no stream -- what an operand holds while its true content is in flight."""
import numpy as np
import pytest
import torch

import smvp_toolkit_amd as sm
import stream_order as so


def test_stale_structures_are_valid_and_differ_from_the_true_ones():
    coo = sm.make_coo([3, 1, 2], [0, 2, 1], [1.5, -2.0, 4.0])
    raw = torch.from_numpy(np.ascontiguousarray(coo).view(np.uint8).copy())
    stale = so.stale_like(torch, raw, "coo")
    back = stale.numpy().view(sm.COO_DTYPE)
    assert stale.shape == raw.shape and back["row"].tolist() == [0] * 3 and back["col"].tolist() == [0] * 3 and back["val"].tolist() == [1.0] * 3
    index = torch.tensor([4, 0, 7], dtype=torch.int32)
    assert so.stale_like(torch, index).tolist() == [0, 0, 0] and so.stale_like(torch, index).dtype == index.dtype


def test_stage_leaves_stale_content_and_keeps_the_true_one_apart():
    x = torch.arange(5, dtype=torch.float64)
    dst, true = so.stage(torch, x)
    assert dst is x and torch.isnan(x).all() and true.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and true.data_ptr() != x.data_ptr()
    index = torch.tensor([4, 0, 7], dtype=torch.int32)
    dst, true = so.stage(torch, index, so.stale_like(torch, index))
    assert index.tolist() == [0, 0, 0] and true.tolist() == [4, 0, 7]
    with pytest.raises(AssertionError):
        so.stage(torch, torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32))       # a stale copy of the true content shows nothing
    with pytest.raises(AssertionError):
        so.stage(torch, torch.tensor([1, 2], dtype=torch.int32))                                     # an index array needs its stale structure
