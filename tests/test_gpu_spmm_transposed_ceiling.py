"""The block transposed product at the size ceiling: the matrix of tests/ceiling.py (exactly K_MAX = 2^31 - 1 - 65536 entries,
small integer values and operand, so every product and sum is exact in fp64) multiplied by A^T for k = 2 vectors through
smvp_tjds_spmm_transposed (K9) on the TJDS built by smvp_tjds_from_coo_device, against the exact int64 reference of
test_gpu_transposed_ceiling.py (TransposedCeiling.transposed_ref), the way test_k8_at_the_ceiling checks K8.

Column 0 of X is the integer operand x, column 1 is 2 - x: Y(:, 0) = A^T x and Y(:, 1) = 2 A^T 1 - A^T x, exactly.  Y is a slice
of a block with leading dimension 3 between guards, X one with leading dimension 2.
"""
import pytest

import ceiling as cz
import smvp_toolkit_amd as sm
from parity import G, GUARD
from test_gpu_ceiling import assert_exact, assert_guards, free
from test_gpu_transposed_ceiling import TransposedCeiling

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert sm.device_count() >= 1
    return torch


@pytest.fixture(scope="module")
def M(torch):
    free(torch)
    m = TransposedCeiling(torch)
    yield m
    assert (cz.checksum(torch, m.row_ptr), cz.checksum(torch, m.col_ind[:m.nnz]), cz.checksum(torch, m.val[:m.nnz])) == m.check
    del m
    free(torch)


def test_k9_at_the_ceiling(torch, M):
    """K9 with k = 2 on the TJDS of the shuffled COO: both columns are the exact products, the padding column and the guards
    keep their bits, and column 0 is bit for bit what K8 gives on the same handle."""
    ones_ref = M.transposed_ref(torch.ones(M.rows, dtype=torch.float64, device="cuda"))
    coo = cz.build_coo(torch, M.row_ptr, M.col_ind, M.val, M.nnz, "cuda")
    t = sm.tjds_from_coo_device(coo, M.rows, M.cols, M.nnz)
    del coo
    free(torch)
    T = sm.TjdsMatrix(t)
    try:
        k, ldy = 2, 3
        name, alg = T.spmm_transposed_describe(k)
        assert name == "tjds_spmm_transposed_columns<2>"
        assert alg == 12.0 * M.nnz + 4.0 * (t.num_diag + 1) + 4.0 * M.cols + 8.0 * k * (M.rows + M.cols)
        X = torch.empty(M.rows, k, dtype=torch.float64, device="cuda")
        X[:, 0] = M.x
        X[:, 1] = 2.0 - M.x
        buf = torch.empty(M.cols * ldy + 2 * G, dtype=torch.float64, device="cuda")
        buf.view(torch.int64).fill_(int(GUARD))
        Y = buf[G:G + M.cols * ldy].view(M.cols, ldy)[:, :k]
        Y.fill_(float("nan"))
        T.spmm_transposed(X, Y, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert_guards(torch, buf, name)
        pad = buf[G:G + M.cols * ldy].view(M.cols, ldy)[:, k:].contiguous().view(torch.int64)
        assert bool((pad == int(GUARD)).all()), "%s wrote the padding column" % name
        del pad
        assert_exact(torch, Y[:, 0].contiguous(), M.yt_ref, name + ", column 0")
        assert_exact(torch, Y[:, 1].contiguous(), 2.0 * ones_ref - M.yt_ref, name + ", column 1")
        y8 = torch.full((M.cols,), float("nan"), dtype=torch.float64, device="cuda")
        T.spmv_transposed(M.x, y8, stream=torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert torch.equal(Y[:, 0].contiguous().view(torch.int64), y8.view(torch.int64)), "column 0 differs from K8's bits"
        del X, Y, buf, y8
    finally:
        T.close()
        del T, t
        free(torch)
