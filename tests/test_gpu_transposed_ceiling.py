"""The transposed product at the size ceiling: the matrix of tests/ceiling.py (exactly K_MAX = 2^31 - 1 - 65536 entries, small
integer values and operand, so every product and sum is exact in fp64) multiplied by A^T through both routes --
smvp_csr_create_transposed + the default smvp_csr_spmv + smvp_csr_spmm with k = 1, and smvp_tjds_spmv_transposed (K8) on the
TJDS built by smvp_tjds_from_coo_device -- against the exact int64 reference (index_add_ over the columns, in row chunks: the
mirror of Ceiling.product_ref).  A non-integer operand is checked on column slices against the C oracle run over the
transposed arrays.  Each section frees what it holds before the next.

Observed on the MI355X (309 GB of HBM by hipMemGetInfo), polling the free memory from a thread while
smvp_csr_create_transposed ran: 83.7 GB in use before the call (the matrix, its references, the source handle's plan), 171.0 GB
more at the peak (the 34.4 GB entry list, the sort's key and index buffers, the 25.8 GB result), 57.5 GB more afterwards (the
transposed arrays and the plan AUTO built over them: the binned plan); the call took 8.7 s.  test_create_transposed_at_the_ceiling
prints the figures of its own run.
"""
import threading
import time

import numpy as np
import pytest

import ceiling as cz
import oracle_binding as ob
import smvp_toolkit_amd as sm
from parity import check_y, guarded_y
from test_gpu_ceiling import Ceiling, assert_exact, assert_guards, free

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert sm.device_count() >= 1
    return torch


class TransposedCeiling(Ceiling):
    """The ceiling matrix plus the exact A^T x of the integer operand and what the column slices need."""

    def __init__(self, torch):
        super().__init__(torch)
        self.yt_ref = self.transposed_ref(self.x)
        self.frac = {}          # column slice -> the oracle's A^T x_frac on it (oracle_slices)

    def transposed_ref(self, x, chunk=1 << 21):
        """A^T x for an integer-valued float64 x, exact (int64 sums over the columns, row chunk by row chunk)."""
        import torch

        xi = x.to(torch.int64)
        y = torch.zeros(self.cols, dtype=torch.int64, device="cuda")
        rp = self.row_ptr.to(torch.int64)
        for r0 in range(0, self.L["first_empty"], chunk):
            r1 = min(self.L["first_empty"], r0 + chunk)
            e0, e1 = int(rp[r0]), int(rp[r1])
            row = torch.repeat_interleave(torch.arange(r0, r1, device="cuda"), rp[r0 + 1:r1 + 1] - rp[r0:r1])
            y.index_add_(0, self.col_ind[e0:e1].to(torch.int64), self.val[e0:e1].to(torch.int64) * xi[row])
        assert int(y.abs().max()) < 2 ** 53
        return y.to(torch.float64)

    def column_slices(self):
        """The first 2^16 columns, 2^16 in the middle (the scattered rows' columns) and the last 2^16."""
        w = 1 << 16
        return [(0, w), (self.cols // 2, self.cols // 2 + w), (self.cols - w, self.cols)]


@pytest.fixture(scope="module")
def M(torch):
    free(torch)
    m = TransposedCeiling(torch)
    yield m
    assert (cz.checksum(torch, m.row_ptr), cz.checksum(torch, m.col_ind[:m.nnz]), cz.checksum(torch, m.val[:m.nnz])) == m.check
    del m
    free(torch)


class LowWater:
    """Polls the device's free memory from a thread while a call runs: the least it saw."""

    def __init__(self, torch):
        self.torch, self.least, self.stop = torch, torch.cuda.mem_get_info()[0], False
        self.thread = threading.Thread(target=self.run)

    def run(self):
        while not self.stop:
            self.least = min(self.least, self.torch.cuda.mem_get_info()[0])
            time.sleep(0.002)

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        self.thread.join()
        return False


def view(torch, ptr, n, typestr):
    class Raw:
        __cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}

    return torch.as_tensor(Raw(), device="cuda")


def oracle_slices(M, trp, tci, tv):
    """M.frac[column slice] = (the oracle's A^T x_frac, its sum of |terms|, the terms per column) over the transposed arrays."""
    xh = M.x_frac.cpu().numpy()
    h_trp = trp.cpu().numpy()
    for c0, c1 in M.column_slices():
        rp = h_trp[c0:c1 + 1].astype(np.int64)
        e0, e1 = int(rp[0]), int(rp[-1])
        ci, v = tci[e0:e1].cpu().numpy(), tv[e0:e1].cpu().numpy()
        rp32 = (rp - e0).astype(np.int32)
        M.frac[(c0, c1)] = (ob.csr_spmv(rp32, ci, v, xh), ob.csr_spmv(rp32, ci, np.abs(v), np.abs(xh)), np.diff(rp))


def product(torch, M, call, what):
    buf, y = guarded_y(torch, M.cols)
    call(y)
    torch.cuda.synchronize()
    assert_guards(torch, buf, what)
    return y


def test_create_transposed_at_the_ceiling(torch, M):
    """smvp_csr_create_transposed of the adopted ceiling matrix: the result's arrays are a CSR of A^T (column counts, rows
    ascending inside every column), its default spmv and spmm k = 1 give the exact product; with the non-integer operand
    spmm k = 1 is the oracle's bits on the column slices and the default spmv is inside check_y's bound."""
    A = sm.CsrMatrix(M.rows, M.cols, M.row_ptr, M.col_ind[:M.nnz], M.val[:M.nnz])
    At = None
    try:
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        t0 = time.time()
        with LowWater(torch) as low:
            At = A.transposed()
        after = torch.cuda.mem_get_info()[0]
        print("smvp_csr_create_transposed at K_MAX: %.1f s; device memory in use before %.1f GB, at the peak %.1f GB more, "
              "afterwards %.1f GB more (the transposed arrays and their plan); AUTO runs %s"
              % (time.time() - t0, (torch.cuda.mem_get_info()[1] - before) / 1e9, (before - low.least) / 1e9,
                 (before - after) / 1e9, At.describe()[0]))
        A.close()
        A = None
        free(torch)
        assert (At.rows, At.cols, At.nnz) == (M.cols, M.rows, M.nnz)
        p = At.device_arrays()
        trp, tci, tv = view(torch, p[0], M.cols + 1, "<i4"), view(torch, p[1], M.nnz, "<i4"), view(torch, p[2], M.nnz, "<f8")
        # a CSR of A^T: the columns' counts, and inside every column strictly ascending rows (the matrix repeats no pair)
        counts = torch.zeros(M.cols, dtype=torch.int64, device="cuda")
        for e0 in range(0, M.nnz, 1 << 28):
            c = M.col_ind[e0:min(M.nnz, e0 + (1 << 28))].to(torch.int64)
            counts += torch.bincount(c, minlength=M.cols)
            del c
        assert int(trp[0]) == 0 and torch.equal(trp[1:].to(torch.int64), torch.cumsum(counts, 0))
        del counts
        for e0 in range(0, M.nnz - 1, 1 << 28):
            e1 = min(M.nnz - 1, e0 + (1 << 28))
            falls = torch.nonzero(tci[e0 + 1:e1 + 1] <= tci[e0:e1]).flatten() + e0 + 1     # positions that do not ascend ...
            starts = torch.searchsorted(trp, falls.to(torch.int32), right=False)
            assert bool((trp[starts.clamp(max=M.cols)] == falls).all()), "rows do not ascend inside a column"   # ... start a column
            del falls, starts
        free(torch)
        y = product(torch, M, lambda y: At.spmv(M.x, y, stream=torch.cuda.current_stream()), "default spmv")
        assert_exact(torch, y, M.yt_ref, "default spmv on the transposed handle (%s)" % At.describe()[0])
        y = product(torch, M, lambda y: At.spmm(M.x.view(-1, 1), y.view(-1, 1), stream=torch.cuda.current_stream()), "spmm k = 1")
        assert_exact(torch, y, M.yt_ref, "spmm k = 1 on the transposed handle")
        y_mm = product(torch, M, lambda y: At.spmm(M.x_frac.view(-1, 1), y.view(-1, 1), stream=torch.cuda.current_stream()), "spmm k = 1")
        y_mv = product(torch, M, lambda y: At.spmv(M.x_frac, y, stream=torch.cuda.current_stream()), "default spmv")
        oracle_slices(M, trp, tci, tv)
        for (c0, c1), (ref, scale, terms) in M.frac.items():
            assert np.array_equal(y_mm[c0:c1].cpu().numpy(), ref), "columns [%d, %d): spmm k = 1 differs from the oracle's bits" % (c0, c1)
            check_y(y_mv[c0:c1].cpu().numpy(), ref, scale, terms)
        del trp, tci, tv, y, y_mm, y_mv
    finally:
        if A is not None:
            A.close()
        if At is not None:
            At.close()
        free(torch)


def test_k8_at_the_ceiling(torch, M):
    """K8 on the TJDS that smvp_tjds_from_coo_device builds from the shuffled COO: the exact product, and on the column
    slices the bits the oracle gave over the transposed CSR arrays (one lane sums a column from top to bottom)."""
    if not M.frac:              # (run on its own: the oracle's slices need the transposed arrays)
        A = sm.CsrMatrix(M.rows, M.cols, M.row_ptr, M.col_ind[:M.nnz], M.val[:M.nnz])
        At = A.transposed()
        A.close()
        p = At.device_arrays()
        oracle_slices(M, view(torch, p[0], M.cols + 1, "<i4"), view(torch, p[1], M.nnz, "<i4"), view(torch, p[2], M.nnz, "<f8"))
        At.close()
        free(torch)
    coo = cz.build_coo(torch, M.row_ptr, M.col_ind, M.val, M.nnz, "cuda")
    t = sm.tjds_from_coo_device(coo, M.rows, M.cols, M.nnz)
    del coo
    free(torch)
    T = sm.TjdsMatrix(t)
    try:
        name, alg = T.transposed_describe()
        assert name == "tjds_transposed_columns"
        assert alg == 12.0 * M.nnz + 4.0 * (t.num_diag + 1) + 4.0 * M.cols + 8.0 * M.rows + 8.0 * M.cols
        y = product(torch, M, lambda y: T.spmv_transposed(M.x, y, stream=torch.cuda.current_stream()), name)
        assert_exact(torch, y, M.yt_ref, name)
        y = product(torch, M, lambda y: T.spmv_transposed(M.x_frac, y, stream=torch.cuda.current_stream()), name)
        for (c0, c1), (ref, _, _) in M.frac.items():
            assert np.array_equal(y[c0:c1].cpu().numpy(), ref), "columns [%d, %d): K8 differs from the oracle's bits" % (c0, c1)
        del y
    finally:
        T.close()
        del T, t
        free(torch)
