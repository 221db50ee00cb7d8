"""Every product path at the size ceiling: one matrix of exactly K_MAX = 2^31 - 1 - 65536 entries (the most smvp_csr_create
and smvp_tjds_create accept), built on the device (tests/ceiling.py) and adopted in place, multiplied by every CSR kernel,
smvp_csr_spmm and every TJDS mode; the device converters and the radix sort / scans at the same size; the refusal of one
entry more.

Values and operands are small integers, so every product is exact in fp64 and every path must give the int64 reference bit
for bit, whatever its order of summation (the atomic TJDS mode and the column parts included).  A second, non-integer
operand is checked on host-side slices against the C oracle.  Every y lies in a guarded buffer.  Sections free what they
hold before the next: torch's own peak is about 100 GB (the TJDS section), the library's plans come on top of it.
"""
import os
import subprocess
import time

import numpy as np
import pytest

import ceiling as cz
import oracle_binding as ob
import smvp_toolkit_amd as sm
from parity import BIN_ROW_CAP, G, GUARD, binned_fits, check_y, guarded_y

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert sm.device_count() >= 1       # the library's HIP runtime starts here, before anything else uses the card
    return torch


def free(torch):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


class Ceiling:
    """The full-size matrix on the device, its reference products and what the checks need on the host."""

    def __init__(self, torch):
        t0 = time.time()
        self.L = L = cz.layout()
        self.rows = self.cols = L["rows"]
        self.nnz = L["nnz"]
        self.row_ptr, self.col_ind, self.val, self.y_ref = cz.build(torch, L, "cuda")
        self.x = cz.x_int(torch, self.cols, "cuda").to(torch.float64)
        ones = torch.ones(self.cols, dtype=torch.float64, device="cuda")
        self.h_row_ptr = self.row_ptr.cpu().numpy()
        self.sums = None
        self.sums = self.product_ref(ones)            # A 1: the spmm operands' second term
        del ones
        # a non-integer operand for the slices: x / 3 rounded (the products and sums then round)
        self.x_frac = self.x / 3.0
        self.check = (cz.checksum(torch, self.row_ptr), cz.checksum(torch, self.col_ind[:self.nnz]),
                      cz.checksum(torch, self.val[:self.nnz]))
        self.build_s = time.time() - t0

    def product_ref(self, x, chunk=1 << 21):
        """A x for an integer-valued float64 x, exact (int64 sums over row chunks)."""
        import torch

        xi = x.to(torch.int64)
        y = torch.zeros(self.rows, dtype=torch.int64, device="cuda")
        rp = self.row_ptr.to(torch.int64)
        for r0 in range(0, self.L["first_empty"], chunk):
            r1 = min(self.L["first_empty"], r0 + chunk)
            e0, e1 = int(rp[r0]), int(rp[r1])
            row = torch.repeat_interleave(torch.arange(r0, r1, device="cuda"), rp[r0 + 1:r1 + 1] - rp[r0:r1])
            y.index_add_(0, row, self.val[e0:e1].to(torch.int64) * xi[self.col_ind[e0:e1].to(torch.int64)])
        return y.to(torch.float64)

    def slices(self):
        """Row slices checked against the C oracle: the first 2^16 rows, every row with an entry beyond 2^31 - 2^25, the
        long (last non-empty) row and the empty rows after it."""
        rp = self.h_row_ptr
        tail = int(np.searchsorted(rp, 2 ** 31 - 2 ** 25, side="right")) - 1
        return [(0, 1 << 16), (tail, self.rows), (self.L["long_row"], self.L["long_row"] + 1)]


@pytest.fixture(scope="module")
def M(torch):
    free(torch)
    m = Ceiling(torch)
    yield m
    # the matrix arrays are only read by every path (and every plan built over them)
    assert (cz.checksum(torch, m.row_ptr), cz.checksum(torch, m.col_ind[:m.nnz]), cz.checksum(torch, m.val[:m.nnz])) == m.check
    del m
    free(torch)


def assert_guards(torch, buf, what):
    g = buf.view(torch.int64)
    assert bool((g[:G] == int(GUARD)).all()) and bool((g[-G:] == int(GUARD)).all()), "%s: wrote outside y" % what


def assert_exact(torch, y, ref, what):
    if torch.equal(y, ref):
        return
    bad = torch.nonzero(y != ref).flatten()
    r = int(bad[0]) if bad.numel() else -1
    raise AssertionError("%s: %d rows differ from the exact product; first row %d: %r against %r" % (
        what, bad.numel(), r, float(y[r]), float(ref[r])))


def csr_product(torch, M, A, x, what):
    buf, y = guarded_y(torch, M.rows)
    A.spmv(x, y, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert_guards(torch, buf, what)
    return y


def all_rows(rows, lens):
    return np.ones(len(rows), bool)


def check_slices(torch, M, y, serial):
    """y of the non-integer operand against the C oracle on M.slices(): inside the rounding bound everywhere, the serial
    loop's bits on the rows `serial(row numbers, row lengths)` marks."""
    xh = M.x_frac.cpu().numpy()
    for r0, r1 in M.slices():
        rp = M.h_row_ptr[r0:r1 + 1].astype(np.int64)
        e0, e1 = int(rp[0]), int(rp[-1])
        ci, v = M.col_ind[e0:e1].cpu().numpy(), M.val[e0:e1].cpu().numpy()
        rp32 = (rp - e0).astype(np.int32)
        ref = ob.csr_spmv(rp32, ci, v, xh)
        scale = ob.csr_spmv(rp32, ci, np.abs(v), np.abs(xh))
        got = y[r0:r1].cpu().numpy()
        lens = np.diff(rp)
        check_y(got, ref, scale, lens)
        s = serial(np.arange(r0, r1), lens)
        assert np.array_equal(got[s], ref[s]), "rows [%d, %d): a row summed in the serial order differs" % (r0, r1)


def run_csr(torch, M, A, kernel, param, want_name, frac=None):
    A.set_kernel(kernel, param)
    name = A.describe()[0]
    assert want_name in name, "set_kernel(%d, %#x) runs %s, not %s" % (kernel, param, name, want_name)
    y = csr_product(torch, M, A, M.x, name)
    assert_exact(torch, y, M.y_ref, name)
    if frac is not None:
        check_slices(torch, M, csr_product(torch, M, A, M.x_frac, name), frac)
    return name


# ------------------------------------------------------------------------------------------------- 1: the matrix itself
def test_matrix_holds_exactly_the_ceiling(torch, M):
    L, rp = M.L, M.h_row_ptr
    assert int(rp[-1]) == cz.K_MAX == M.nnz
    lens = np.diff(rp.astype(np.int64))
    assert lens[L["long_row"]] > 2048 and rp[L["long_row"] + 1] == cz.K_MAX and (lens[L["first_empty"]:] == 0).all()
    assert rp[L["long_row"]] >= cz.K_MAX - (1 << 20)          # the long row lies in the last 2^20 entries
    assert cz.K_MAX % 2048 and cz.K_MAX % 256                 # the last tile is part full at every tile size
    print("matrix: %d rows, %d entries, built with its reference in %.1f s" % (M.rows, M.nnz, M.build_s))


# ---------------------------------------------------------------------------------------------------- 2: the CSR paths
def test_auto_stream_carry_and_vector(torch, M):
    A = sm.CsrMatrix(M.rows, M.cols, M.row_ptr, M.col_ind[:M.nnz], M.val[:M.nnz])
    try:
        name = A.describe()[0]
        kind = A.get_kernel()
        print("AUTO: %s (kernel %d, param %d), far share %.3f, gather spread %.3f" % (name, kind[0], kind[1], A.far_share(),
                                                                                       A.gather_spread()))
        y = csr_product(torch, M, A, M.x, "AUTO " + name)
        assert_exact(torch, y, M.y_ref, "AUTO " + name)
        del y
        for tile in (256, 1024, 2048):
            for col16 in (1, 0):
                with sm.option("csr_col16", col16):
                    # (the banded rows' tiles span a few hundred columns: most tiles fit 16-bit offsets; 256-entry tiles keep
                    # 32-bit columns)
                    c16 = 5 if col16 and tile >= 1024 else 0
                    run_csr(torch, M, A, sm.CSR_KERNEL_STREAM, tile, "csr_stream_owner<%d, %d, false>" % (tile // 256, c16),
                            frac=(lambda rows, lens: lens <= 32) if (tile, col16) == (2048, 1) else None)
        for tile in (1024, 2048):
            run_csr(torch, M, A, sm.CSR_KERNEL_STREAM_CARRY, tile, "csr_stream_tiles<%d>" % (tile // 256))
        for lanes in (2, 8, 64):
            run_csr(torch, M, A, sm.CSR_KERNEL_VECTOR, lanes, "csr_vector_rows<%d>" % lanes)
    finally:
        A.close()
        free(torch)


def test_colsweep_every_part_count(torch, M):
    A = sm.CsrMatrix(M.rows, M.cols, M.row_ptr, M.col_ind[:M.nnz], M.val[:M.nnz])
    try:
        # one column part: ascending columns, the serial loop's bits on every row
        name = run_csr(torch, M, A, sm.CSR_KERNEL_COLSWEEP, 0, "csr_colsweep<", frac=all_rows)
        assert "parts" not in name, name
        rb = A.get_kernel()[1] & 0xFFFFFF
        for parts in (2, 4, 8):
            run_csr(torch, M, A, sm.CSR_KERNEL_COLSWEEP, sm.sweep_parts(min(rb, 20480 // parts // 4 * 4), parts),
                    "(%d column parts" % parts)
    finally:
        A.close()
        free(torch)


def test_binned_on_both_sides_of_its_32_bit_guard(torch, M):
    """The default band (far share about 0.36) fits the binned plan's 32-bit stream positions and multiplies exactly; band 1
    (every banded entry far) does not, is refused with ERR_UNSUPPORTED as binned_fits predicts, and leaves the handle on the
    tile kernel, multiplying exactly.  With the non-integer operand, the banded rows (at most 16 entries, none far: one lane
    from left to right in the near part, nothing added by the far part) are the serial loop's bits."""
    A = sm.CsrMatrix(M.rows, M.cols, M.row_ptr, M.col_ind[:M.nnz], M.val[:M.nnz])
    try:
        for band in (0, 1):
            nf = cz.binned_far_count(torch, M.row_ptr, M.col_ind[:M.nnz], band if band else 4096, BIN_ROW_CAP)
            print("band %d: %d far entries, fits %s" % (band, nf, binned_fits(nf, M.cols)))
            assert binned_fits(nf, M.cols) == (band == 0)
            for near in (0, 1):
                with sm.option("binned_near", near):
                    if band == 0:
                        run_csr(torch, M, A, sm.CSR_KERNEL_BINNED, 0,
                                "csr_binned: csr_stream_owner<" if near else "csr_binned: csr_near_window",
                                frac=lambda rows, lens: rows < M.L["rb"])
                        continue
                    run_csr(torch, M, A, sm.CSR_KERNEL_STREAM, 2048, "csr_stream_owner<8, 5, false>")
                    with pytest.raises(sm.SmvpError) as e:
                        A.set_kernel(sm.CSR_KERNEL_BINNED, band)
                    assert e.value.code == sm.ERR_UNSUPPORTED, str(e.value)
                    name = A.describe()[0]
                    assert name == "csr_stream_owner<8, 5, false>", name   # the tile kernel's default plan
                    assert_exact(torch, csr_product(torch, M, A, M.x, name), M.y_ref, "after the refusal: " + name)
    finally:
        A.close()
        free(torch)


def test_spmm_k_1_8_17_and_a_wider_y(torch, M):
    """Column v of X is s_v x + t_v (s_v = +-1, t_v in -2 ... 2): Y(:, v) = s_v A x + t_v A 1, exactly."""
    A = sm.CsrMatrix(M.rows, M.cols, M.row_ptr, M.col_ind[:M.nnz], M.val[:M.nnz])
    try:
        for k, ldy in ((1, 1), (8, 8), (17, 17), (8, 9)):
            s = [1.0 if v % 2 == 0 else -1.0 for v in range(k)]
            t = [float(v % 5 - 2) for v in range(k)]
            X = torch.empty(M.cols, k, dtype=torch.float64, device="cuda")
            for v in range(k):
                X[:, v] = s[v] * M.x + t[v]
            buf = torch.empty(M.rows * ldy + 2 * G, dtype=torch.float64, device="cuda")
            buf.view(torch.int64).fill_(int(GUARD))
            Y = buf[G:G + M.rows * ldy].view(M.rows, ldy)[:, :k]
            Y.fill_(float("nan"))
            A.spmm(X, Y, stream=torch.cuda.current_stream())
            torch.cuda.synchronize()
            assert_guards(torch, buf, "spmm k = %d" % k)
            if ldy > k:
                pad = buf[G:G + M.rows * ldy].view(M.rows, ldy)[:, k:].contiguous().view(torch.int64)
                assert bool((pad == int(GUARD)).all()), "spmm k = %d wrote a padding column" % k
            for v in range(k):
                assert_exact(torch, Y[:, v].contiguous(), s[v] * M.y_ref + t[v] * M.sums, "spmm k = %d column %d" % (k, v))
            if k == 1:
                X1 = M.x_frac.view(M.cols, 1)
                Y.fill_(float("nan"))
                A.spmm(X1, Y, stream=torch.cuda.current_stream())
                torch.cuda.synchronize()
                check_slices(torch, M, Y[:, 0].contiguous(), all_rows)
            del X, Y, buf
            free(torch)
    finally:
        A.close()
        free(torch)


# ------------------------------------------------------------------------------------------------ TJDS and the converters
def test_device_converters_and_every_tjds_mode(torch, M):
    """The matrix as a shuffled COO (34 GB): the device CSR equals the torch-built arrays; the device TJDS multiplies exactly
    in ROW_GATHER with each of its three index forms (16-bit half words, 32-bit sorted words, 32-bit columns: a handle built
    under each tjds_index option) at tiles 256 and 2048, in TWO_PHASE and in ATOMIC."""
    coo = cz.build_coo(torch, M.row_ptr, M.col_ind, M.val, M.nnz, "cuda")
    rp, ci, v = sm.csr_from_coo_device(coo, M.rows, M.cols, M.nnz)
    assert torch.equal(rp, M.row_ptr) and torch.equal(ci, M.col_ind[:M.nnz]) and torch.equal(v, M.val[:M.nnz])
    del rp, ci, v
    free(torch)
    t = sm.tjds_from_coo_device(coo, M.rows, M.cols, M.nnz)
    del coo
    free(torch)
    for index, flavor in ((0, 4), (1, 3), (2, 2)):         # kFlavorTjdsH / S / K (smvp_kernels.h)
        with sm.option("tjds_index", index):
            T = sm.TjdsMatrix(t)                            # (the arrays are adopted; the row-gather plan is built here)
        try:
            T.set_x(M.x)
            for tile in (256, 2048):
                T.set_tile(tile)
                tjds_check(torch, M, T, "csr_stream_owner<%d, %d, false>" % (tile // 256, flavor),
                           frac=index == 0 and tile == 2048)
            if index == 0:
                T.set_mode(sm.TJDS_MODE_TWO_PHASE)
                tjds_check(torch, M, T, "tjds_colmajor_products + csr_stream_owner<")
                T.set_mode(sm.TJDS_MODE_ATOMIC)
                tjds_check(torch, M, T, "tjds_colmajor_scatter<false>", frac=True)
        finally:
            T.close()
            del T
            free(torch)
    del t
    free(torch)


def tjds_check(torch, M, T, want_name, frac=False):
    """One product of T into a guarded y: T runs `want_name` (a prefix of describe()) and gives the exact product; with frac,
    also the non-integer operand against the C oracle on the slices -- the serial bits only on rows of one or two entries,
    which every order sums alike (TJDS sums a row in the order of its jagged diagonals, not of its columns)."""
    name = T.describe()[0]
    assert name.startswith(want_name), "TJDS runs %s, not %s" % (name, want_name)
    for x in (M.x, M.x_frac) if frac else (M.x,):
        T.set_x(x)
        buf, y = guarded_y(torch, M.rows)
        T.zero_y(y)
        T.spmv(y)
        torch.cuda.synchronize()
        assert_guards(torch, buf, name)
        if x is M.x:
            assert_exact(torch, y, M.y_ref, name)
        else:
            check_slices(torch, M, y, lambda rows, lens: lens <= 2)
        del buf, y
    T.set_x(M.x)


# ------------------------------------------------------------------------------------------------------- 4: the ceiling
def test_one_entry_more_is_refused_before_any_allocation(torch, M):
    """K_MAX + 1 entries: CsrMatrix, TjdsMatrix, both device converters (their Python wrappers, which allocate the outputs,
    and the C functions themselves) refuse with ERR_UNSUPPORTED before anything large is allocated."""
    import ctypes as C

    rp = M.row_ptr.clone()
    rp[M.L["long_row"] + 1:] += 1                     # the long row takes the spare element
    n = cz.K_MAX + 1
    assert n == sm.MAX_ENTRIES + 1
    M.col_ind[M.nnz] = 0
    M.val[M.nnz] = 1.0
    coo = torch.empty(16, dtype=torch.uint8, device="cuda")      # never read: the count is refused first
    tiny = torch.empty(16, dtype=torch.int32, device="cuda")     # nor written
    t = sm.TjdsArrays()
    t.rows, t.cols, t.nnz, t.num_diag = M.rows, M.cols, n, 1
    t.perm, t.start_pos, t.row_ind, t.val = rp, rp, M.col_ind, M.val
    t.ref_num_tjdiag, t.last_diag_single = 1, 0
    nd, rn, ls = C.c_int(), C.c_int(), C.c_int()
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    refusals = [
        ("CsrMatrix", lambda: sm.CsrMatrix(M.rows, M.cols, rp, M.col_ind[:n], M.val[:n])),
        ("TjdsMatrix", lambda: sm.TjdsMatrix(t)),
        ("csr_from_coo_device", lambda: sm.csr_from_coo_device(coo, M.rows, M.cols, n)),
        ("tjds_from_coo_device", lambda: sm.tjds_from_coo_device(coo, M.rows, M.cols, n)),
    ]
    for what, call in refusals:
        with pytest.raises(sm.SmvpError) as e:
            call()
        assert e.value.code == sm.ERR_UNSUPPORTED, "%s: %s" % (what, e.value)
    p = sm._dev_ptr
    assert sm.lib().smvp_csr_from_coo_device(p(coo), M.rows, M.cols, n, p(tiny), p(tiny), p(tiny), None) == sm.ERR_UNSUPPORTED
    assert sm.lib().smvp_tjds_from_coo_device(p(coo), M.rows, M.cols, n, p(tiny), p(tiny), 16, p(tiny), p(tiny), C.byref(nd),
                                              C.byref(rn), C.byref(ls), None) == sm.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert free_before - torch.cuda.mem_get_info()[0] < (64 << 20)
    M.col_ind[M.nnz] = 0
    M.val[M.nnz] = 0.0
    import resource
    print("peak HBM (torch) %.1f GB, peak host RSS %.2f GB" % (torch.cuda.max_memory_allocated() / 1e9,
                                                              resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6))


# ------------------------------------------------------------------------------------------------------- 3: primitives
def test_prim_check_at_full_size(torch):
    """The radix sort (32-bit keys: a multiplicative permutation and i mod 7; 64-bit keys) and the scans of ones at K_MAX
    elements, generated and checked on the device.  Last in the file: the library's own HIP runtime has started before (in a
    process where it started only after this child had used the card, it found no device)."""
    exe = os.path.join(ROOT, "smvp-toolkit_amd", "bin", "prim_check")
    r = subprocess.run([exe, "full", str(cz.K_MAX)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "prim full ok" in r.stdout, r.stdout + r.stderr
