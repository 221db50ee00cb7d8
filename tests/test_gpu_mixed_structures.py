"""GPU: every product path on the structures of tests/mixed_structures.py -- repeated (row, col) pairs, rows whose columns are
not ascending, rectangular matrices and row blocks (first_row != 0), at sizes that cross K6's row blocks, the binned plan's column
blocks and buckets and the 65536-column span of the 16-bit offsets (test_mixed_structures_host.py holds the structures to those
conditions and shows that the exact reference rejects the wrong kernels they are for).

Forward: the path list of test_gpu_special_values.py (csr_paths with the block's first_row; tjds_paths on the whole matrices), the
binned plan with binned_overlap 0 | 1 and bands 1, 600 and 4096.  Exact operands: the int64 reference's bits on every path, x and
y aligned and one double off.  Real operands: parity.check_y and the serial loop's bits on the rows a path sums left to right.
Products that promise bits (smvp_csr_spmm, K8, K9, the transposed handle) run on the real operands, where the order of a column's
ties shows.  The converters run on the shuffled entry lists; the sharded layer on `repeats` and `tall`."""
import ctypes as C
import itertools

import numpy as np
import pytest

import mixed_structures as ms
import oracle_binding as ob
import smvp_toolkit_amd as sm
import special_values as sv
import test_gpu_parity as gp
import test_gpu_spmm as gs
import test_gpu_spmm_transposed as gst
import test_gpu_transposed as gt
import transposed as tr
from parity import check_y
from test_gpu_special_values import Operands, csr_paths, scale_of, tjds_paths

pytestmark = pytest.mark.gpu

BANDS = (1, 600, 4096)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def binned_paths(rows, cols, row_ptr, col_ind, val, first_row):
    """(label, run, mask, kernel name) of the binned plan with pass A beside the near part (binned_overlap 1) and behind it (0),
    at the default band and at bands 1, 600 and 4096; no promise of the serial loop's bits."""
    none = np.zeros(rows, dtype=bool)
    for overlap in (0, 1):
        with sm.option("binned_overlap", overlap):
            A = sm.CsrMatrix(rows, cols, row_ptr, col_ind, val, first_row=first_row)
            try:
                for band in (0,) + BANDS:
                    A.set_kernel(sm.CSR_KERNEL_BINNED, band)
                    assert A.get_kernel() == (sm.CSR_KERNEL_BINNED, band or 4096)
                    yield "BINNED band %d, binned_overlap %d" % (band, overlap), (lambda dx, dy, stream=None: A.spmv(dx, dy, stream=stream)), none, A.describe()[0]
            finally:
                A.close()


# ---------------------------------------------------------------------------------------------------------- forward paths
@pytest.mark.parametrize("name", ms.NAMES)
def test_forward_products_on_every_path(torch, name):
    rows, cols, row0, _ = ms.structure(name)
    g = ms.assert_regime(name)
    ops = Operands(torch, rows, cols)
    checks, kernels = 0, set()
    for kind in ("exact", "real"):
        coo, x, _ = ms.operands(name, kind)
        rp, ci, v = ms.csr_of(name, coo)
        terms = np.diff(rp)
        if kind == "exact":
            ref = ms.reference(name)
        else:
            ref, scale, finite = ob.csr_spmv(rp, ci, v, x), scale_of(rp, ci, v, x), np.zeros(rows, dtype=int)
        paths = [csr_paths(rows, cols, rp, ci, v, first_row=row0), binned_paths(rows, cols, rp, ci, v, row0)]
        if row0 == 0:
            paths.append(tjds_paths(rows, cols, rp, ci, v))
        for label, run, serial, kernel in itertools.chain(*paths):
            what = "%s, %s operands, %s (%s)" % (name, kind, label, kernel)
            first = ops.product(run, x)
            if kind == "exact":
                sv.check_bits(first, ref, what)
                sv.check_bits(ops.product(run, x, 1), ref, what + ", x and y one double off")
            else:
                sv.assert_against_oracle(first, ref, scale, terms, finite, what, serial)
            if serial is not None:                                    # (None: TJDS ATOMIC, whose order changes from run to run)
                sv.check_bits(ops.product(run, x), first, what + ": the second product against the first")
            kernels.add(kernel.split("<")[0].split(":")[0])
            checks += 1
    assert {"csr_stream_owner", "csr_stream_tiles", "csr_colsweep", "csr_binned"} <= kernels, kernels
    print("mixed structures: %s: %d (path, operands) checks; regime %r" % (name, checks, g))


@pytest.mark.parametrize("name", ms.NAMES)
def test_auto_far_share_and_the_window_plan(torch, name):
    """AUTO goes to the carry form of the tile kernel (a row above kOwnerMaxRow); the far share is the host's count with the
    diagonal at first_row + r; the binned plan of a block whose windows reach into x keeps its near part on csr_near_window."""
    rows, cols, row0, _ = ms.structure(name)
    g = ms.regime(name)
    coo, x, _ = ms.operands(name, "exact")
    rp, ci, v = ms.csr_of(name, coo)
    A = sm.CsrMatrix(rows, cols, rp, ci, v, first_row=row0)
    assert A.get_kernel()[0] == sm.CSR_KERNEL_STREAM_CARRY and g["max_row"] > ms.OWNER_MAX_ROW
    assert abs(A.far_share() - g["far_share"]) <= 1e-6, (A.far_share(), g["far_share"])
    A.set_kernel(sm.CSR_KERNEL_BINNED, 0)
    if ms.kind_of(name) != "block_off":
        assert "csr_near_window" in A.describe()[0], A.describe()[0]
    sv.check_bits(Operands(torch, rows, cols).product(lambda dx, dy: A.spmv(dx, dy), x), ms.reference(name), name + ", " + A.describe()[0])
    A.close()


# ------------------------------------------------------------------------------------------- products with bit promises
@pytest.mark.parametrize("name", ms.WHOLE)
def test_spmm_gives_the_serial_loops_bits_per_column(torch, name):
    rows, cols, _, _ = ms.structure(name)
    coo, _, _ = ms.operands(name, "real")
    rp, ci, v = ms.csr_of(name, coo)
    X = np.random.default_rng(17).standard_normal((cols, 17))
    for k, ldx, ldy in ((1, 2, 3), (3, 5, 4), (17, 19, 24)):
        gs.run_case(torch, rows, cols, rp, ci, v, np.ascontiguousarray(X[:, :k]), ldx=ldx, ldy=ldy)


@pytest.mark.parametrize("name", ms.WHOLE)
def test_transposed_products_sum_ties_in_storage_order(torch, name):
    """K8 and K9 from the TJDS handle, the transposed CSR handle under AUTO, STREAM 1024 and VECTOR 8 with smvp_csr_spmm on it:
    the bits of transposed.reference; the transposed handle's arrays are smvp_csr_from_coo's of the swapped entries, and
    transposing twice gives back smvp_csr_from_coo of the entries themselves -- whatever order the rows of the source have."""
    rows, cols, _, _ = ms.structure(name)
    coo, _, xr = ms.operands(name, "real")
    rp, ci, v = ms.csr_of(name, coo)
    ref = gt.both_routes(torch, rows, cols, coo, xr, name, csr_arrays=(rp, ci, v))
    A = sm.CsrMatrix(rows, cols, rp, ci, v)
    At = A.transposed()
    want = tr.transposed_csr(coo, cols)
    scale = ob.csr_spmv(want[0], want[1], np.abs(want[2]), np.abs(xr))
    for kernel, param in ((sm.CSR_KERNEL_AUTO, 0), (sm.CSR_KERNEL_STREAM, 1024), (sm.CSR_KERNEL_VECTOR, 8)):
        At.set_kernel(kernel, param)
        tr.assert_bits(gt.spmm1(torch, At, xr), ref, "%s: spmm k = 1 on the transposed handle, kernel %d param %d" % (name, kernel, param))
        check_y(gt.spmv(torch, At, xr), ref, scale, np.diff(want[0]))
    Att = At.transposed()
    gt.assert_arrays(gt.arrays_of(torch, Att), sm.csr_from_coo(coo, rows), name + ": transposed twice")
    for M in (Att, At, A):
        M.close()
    Xr = np.random.default_rng(18).standard_normal((rows, 17))
    for k, ldx, ldy in ((1, 1, 1), (3, 4, 6), (17, 20, 17)):
        gst.run_case(torch, rows, cols, coo, np.ascontiguousarray(Xr[:, :k]), "%s, K9, k = %d" % (name, k), ldx=ldx, ldy=ldy, routes=(k == 3))


# --------------------------------------------------------------------------------------------------------------- converters
@pytest.mark.parametrize("name", ms.WHOLE)
def test_device_converters_on_the_shuffled_entries(torch, name):
    rows, cols, _, _ = ms.structure(name)
    coo, x, _ = ms.operands(name, "exact")
    t = gp._check_device_conversion(torch, coo, rows, cols)
    assert (t.num_diag > rows) == (ms.kind_of(name) != "square")
    ref = ms.reference(name)
    ops = Operands(torch, rows, cols)
    T = sm.TjdsMatrix(t)                                               # over the device-built arrays, adopted in place
    for mode in gp.TJDS_MODES:
        T.set_mode(mode)

        def run(dx, dy):
            T.set_x(dx)
            T.zero_y(dy)
            T.spmv(dy)
        sv.check_bits(ops.product(run, x), ref, "%s: TJDS mode %d over the device-built arrays" % (name, mode))
    T.close()


@pytest.mark.parametrize("name", [n for n in ms.WHOLE if ms.kind_of(n) == "repeats"])
def test_converters_refuse_a_start_pos_too_short_for_the_repeats(torch, name):
    """start_pos_capacity = rows + 1 suffices only when no pair repeats: both converters return SMVP_ERR_INVALID, and the device
    one leaves the words around its start_pos alone."""
    rows, cols, _, coo = ms.structure(name)
    nnz, cap, g = len(coo), rows + 1, 64
    assert ms.regime(name)["num_diag"] + 1 > cap
    nd = C.c_int(-1)
    perm, ri, val = np.zeros(cols, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz)
    sp = np.full(cap + 2 * g, 0x5A17C0DE, dtype=np.int32)
    rc = sm.lib().smvp_tjds_from_coo(sm._p(coo), rows, cols, nnz, sm._p(perm), C.c_void_p(sp.ctypes.data + 4 * g), cap, sm._p(ri), sm._p(val),
                                     C.byref(nd), None, None)
    assert rc == sm.ERR_INVALID and (sp[:g] == 0x5A17C0DE).all() and (sp[g + cap:] == 0x5A17C0DE).all()
    d_coo = gp._coo_to_device(torch, coo)
    d_perm = torch.zeros(cols, dtype=torch.int32, device="cuda")
    d_ri = torch.zeros(nnz, dtype=torch.int32, device="cuda")
    d_val = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    d_sp = torch.full((cap + 2 * g,), 0x5A17C0DE, dtype=torch.int32, device="cuda")
    rc = sm.lib().smvp_tjds_from_coo_device(sm._dev_ptr(d_coo), rows, cols, nnz, sm._dev_ptr(d_perm), sm._dev_ptr(d_sp.data_ptr() + 4 * g), cap,
                                            sm._dev_ptr(d_ri), sm._dev_ptr(d_val), C.byref(nd), None, None, None)
    torch.cuda.synchronize()
    assert rc == sm.ERR_INVALID
    h = d_sp.cpu().numpy()
    assert (h[:g] == 0x5A17C0DE).all() and (h[g + cap:] == 0x5A17C0DE).all(), "the device converter wrote past the start_pos it was given"
    # with room for every diagonal the same call succeeds (sm.tjds_from_coo_device: capacity max(rows, nnz) + 2)
    assert sm.tjds_from_coo_device(d_coo, rows, cols, nnz).num_diag == ms.regime(name)["num_diag"]


# ------------------------------------------------------------------------------------------------------------------ sharded
@pytest.mark.parametrize("push", ["copies", "direct"])
@pytest.mark.parametrize("name", [n for n in ms.WHOLE if ms.kind_of(n) in ("repeats", "tall")])
def test_sharded_products_on_three_virtual_ranks(torch, name, push):
    """3 virtual ranks x 2 chunks: every chunk is a row block with a first_row of its own (CSR) or a TJDS matrix whose longest
    column may outgrow its rows; every rank's gathered y has the exact reference's bits."""
    rows, cols, _, _ = ms.structure(name)
    coo, x, _ = ms.operands(name, "exact")
    csr = ms.csr_of(name, coo)
    ref = ms.reference(name)
    exchange = sm.EXCHANGE_COPIES if push == "copies" else sm.EXCHANGE_DIRECT
    for fmt, settings in (("csr", (None, (sm.CSR_KERNEL_BINNED, 0))), ("tjds", (None,))):
        S = sm.ShardedMatrix(fmt, 3, rows, cols, coo=coo, csr=csr, devices=[0] * 3, chunks=2, exchange=exchange)
        chunks, bounds, cb = S.layout()
        assert chunks == 2 and bounds[0] == 0 and bounds[-1] == rows
        firsts = np.unique(cb[:, :-1])
        assert (firsts % ms.K6_ROWS != 0).any() and len(firsts) >= 4, cb
        if fmt == "tjds" and ms.kind_of(name) == "repeats":            # the chunk that holds the repeated pair: a column longer than its rows
            assert ms.regime(name)["most_copies"] > np.diff(cb, axis=1).max()
        for setting in settings:
            if setting:
                S.set_csr_kernel(*setting)
            S.set_x(x)
            S.spmv(allgather=sm.GATHER_OVERLAPPED)
            S.synchronize()
            for slot in range(3):
                sv.check_bits(S.get_y(slot, gathered=True), ref, "%s, %s, %s, %r, rank %d" % (name, fmt, push, setting, slot))
        S.close()
