"""GPU: handles over adopted device arrays (SMVP_MEM_DEVICE) on every plan, and the re-plan contract of include/smvp_amd.h (the
note above SMVP_CSR_KERNEL_*): which plans see val / col_ind changed in place at once, which need smvp_csr_set_kernel,
smvp_tjds_set_value_cache or re-creation, and that a transposed handle is a copy of its own.

tests/adopted.py has the structure `mixed`, its three column arrays and two value arrays, and the exact int64 references;
test_adopted_host.py shows that a product of stale entries never has the new reference's bits.  Operands are integers: every path,
TJDS ATOMIC included, is compared bit for bit (transposed.assert_bits), no tolerance anywhere.  Every product goes into a guarded
buffer and the guards are checked.  Only promises are asserted: no test says that a path IS stale.

The CSR paths are those of test_gpu_special_values.csr_paths (AUTO, the CSR_VARIANTS, COLSWEEP with 2 | 4 | 8 column parts,
STREAM 1024 under csr_col16 1 | 0 and csr_rowrel default | 0, BINNED under binned_near 0 | 1), the TJDS paths the TJDS_MODES and
the TJDS_GATHER_VARIANTS with the value cache 0 and 2 (the row-order stream "k32" has no cache: 0 only).
"""
import contextlib
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import adopted as ad
import smvp_toolkit_amd as sm
from parity import check_guards, guarded_y
from test_gpu_parity import CSR_VARIANTS, TJDS_GATHER_VARIANTS, TJDS_MODES, tjds_gather_matrix
from test_gpu_spmm import spmm
from test_gpu_spmm_transposed import k9
from transposed import assert_bits

pytestmark = pytest.mark.gpu

M = ad.mixed()
TILE_KERNELS = (sm.CSR_KERNEL_STREAM, sm.CSR_KERNEL_STREAM_CARRY)
COL16_STREAM = "STREAM 1024, csr_col16 1, csr_rowrel None"            # the path test 4 is for


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def refs():
    """(columns, values) -> the exact y = A x, computed once and left unchanged."""
    cache = {}

    def ref(cols="cols_a", val="val0"):
        if (cols, val) not in cache:
            cache[cols, val] = ad.reference(M.row_ptr, getattr(M, cols), getattr(M, val), M.x)
            cache[cols, val].setflags(write=False)
        return cache[cols, val]
    return ref


# ------------------------------------------------------------------------------------------------------------------ paths
def csr_settings():
    """(label, plan options, kernel, param) of every CSR path."""
    out = [("AUTO", {}, sm.CSR_KERNEL_AUTO, 0)] + [("kernel %d param %d" % kp, {}, kp[0], kp[1]) for kp in CSR_VARIANTS]
    out += [("COLSWEEP 1024 rows, %d parts" % p, {}, sm.CSR_KERNEL_COLSWEEP, sm.sweep_parts(1024, p)) for p in (2, 4, 8)]
    out += [("STREAM 1024, csr_col16 %r, csr_rowrel %r" % (c, r), {"csr_col16": c, "csr_rowrel": r}, sm.CSR_KERNEL_STREAM, 1024)
            for c in (1, 0) for r in (None, 0)]
    out += [("BINNED band 0, binned_near %d" % n, {"binned_near": n}, sm.CSR_KERNEL_BINNED, 0) for n in (0, 1)]
    assert COL16_STREAM in [s[0] for s in out]
    return out


@contextlib.contextmanager
def options(opts):
    with contextlib.ExitStack() as stack:
        for name, value in opts.items():
            stack.enter_context(sm.option(name, value))
        yield


def replan(A, setting):
    """The documented refresh: smvp_csr_set_kernel with the same kernel and the same param, under the setting's plan options."""
    label, opts, kernel, param = setting
    with options(opts):
        A.set_kernel(kernel, param)
    assert kernel == sm.CSR_KERNEL_AUTO or A.get_kernel()[0] == kernel, label
    return A


def csr_handle(setting, rows, cols, rp, ci, v, first_row=0):
    """A handle under the setting over numpy arrays (copied) or torch tensors (adopted)."""
    with options(setting[1]):
        A = sm.CsrMatrix(rows, cols, rp, ci, v, first_row=first_row)
    return replan(A, setting)


def state(A):
    return A.describe(), A.get_kernel(), A.launches()


def tjds_paths(t):
    """(label, handle) of every TJDS path over t (numpy arrays: copied, torch tensors: adopted); the handle is closed afterwards."""
    T = sm.TjdsMatrix(t)
    try:
        for mode in TJDS_MODES:
            T.set_mode(mode)
            yield "TJDS mode %d" % mode, T
    finally:
        T.close()
    for label, index, tile, cache in gather_settings():
        T = gather_handle(t, index, tile, cache)
        try:
            yield label, T
        finally:
            T.close()


def gather_settings():
    return [("TJDS %s tile %d, value cache %d" % (index, tile, cache), index, tile, cache) for index, tile in TJDS_GATHER_VARIANTS
            for cache in ((0, 2) if index in ("half", "sorted") else (0,))]


def gather_handle(t, index, tile, cache):
    T = tjds_gather_matrix(t, index, tile)
    T.set_value_cache(cache)
    assert T.get_value_cache()[0] == cache and (T.get_value_cache()[1] > 0) == (cache > 0)
    return T


# --------------------------------------------------------------------------------------------------------------- products
def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()                        # (a copy: the fixtures are read-only)


def adopt(torch, cols="cols_a", val="val0"):
    return dev(torch, M.row_ptr), dev(torch, getattr(M, cols)), dev(torch, getattr(M, val))


def put(torch, tensor, a):
    """tensor <- a in place, finished before the next call."""
    tensor.copy_(torch.from_numpy(np.array(a)))
    torch.cuda.synchronize()


def spmv(torch, A, dx):
    buf, dy = guarded_y(torch, A.rows)
    A.spmv(dx, dy)
    torch.cuda.synchronize()
    check_guards(buf, A.rows)
    return dy.cpu().numpy()


def tjds_spmv(torch, T, dx=None):
    """One TJDS product; dx None: the operand of an earlier smvp_tjds_set_x is multiplied again."""
    buf, dy = guarded_y(torch, T.rows)
    if dx is not None:
        T.set_x(dx)
    T.zero_y(dy)
    T.spmv(dy)
    torch.cuda.synchronize()
    check_guards(buf, T.rows)
    return dy.cpu().numpy()


def k8(torch, T, dx_rows):
    buf, dy = guarded_y(torch, T.cols)
    T.spmv_transposed(dx_rows, dy)
    torch.cuda.synchronize()
    check_guards(buf, T.cols)
    return dy.cpu().numpy()


def coo_to_device(torch, coo):
    return torch.from_numpy(np.ascontiguousarray(coo, dtype=sm.COO_DTYPE).view(np.uint8).copy()).cuda()


def tjds_pair(torch, cols="cols_a", val="val0"):
    """(host arrays, device tensors) of the structure's TJDS form: smvp_tjds_from_coo and smvp_tjds_from_coo_device."""
    coo = ad.coo(M.row_ptr, getattr(M, cols), getattr(M, val))
    return sm.tjds_from_coo(coo, M.rows, M.cols), sm.tjds_from_coo_device(coo_to_device(torch, coo), M.rows, M.cols, len(coo))


def tjds_values(val):
    """`val` (CSR order) in the order of the TJDS val array: the structure is the same, so are perm, start_pos and row_ind."""
    t = sm.tjds_from_coo(ad.coo(M.row_ptr, M.cols_a, val), M.rows, M.cols)
    return t.val


def bits_equal(torch, a, b):
    view = (lambda t: t.view(torch.int64)) if a.dtype == torch.float64 else (lambda t: t)
    return a.shape == b.shape and bool(torch.equal(view(a), view(b)))


# ------------------------------------------------------------------------------------------------- 1. adopted equals copied
def test_adopted_equals_copied_on_every_csr_path(torch, refs):
    d_rp, d_ci, d_v = adopt(torch)
    dx = dev(torch, M.x)
    ref = refs()
    for setting in csr_settings():
        A = csr_handle(setting, M.rows, M.cols, d_rp, d_ci, d_v)
        B = csr_handle(setting, M.rows, M.cols, M.row_ptr, M.cols_a, M.val0)
        assert state(A) == state(B), setting[0]
        ya, yb = spmv(torch, A, dx), spmv(torch, B, dx)
        assert_bits(ya, ref, "%s (%s), adopted" % (setting[0], A.describe()[0]))
        assert_bits(yb, ref, "%s (%s), copied" % (setting[0], B.describe()[0]))
        assert_bits(ya, yb, "%s, adopted against copied" % setting[0])
        A.close()
        B.close()


def test_adopted_equals_copied_on_every_tjds_path(torch, refs):
    t_host, t_dev = tjds_pair(torch)
    dx, dx_rows = dev(torch, M.x), dev(torch, M.x_rows)
    ref = refs()
    ref_t = ad.reference_t(M.row_ptr, M.cols_a, M.val0, M.x_rows, M.cols)
    ref_block = ad.reference_t(M.row_ptr, M.cols_a, M.val0, M.X_rows, M.cols)
    checked = 0
    for (label, A), (label_b, B) in zip(tjds_paths(t_dev), tjds_paths(t_host)):
        assert label == label_b and A.describe() == B.describe() and A.get_value_cache() == B.get_value_cache(), label
        ya, yb = tjds_spmv(torch, A, dx), tjds_spmv(torch, B, dx)
        assert_bits(ya, ref, "%s (%s), adopted" % (label, A.describe()[0]))
        assert_bits(yb, ref, "%s, copied" % label)
        if label.startswith("TJDS mode") or label.endswith("tile 0, value cache 2"):
            for T, kind in ((A, "adopted"), (B, "copied")):
                assert_bits(k8(torch, T, dx_rows), ref_t, "K8, %s, %s" % (label, kind))
                assert_bits(k9(torch, T, M.X_rows, ldx=5, ldy=4), ref_block, "K9 k = 3, %s, %s" % (label, kind))
        checked += 1
    assert checked == len(TJDS_MODES) + len(gather_settings())


def test_adopted_row_block(torch, refs):
    """The last third of the rows adopted as a row block with first_row = 8192 (views into the whole matrix's arrays): the
    binned plan, whose near / far split goes by first_row, and smvp_csr_spmm give the matching slice of the reference."""
    d_rp, d_ci, d_v = adopt(torch)
    r0 = ad.block_start(M.row_ptr, M.rows)
    e0 = int(M.row_ptr[r0])
    rows = M.rows - r0
    block_rp = (M.row_ptr[r0:] - e0).astype(np.int32)
    assert d_ci[e0:].data_ptr() % 16 == 0 and d_v[e0:].data_ptr() % 16 == 0
    setting = ("BINNED band 0", {}, sm.CSR_KERNEL_BINNED, 0)
    A = csr_handle(setting, rows, M.cols, dev(torch, block_rp), d_ci[e0:], d_v[e0:], first_row=8192)
    B = csr_handle(setting, rows, M.cols, block_rp, M.cols_a[e0:], M.val0[e0:], first_row=8192)
    assert state(A) == state(B) and A.far_share() == B.far_share() >= 0
    dx = dev(torch, M.x)
    ref_block = ad.reference(M.row_ptr, M.cols_a, M.val0, M.X)
    for T, kind in ((A, "adopted"), (B, "copied")):
        assert_bits(spmv(torch, T, dx), refs()[r0:], "row block, BINNED, %s" % kind)
        assert_bits(spmm(torch, T, M.X, 3, 3, 3), ref_block[r0:], "row block, spmm, %s" % kind)
        T.close()


# ------------------------------------------------------------- 2. inputs are never modified; destroy frees nothing it adopted
def test_adopted_arrays_come_back_unmodified_and_alive(torch, refs):
    tensors = adopt(torch)
    t_host, t_dev = tjds_pair(torch)
    tjds_tensors = (t_dev.perm, t_dev.start_pos, t_dev.row_ind, t_dev.val)
    clones = [t.clone() for t in tensors + tjds_tensors]
    dx, dX = dev(torch, M.x), M.X
    ref = refs()
    for setting in csr_settings():                                     # every plan builder, the ones that sort included
        A = csr_handle(setting, M.rows, M.cols, *tensors)
        assert_bits(spmv(torch, A, dx), ref, setting[0])
        A.close()
    A = sm.CsrMatrix(M.rows, M.cols, *tensors)
    assert_bits(spmm(torch, A, dX, 3, 3, 3), ad.reference(M.row_ptr, M.cols_a, M.val0, M.X), "spmm")
    At = A.transposed()
    A.close()
    At.close()
    for label, T in tjds_paths(t_dev):
        assert_bits(tjds_spmv(torch, T, dx), ref, label)
    for t, c in zip(tensors + tjds_tensors, clones):
        assert bits_equal(torch, t, c), "an adopted array was modified"
    # the arrays are still there after every close(): new handles over them, two alive at once
    A = csr_handle(("COLSWEEP", {}, sm.CSR_KERNEL_COLSWEEP, 0), M.rows, M.cols, *tensors)
    B = csr_handle(("BINNED", {}, sm.CSR_KERNEL_BINNED, 0), M.rows, M.cols, *tensors)
    assert A.get_kernel()[0] == sm.CSR_KERNEL_COLSWEEP and B.get_kernel()[0] == sm.CSR_KERNEL_BINNED
    assert_bits(spmv(torch, A, dx), ref, "COLSWEEP beside BINNED")
    assert_bits(spmv(torch, B, dx), ref, "BINNED beside COLSWEEP")
    assert_bits(spmv(torch, A, dx), ref, "COLSWEEP after BINNED ran")
    A.close()
    assert_bits(spmv(torch, B, dx), ref, "BINNED after the COLSWEEP handle was closed")
    B.close()
    T = sm.TjdsMatrix(t_dev)
    assert_bits(tjds_spmv(torch, T, dx), ref, "a new TJDS handle")
    T.close()
    for t, c in zip(tensors + tjds_tensors, clones):
        assert bits_equal(torch, t, c), "an adopted array was modified"


# --------------------------------------------------------------------------------------------------- 3. val changed in place
def test_val_changed_in_place_is_seen_at_once_where_no_copy_is_kept(torch, refs):
    """smvp_csr_spmm, K8, K9, VECTOR, STREAM, STREAM_CARRY (their copy is of columns only), TJDS ATOMIC and TWO_PHASE read val
    itself: the next product has the new values without any call, and the old ones again after val is put back."""
    d_rp, d_ci, d_v = adopt(torch)
    t_host, t_dev = tjds_pair(torch)
    tv = {"val0": t_host.val.copy(), "val1": tjds_values(M.val1)}
    dx, dx_rows = dev(torch, M.x), dev(torch, M.x_rows)
    csr = []
    for kernel, param in CSR_VARIANTS:
        if kernel in TILE_KERNELS + (sm.CSR_KERNEL_VECTOR,):
            for col16 in ((1, 0) if kernel in TILE_KERNELS else (None,)):
                setting = ("kernel %d param %d, csr_col16 %r" % (kernel, param, col16), {"csr_col16": col16}, kernel, param)
                csr.append((setting[0], csr_handle(setting, M.rows, M.cols, d_rp, d_ci, d_v)))
    names = {label: A.describe()[0] for label, A in csr}                # (the 16-bit offsets are in use where cols_a has them)
    for tile in (1024, 2048):
        with_offsets, without = (names["kernel %d param %d, csr_col16 %d" % (sm.CSR_KERNEL_STREAM, tile, c)] for c in (1, 0))
        assert (with_offsets != without) == ad.offsets_used(M.nnz, M.cols_a, tile) == True, (tile, with_offsets, without)
    S = sm.CsrMatrix(M.rows, M.cols, d_rp, d_ci, d_v)
    tjds = []
    for mode in (sm.TJDS_MODE_ATOMIC, sm.TJDS_MODE_TWO_PHASE):
        T = sm.TjdsMatrix(t_dev)
        T.set_mode(mode)
        T.set_x(dx)                                                    # once: no call on the handle between the products below
        tjds.append(("TJDS mode %d" % mode, T))
    for val in ("val0", "val1", "val0"):
        put(torch, d_v, getattr(M, val))
        put(torch, t_dev.val, tv[val])
        for label, A in csr:
            assert_bits(spmv(torch, A, dx), refs("cols_a", val), "%s (%s), %s in place" % (label, A.describe()[0], val))
        assert_bits(spmm(torch, S, M.X, 3, 3, 3), ad.reference(M.row_ptr, M.cols_a, getattr(M, val), M.X), "spmm, %s in place" % val)
        for label, T in tjds:
            assert_bits(tjds_spmv(torch, T), refs("cols_a", val), "%s (%s), %s in place" % (label, T.describe()[0], val))
            assert_bits(k8(torch, T, dx_rows), ad.reference_t(M.row_ptr, M.cols_a, getattr(M, val), M.x_rows, M.cols), "K8, %s in place" % val)
            assert_bits(k9(torch, T, M.X_rows, ldx=5, ldy=4), ad.reference_t(M.row_ptr, M.cols_a, getattr(M, val), M.X_rows, M.cols),
                        "K9, %s in place" % val)
    for _, H in csr + tjds + [("", S)]:
        H.close()


def test_val_changed_in_place_is_right_after_the_documented_refresh(torch, refs):
    """smvp_csr_set_kernel (same kernel, same param) on every CSR path, smvp_tjds_set_value_cache (same min_tiles) on every
    ROW_GATHER variant -- the tile-overflow values are a copy too -- and re-creation of a TJDS handle."""
    d_rp, d_ci, d_v = adopt(torch)
    t_host, t_dev = tjds_pair(torch)
    dx = dev(torch, M.x)
    settings = csr_settings()
    handles = [csr_handle(s, M.rows, M.cols, d_rp, d_ci, d_v) for s in settings]
    gathers = [(label, gather_handle(t_dev, index, tile, cache), (index, tile, cache)) for label, index, tile, cache in gather_settings()]
    T_old = sm.TjdsMatrix(t_dev)
    before = [state(A) for A in handles] + [(T.describe(), T.get_value_cache()) for _, T, _ in gathers]
    for setting, A in zip(settings, handles):
        assert_bits(spmv(torch, A, dx), refs(), setting[0] + ", before the change")
    for label, T, _ in gathers:
        assert_bits(tjds_spmv(torch, T, dx), refs(), label + ", before the change")
    put(torch, d_v, M.val1)
    put(torch, t_dev.val, tjds_values(M.val1))
    want = refs("cols_a", "val1")
    for setting, A, was in zip(settings, handles, before):
        replan(A, setting)
        fresh = csr_handle(setting, M.rows, M.cols, d_rp, d_ci, d_v)
        y = spmv(torch, A, dx)
        assert_bits(y, want, "%s (%s), re-planned" % (setting[0], A.describe()[0]))
        assert_bits(y, spmv(torch, fresh, dx), "%s, re-planned against fresh" % setting[0])
        assert state(A) == was == state(fresh), setting[0]
        fresh.close()
        A.close()
    for (label, T, (index, tile, cache)), was in zip(gathers, before[len(handles):]):
        T.set_value_cache(cache)
        fresh = gather_handle(t_dev, index, tile, cache)
        y = tjds_spmv(torch, T, dx)
        assert_bits(y, want, "%s (%s), set_value_cache again" % (label, T.describe()[0]))
        assert_bits(y, tjds_spmv(torch, fresh, dx), "%s, refreshed against fresh" % label)
        assert (T.describe(), T.get_value_cache()) == was == (fresh.describe(), fresh.get_value_cache()), label
        fresh.close()
        T.close()
    T_old.close()                                                       # re-creation
    T = sm.TjdsMatrix(t_dev)
    for mode in TJDS_MODES:
        T.set_mode(mode)
        assert_bits(tjds_spmv(torch, T, dx), want, "TJDS mode %d, re-created" % mode)
    T.close()


def test_a_transposed_handle_is_a_copy_of_its_own(torch):
    d_rp, d_ci, d_v = adopt(torch)
    dx_rows = dev(torch, M.x_rows)
    want = {v: ad.reference_t(M.row_ptr, M.cols_a, getattr(M, v), M.x_rows, M.cols) for v in ("val0", "val1")}
    A = sm.CsrMatrix(M.rows, M.cols, d_rp, d_ci, d_v)
    At = A.transposed()
    assert (At.rows, At.cols) == (M.cols, M.rows)
    assert_bits(spmv(torch, At, dx_rows), want["val0"], "A^T x")
    put(torch, d_v, M.val1)
    assert_bits(spmv(torch, At, dx_rows), want["val0"], "A^T x of the handle made before val changed")
    A2t = A.transposed()
    A.close()
    assert_bits(spmv(torch, At, dx_rows), want["val0"], "A^T x of the earlier handle after A.close()")
    assert_bits(spmv(torch, A2t, dx_rows), want["val1"], "A^T x of the handle made after val changed")
    At.close()
    A2t.close()


# ----------------------------------------------------------------------------------------------- 4. col_ind changed in place
def test_col_ind_changed_in_place_a_b_c_a(torch, refs):
    """After each change smvp_csr_set_kernel(same, same) gives the new columns' product, the describe() and the plan bytes of a
    fresh handle; smvp_csr_spmm needs no call.  The STREAM handle with 16-bit offsets goes through: other tiles narrow (a -> b),
    offsets dropped (b -> c), offsets taken up again (c -> a)."""
    d_rp, d_ci, d_v = adopt(torch)
    dx = dev(torch, M.x)
    settings = csr_settings()
    handles = [csr_handle(s, M.rows, M.cols, d_rp, d_ci, d_v) for s in settings]
    S = sm.CsrMatrix(M.rows, M.cols, d_rp, d_ci, d_v)
    assert_bits(spmm(torch, S, M.X, 3, 3, 3), ad.reference(M.row_ptr, M.cols_a, M.val0, M.X), "spmm, cols_a")
    names = {}
    for cols in ("cols_b", "cols_c", "cols_a"):
        put(torch, d_ci, getattr(M, cols))
        want = refs(cols, "val0")
        assert_bits(spmm(torch, S, M.X, 3, 3, 3), ad.reference(M.row_ptr, getattr(M, cols), M.val0, M.X), "spmm, %s in place" % cols)
        for setting, A in zip(settings, handles):
            replan(A, setting)
            fresh = csr_handle(setting, M.rows, M.cols, d_rp, d_ci, d_v)
            what = "%s (%s), %s in place" % (setting[0], A.describe()[0], cols)
            assert_bits(spmv(torch, A, dx), want, what)
            assert_bits(spmv(torch, fresh, dx), want, what + ", fresh")
            assert state(A) == state(fresh), what
            assert A.plan_info()["plan_bytes"] == fresh.plan_info()["plan_bytes"], what
            names[cols, setting[0]] = (A.describe()[0], A.plan_info()["plan_bytes"])
            fresh.close()
    # the offsets were in use on b and a and dropped on c: what the host says of the columns (adopted.offsets_used) shows in the
    # handle as the kernel and the plan bytes of the same setting without offsets
    plain = COL16_STREAM.replace("csr_col16 1", "csr_col16 0")
    for cols in ("cols_b", "cols_c", "cols_a"):
        assert (names[cols, COL16_STREAM] != names[cols, plain]) == ad.offsets_used(M.nnz, getattr(M, cols), 1024), cols
    assert names["cols_b", COL16_STREAM] == names["cols_a", COL16_STREAM] != names["cols_c", COL16_STREAM]
    for H in handles + [S]:
        H.close()


# ------------------------------------------------------------------------------------------------- 5. host_row_ptr = NULL
def raw_create(rows, cols, nnz, rp, ci, v, host_rp=None):
    """smvp_csr_create(SMVP_MEM_DEVICE) through the C ABI with raw device addresses -> (status, handle or None, message)."""
    h = C.c_void_p()
    rc = sm.lib().smvp_csr_create(C.byref(h), 0, rows, cols, nnz, C.c_void_p(rp), C.c_void_p(ci), C.c_void_p(v), sm.MEM_DEVICE, host_rp)
    return rc, h.value, sm.lib().smvp_last_error().decode(errors="replace")


def test_row_ptr_is_read_back_when_no_host_copy_is_given(torch, refs):
    d_rp, d_ci, d_v = adopt(torch)
    dx = dev(torch, M.x)
    rc, h, msg = raw_create(M.rows, M.cols, M.nnz, d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr())
    assert rc == sm.OK and h, msg
    A = sm.CsrMatrix._wrap(C.c_void_p(h), M.rows, M.cols, M.nnz)
    assert_bits(spmv(torch, A, dx), refs(), "host_row_ptr = NULL, AUTO")
    replan(A, ("BINNED", {}, sm.CSR_KERNEL_BINNED, 0))                  # (a plan built from the host copy that was read back)
    assert_bits(spmv(torch, A, dx), refs(), "host_row_ptr = NULL, BINNED")
    A.close()
    bad = M.row_ptr.copy()
    r = M.rows // 2
    bad[r] = bad[r + 1] + 1                                             # decreasing from row r to r + 1; first and last entry intact
    assert bad[r] > bad[r + 1] and bad[0] == 0 and bad[-1] == M.nnz
    d_bad = dev(torch, bad)
    rc, h, msg = raw_create(M.rows, M.cols, M.nnz, d_bad.data_ptr(), d_ci.data_ptr(), d_v.data_ptr())
    assert rc == sm.ERR_INVALID and h is None and "row_ptr" in msg, (rc, h, msg)


# ----------------------------------------------------------------------------------------------------------- 6. alignment
def shifted(torch, a, elements):
    """A copy of `a` on the device that starts `elements` elements past a 16-byte boundary."""
    buf = torch.zeros(len(a) + 8, dtype=torch.from_numpy(np.array(a[:1])).dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[elements:elements + len(a)]
    view.copy_(torch.from_numpy(np.array(a)))
    return view


def test_misaligned_col_ind_or_val_is_refused(torch):
    d_rp, d_ci, d_v = adopt(torch)
    slack = torch.zeros(M.nnz + 8, dtype=torch.float64, device="cuda")   # val 4 bytes off: a raw address inside valid memory
    cases = {"col_ind 4 bytes off": (shifted(torch, M.cols_a, 1).data_ptr(), d_v.data_ptr()),
             "col_ind 8 bytes off": (shifted(torch, M.cols_a, 2).data_ptr(), d_v.data_ptr()),
             "val 8 bytes off": (d_ci.data_ptr(), shifted(torch, M.val0, 1).data_ptr()),
             "val 4 bytes off": (d_ci.data_ptr(), slack.data_ptr() + 4)}
    for what, (ci, v) in cases.items():
        assert (ci % 16, v % 16) != (0, 0)
        rc, h, msg = raw_create(M.rows, M.cols, M.nnz, d_rp.data_ptr(), ci, v, M.row_ptr.ctypes.data_as(C.c_void_p))
        assert rc == sm.ERR_INVALID and h is None and "16-byte aligned" in msg, (what, rc, h, msg)
    with pytest.raises(sm.SmvpError) as e:                               # the wrapper reports the same refusal
        sm.CsrMatrix(M.rows, M.cols, d_rp, shifted(torch, M.cols_a, 1), d_v)
    assert e.value.code == sm.ERR_INVALID and "16-byte aligned" in str(e.value)


def test_row_ptr_needs_no_alignment_beyond_its_own(torch, refs):
    rp = shifted(torch, M.row_ptr, 1)
    _, d_ci, d_v = adopt(torch)
    assert rp.data_ptr() % 16 == 4 and d_ci.data_ptr() % 16 == 0 and d_v.data_ptr() % 16 == 0
    dx = dev(torch, M.x)
    A = sm.CsrMatrix(M.rows, M.cols, rp, d_ci, d_v)
    for setting in (("STREAM", {}, sm.CSR_KERNEL_STREAM, 0), ("STREAM 1024", {}, sm.CSR_KERNEL_STREAM, 1024),
                    ("VECTOR", {}, sm.CSR_KERNEL_VECTOR, 8)):
        replan(A, setting)
        assert_bits(spmv(torch, A, dx), refs(), "row_ptr 4 bytes off, %s (%s)" % (setting[0], A.describe()[0]))
    assert_bits(spmm(torch, A, M.X, 3, 3, 3), ad.reference(M.row_ptr, M.cols_a, M.val0, M.X), "row_ptr 4 bytes off, spmm")
    A.close()


def test_tjds_arrays_need_no_alignment_beyond_their_own(torch, refs):
    """smvp_tjds_create has no alignment check and needs none: val 8 bytes past a 16-byte boundary, row_ind, perm and start_pos
    4 bytes past one, in every mode and on K8 and K9."""
    t_host, _ = tjds_pair(torch)
    t = SimpleNamespace(**{k: getattr(t_host, k) for k in ("rows", "cols", "nnz", "num_diag", "ref_num_tjdiag", "last_diag_single")})
    t.val, t.row_ind = shifted(torch, t_host.val, 1), shifted(torch, t_host.row_ind, 1)
    t.perm, t.start_pos = shifted(torch, t_host.perm, 1), shifted(torch, t_host.start_pos, 1)
    assert t.val.data_ptr() % 16 == 8 and all(a.data_ptr() % 16 == 4 for a in (t.row_ind, t.perm, t.start_pos))
    dx, dx_rows = dev(torch, M.x), dev(torch, M.x_rows)
    T = sm.TjdsMatrix(t)
    for mode in TJDS_MODES:
        T.set_mode(mode)
        assert_bits(tjds_spmv(torch, T, dx), refs(), "misaligned TJDS arrays, mode %d (%s)" % (mode, T.describe()[0]))
    assert_bits(k8(torch, T, dx_rows), ad.reference_t(M.row_ptr, M.cols_a, M.val0, M.x_rows, M.cols), "misaligned TJDS arrays, K8")
    assert_bits(k9(torch, T, M.X_rows, ldx=5, ldy=4), ad.reference_t(M.row_ptr, M.cols_a, M.val0, M.X_rows, M.cols), "misaligned TJDS arrays, K9")
    T.close()


# ---------------------------------------------------------------------------------------- 7. AUTO after a change of columns
def test_auto_chooses_for_the_columns_that_are_there_now(torch):
    """smvp_csr_set_kernel(AUTO) after col_ind changed in place measures again: the kernel, the gather spread and the far share
    are those of a fresh handle over the same arrays, going from a band (STREAM) to scattered columns and back."""
    P = ad.auto_pair()
    d_rp, d_ci, d_v = dev(torch, P.row_ptr), dev(torch, P.band3), dev(torch, P.val)
    dx = dev(torch, P.x)
    auto = ("AUTO", {}, sm.CSR_KERNEL_AUTO, 0)

    def figures(H):
        return H.get_kernel(), H.gather_spread(), H.far_share()

    A = sm.CsrMatrix(P.rows, P.cols, d_rp, d_ci, d_v)
    assert A.get_kernel()[0] == sm.CSR_KERNEL_STREAM and 0 <= A.gather_spread() < 0.2
    assert_bits(spmv(torch, A, dx), ad.reference(P.row_ptr, P.band3, P.val, P.x), "band3")
    seen = {"band3": figures(A)}
    for cols in ("scattered3", "band3"):
        put(torch, d_ci, getattr(P, cols))
        replan(A, auto)
        fresh = sm.CsrMatrix(P.rows, P.cols, d_rp, d_ci, d_v)
        print("AUTO on %s: re-planned %r, fresh %r (%s)" % (cols, figures(A), figures(fresh), fresh.describe()[0]))
        assert figures(A) == figures(fresh), cols
        assert state(A) == state(fresh), cols
        assert_bits(spmv(torch, A, dx), ad.reference(P.row_ptr, getattr(P, cols), P.val, P.x), cols + ", re-planned")
        seen.setdefault(cols, figures(A))
        assert seen[cols] == figures(A)
        fresh.close()
    assert seen["scattered3"][0] != seen["band3"][0]                   # (the two matrices do not resolve to the same kernel)
    A.close()
