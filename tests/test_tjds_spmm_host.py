"""The forward block product from a TJDS handle Y = A X (smvp_tjds_spmm, K10) on the host: its two entry points are declared,
bound and exported, refuse a NULL handle without a device, and TjdsMatrix.spmm refuses on CPU tensors what sm.spmm_operands
refuses -- X has `cols` rows and Y has `rows` rows, the conventions of CsrMatrix.spmm.  The reference of the GPU tests
(tests/tjds_spmm.py) is pinned against a plain Python loop over the TJDS arrays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import smvp_toolkit_amd as sm
import tjds_spmm as tk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("smvp_tjds_spmm", "smvp_tjds_spmm_describe")


def test_tjds_spmm_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(sm.lib(), name).argtypes is not None, name
    vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
    assert sm.lib().smvp_tjds_spmm.argtypes == [vp, ci, vp, ll, vp, ll, vp]
    assert sm.lib().smvp_tjds_spmm_describe.argtypes == [vp, ci, C.c_char_p, C.c_size_t, C.POINTER(C.c_double), C.POINTER(sm.PlanInfo)]
    for method in ("spmm", "spmm_describe"):
        assert callable(getattr(sm.TjdsMatrix, method)), method


def test_tjds_spmm_null_handles_are_invalid_without_a_device():
    L = sm.lib()
    x, y = (C.c_double * 16)(), (C.c_double * 16)()
    assert L.smvp_tjds_spmm(None, 2, C.cast(x, C.c_void_p), 2, C.cast(y, C.c_void_p), 2, None) == sm.ERR_INVALID
    assert L.smvp_last_error().decode().startswith("smvp_tjds_spmm:")
    name = C.create_string_buffer(b"untouched", 64)
    b = C.c_double(-1.0)
    info = sm.PlanInfo(-2.0, -3.0, -4.0)
    assert L.smvp_tjds_spmm_describe(None, 2, name, 64, C.byref(b), C.byref(info)) == sm.ERR_INVALID
    assert "smvp_tjds_spmm_describe" in L.smvp_last_error().decode()
    assert b.value == -1.0 and name.value == b"untouched"
    assert (info.matrix_bytes, info.plan_bytes, info.build_ms) == (-2.0, -3.0, -4.0)
    assert L.smvp_tjds_spmm_describe(None, 2, None, 0, None, None) == sm.ERR_INVALID


def handle_without_a_device(rows, cols):
    """A TjdsMatrix that holds no handle: the binding checks its operands before it touches the library."""
    T = sm.TjdsMatrix.__new__(sm.TjdsMatrix)
    T.rows, T.cols, T.nnz, T._t, T._h = rows, cols, 0, None, C.c_void_p()
    return T


def test_tjds_spmm_takes_what_spmm_operands_takes_up_to_the_device_check():
    torch = pytest.importorskip("torch")
    f64 = torch.float64
    T = handle_without_a_device(5, 7)
    for X, Y in ((torch.zeros(7, 3, dtype=f64), torch.zeros(5, 3, dtype=f64)),
                 (torch.zeros(7, 8, dtype=f64)[:, :3], torch.zeros(5, 4, dtype=f64)[:, 1:4]),       # column slices of wider arrays
                 (torch.zeros(7, 1, dtype=f64), torch.zeros(5, 1, dtype=f64))):
        assert sm.spmm_operands(X, Y, T.rows, T.cols) == (X.shape[1], X.stride(0), Y.stride(0))
        with pytest.raises(ValueError, match="device tensors"):      # the operands pass; CPU tensors stop at the device check
            T.spmm(X, Y)


@pytest.mark.parametrize("case", ["X with rows rows", "Y with cols rows", "1-D X", "1-D Y", "float32 X", "float32 Y", "differing k",
                                  "k = 0", "column-major X", "column-major Y", "strided X", "strided Y"])
def test_tjds_spmm_refuses_what_spmm_operands_refuses(case):
    torch = pytest.importorskip("torch")
    f64 = torch.float64
    rows, cols, k = 5, 7, 3
    X, Y = torch.zeros(cols, k, dtype=f64), torch.zeros(rows, k, dtype=f64)
    if case == "X with rows rows":
        X = torch.zeros(rows, k, dtype=f64)
    elif case == "Y with cols rows":
        Y = torch.zeros(cols, k, dtype=f64)
    elif case == "1-D X":
        X = torch.zeros(cols, dtype=f64)
    elif case == "1-D Y":
        Y = torch.zeros(rows, dtype=f64)
    elif case == "float32 X":
        X = X.to(torch.float32)
    elif case == "float32 Y":
        Y = Y.to(torch.float32)
    elif case == "differing k":
        Y = torch.zeros(rows, k + 1, dtype=f64)
    elif case == "k = 0":
        X, Y = torch.zeros(cols, 0, dtype=f64), torch.zeros(rows, 0, dtype=f64)
    elif case == "column-major X":
        X = torch.zeros(k, cols, dtype=f64).t()
    elif case == "column-major Y":
        Y = torch.zeros(k, rows, dtype=f64).t()
    elif case == "strided X":
        X = torch.zeros(cols, 2 * k, dtype=f64)[:, ::2]
    else:
        Y = torch.zeros(rows, 2 * k, dtype=f64)[:, ::2]
    with pytest.raises(ValueError) as by_check:
        sm.spmm_operands(X, Y, rows, cols)
    with pytest.raises(ValueError) as by_method:
        handle_without_a_device(rows, cols).spmm(X, Y)
    assert str(by_method.value) == str(by_check.value) and "device tensors" not in str(by_method.value)


def python_loop(t, x):
    """The definition itself, in plain Python: every row's entries in ascending TJDS position, acc += val * x[perm[k]]."""
    y = [0.0] * t.rows
    for d in range(t.num_diag):
        for j in range(int(t.start_pos[d]), int(t.start_pos[d + 1])):
            y[int(t.row_ind[j])] += float(t.val[j]) * float(x[int(t.perm[j - int(t.start_pos[d])])])
    return np.array(y, dtype=np.float64)


def test_reference_block_is_the_definition_on_every_column():
    """Repeated pairs with values that tell the orders apart, empty rows, and a sample matrix: the oracle's loop column by column
    has the bits of the plain loop, and differs from the sum in CSR order where the two orders differ."""
    coo = sm.make_coo([0, 2, 2, 2, 3, 2], [0, 1, 1, 1, 1, 0], [4.0, 1e16, 1.0, -1e16, 0.5, 3.0])
    t = sm.tjds_from_coo(coo, 5, 3)
    X = np.stack([np.ones(3), np.array([1.0, 2.0, -1.0]), -np.ones(3)], axis=1)
    ref = tk.reference_block(t, X)
    assert ref.shape == (5, 3)
    for v in range(3):
        tk.tr.assert_bits(ref[:, v], python_loop(t, X[:, v]), "vector %d" % v)
    assert (ref[[1, 4]].view(np.int64) == 0).all()
    _, m, n, coo = sm.mm_read_coo(ob.fixture_path("curtis54.mtx"))
    t = sm.tjds_from_coo(coo, m, n)
    X = np.random.default_rng(1).standard_normal((n, 2))
    ref = tk.reference_block(t, X)
    for v in range(2):
        tk.tr.assert_bits(ref[:, v], python_loop(t, X[:, v]), "curtis54, vector %d" % v)
    with pytest.raises(AssertionError):
        tk.assert_block(ref + 1.0, ref, "a block that differs")
    assert tk.reference_block(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 4), np.ones((4, 2))).shape == (0, 2)
