"""The block transposed product Y = A^T X (smvp_tjds_spmm_transposed, K9) on the host: its two entry points are declared,
bound and exported, refuse a NULL handle without a device, and TjdsMatrix.spmm_transposed refuses on CPU tensors what
sm.spmm_operands refuses -- X has `rows` rows and Y has `cols` rows, the conventions of CsrMatrix.spmm with the rows and
columns of A changing places."""
import ctypes as C
import os
import re
import subprocess

import pytest

import smvp_toolkit_amd as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("smvp_tjds_spmm_transposed", "smvp_tjds_spmm_transposed_describe")


def test_spmm_transposed_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(sm.lib(), name).argtypes is not None, name
    vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
    assert sm.lib().smvp_tjds_spmm_transposed.argtypes == [vp, ci, vp, ll, vp, ll, vp]
    assert sm.lib().smvp_tjds_spmm_transposed_describe.argtypes == [vp, ci, C.c_char_p, C.c_size_t, C.POINTER(C.c_double)]
    for method in ("spmm_transposed", "spmm_transposed_describe"):
        assert callable(getattr(sm.TjdsMatrix, method)), method


def test_spmm_transposed_null_handles_are_invalid_without_a_device():
    L = sm.lib()
    x, y = (C.c_double * 16)(), (C.c_double * 16)()
    assert L.smvp_tjds_spmm_transposed(None, 2, C.cast(x, C.c_void_p), 2, C.cast(y, C.c_void_p), 2, None) == sm.ERR_INVALID
    assert "smvp_tjds_spmm_transposed:" in L.smvp_last_error().decode()
    name = C.create_string_buffer(b"untouched", 64)
    b = C.c_double(-1.0)
    assert L.smvp_tjds_spmm_transposed_describe(None, 2, name, 64, C.byref(b)) == sm.ERR_INVALID
    assert "smvp_tjds_spmm_transposed_describe" in L.smvp_last_error().decode()
    assert b.value == -1.0 and name.value == b"untouched"


def handle_without_a_device(rows, cols):
    """A TjdsMatrix that holds no handle: the binding checks its operands before it touches the library."""
    T = sm.TjdsMatrix.__new__(sm.TjdsMatrix)
    T.rows, T.cols, T.nnz, T._t, T._h = rows, cols, 0, None, C.c_void_p()
    return T


def test_spmm_transposed_takes_what_spmm_operands_takes_up_to_the_device_check():
    torch = pytest.importorskip("torch")
    f64 = torch.float64
    T = handle_without_a_device(5, 7)
    for X, Y in ((torch.zeros(5, 3, dtype=f64), torch.zeros(7, 3, dtype=f64)),
                 (torch.zeros(5, 8, dtype=f64)[:, :3], torch.zeros(7, 4, dtype=f64)[:, 1:4]),       # column slices of wider arrays
                 (torch.zeros(5, 1, dtype=f64), torch.zeros(7, 1, dtype=f64))):
        assert sm.spmm_operands(X, Y, T.cols, T.rows) == (X.shape[1], X.stride(0), Y.stride(0))
        with pytest.raises(ValueError, match="device tensors"):      # the operands pass; CPU tensors stop at the device check
            T.spmm_transposed(X, Y)


@pytest.mark.parametrize("case", ["X with cols rows", "Y with rows rows", "1-D X", "1-D Y", "float32 X", "float32 Y", "differing k",
                                  "k = 0", "column-major X", "column-major Y", "strided X", "strided Y"])
def test_spmm_transposed_refuses_what_spmm_operands_refuses(case):
    torch = pytest.importorskip("torch")
    f64 = torch.float64
    rows, cols, k = 5, 7, 3
    X, Y = torch.zeros(rows, k, dtype=f64), torch.zeros(cols, k, dtype=f64)
    if case == "X with cols rows":
        X = torch.zeros(cols, k, dtype=f64)
    elif case == "Y with rows rows":
        Y = torch.zeros(rows, k, dtype=f64)
    elif case == "1-D X":
        X = torch.zeros(rows, dtype=f64)
    elif case == "1-D Y":
        Y = torch.zeros(cols, dtype=f64)
    elif case == "float32 X":
        X = X.to(torch.float32)
    elif case == "float32 Y":
        Y = Y.to(torch.float32)
    elif case == "differing k":
        Y = torch.zeros(cols, k + 1, dtype=f64)
    elif case == "k = 0":
        X, Y = torch.zeros(rows, 0, dtype=f64), torch.zeros(cols, 0, dtype=f64)
    elif case == "column-major X":
        X = torch.zeros(k, rows, dtype=f64).t()
    elif case == "column-major Y":
        Y = torch.zeros(k, cols, dtype=f64).t()
    elif case == "strided X":
        X = torch.zeros(rows, 2 * k, dtype=f64)[:, ::2]
    else:
        Y = torch.zeros(cols, 2 * k, dtype=f64)[:, ::2]
    with pytest.raises(ValueError) as by_check:
        sm.spmm_operands(X, Y, cols, rows)
    with pytest.raises(ValueError) as by_method:
        handle_without_a_device(rows, cols).spmm_transposed(X, Y)
    assert str(by_method.value) == str(by_check.value) and "device tensors" not in str(by_method.value)
