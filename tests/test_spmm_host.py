"""smvp_csr_spmm on the host: the two entry points are declared, bound and exported, refuse a NULL handle without a device,
and the binding's shape / stride checks (sm.spmm_operands) accept exactly the row-major operands the C call takes."""
import ctypes as C
import os
import re
import subprocess

import pytest

import smvp_toolkit_amd as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("smvp_csr_spmm", "smvp_csr_spmm_describe")


def test_spmm_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(sm.lib(), name).argtypes is not None, name


def test_spmm_null_handle_is_invalid_without_a_device():
    L = sm.lib()
    x, y = (C.c_double * 8)(), (C.c_double * 8)()
    assert L.smvp_csr_spmm(None, 1, C.cast(x, C.c_void_p), 1, C.cast(y, C.c_void_p), 1, None) == sm.ERR_INVALID
    assert "smvp_csr_spmm" in L.smvp_last_error().decode()
    name = C.create_string_buffer(64)
    b = C.c_double(-1.0)
    info = sm.PlanInfo()
    assert L.smvp_csr_spmm_describe(None, 8, name, 64, C.byref(b), C.byref(info)) == sm.ERR_INVALID
    assert "smvp_csr_spmm_describe" in L.smvp_last_error().decode()
    assert L.smvp_csr_spmm_describe(None, 8, None, 0, None, None) == sm.ERR_INVALID


def test_spmm_operands_accepts_row_major_operands():
    torch = pytest.importorskip("torch")
    X = torch.zeros(7, 3, dtype=torch.float64)
    Y = torch.zeros(5, 3, dtype=torch.float64)
    assert sm.spmm_operands(X, Y, 5, 7) == (3, 3, 3)
    Xw, Yw = torch.zeros(7, 9, dtype=torch.float64), torch.zeros(5, 12, dtype=torch.float64)
    assert sm.spmm_operands(Xw[:, 2:5], Yw[:, 4:7], 5, 7) == (3, 9, 12)     # column slices of wider arrays
    x1 = torch.zeros(7, dtype=torch.float64)
    assert sm.spmm_operands(x1[:, None], torch.zeros(5, 1, dtype=torch.float64), 5, 7) == (1, 1, 1)
    assert sm.spmm_operands(torch.zeros(0, 2, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64), 4, 0)[0] == 2


@pytest.mark.parametrize("case", ["1-D X", "float32 Y", "X rows", "Y rows", "k differs", "k = 0", "column-major X",
                                  "strided Y", "not a tensor"])
def test_spmm_operands_refuses_what_the_c_call_cannot_take(case):
    torch = pytest.importorskip("torch")
    f64 = torch.float64
    X, Y = torch.zeros(7, 3, dtype=f64), torch.zeros(5, 3, dtype=f64)
    if case == "1-D X":
        X = torch.zeros(7, dtype=f64)
    elif case == "float32 Y":
        Y = torch.zeros(5, 3, dtype=torch.float32)
    elif case == "X rows":
        X = torch.zeros(6, 3, dtype=f64)
    elif case == "Y rows":
        Y = torch.zeros(4, 3, dtype=f64)
    elif case == "k differs":
        Y = torch.zeros(5, 2, dtype=f64)
    elif case == "k = 0":
        X, Y = torch.zeros(7, 0, dtype=f64), torch.zeros(5, 0, dtype=f64)
    elif case == "column-major X":
        X = torch.zeros(3, 7, dtype=f64).t()
    elif case == "strided Y":
        Y = torch.zeros(5, 6, dtype=f64)[:, ::2]
    else:
        X = [[0.0] * 3] * 7
    with pytest.raises(ValueError):
        sm.spmm_operands(X, Y, 5, 7)
