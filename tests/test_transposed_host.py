"""The transposed product on the host: the four entry points are declared, bound and exported, refuse a NULL handle without
a device, the binding's operand checks (sm.transposed_operands) accept exactly what the C call takes, and the reference the
GPU tests compare with (tests/transposed.py) equals the definition written as a plain Python loop."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import smvp_toolkit_amd as sm
import transposed as tr
from conftest import SAMPLES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("smvp_tjds_spmv_transposed", "smvp_tjds_transposed_describe", "smvp_csr_create_transposed", "smvp_csr_device_arrays")


def test_transposed_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(sm.lib(), name).argtypes is not None, name
    for cls, method in ((sm.TjdsMatrix, "spmv_transposed"), (sm.TjdsMatrix, "transposed_describe"), (sm.CsrMatrix, "transposed"),
                        (sm.CsrMatrix, "device_arrays")):
        assert callable(getattr(cls, method)), method


def test_transposed_null_handles_are_invalid_without_a_device():
    L = sm.lib()
    x, y = (C.c_double * 8)(), (C.c_double * 8)()
    assert L.smvp_tjds_spmv_transposed(None, C.cast(x, C.c_void_p), C.cast(y, C.c_void_p), None) == sm.ERR_INVALID
    assert "smvp_tjds_spmv_transposed" in L.smvp_last_error().decode()
    name = C.create_string_buffer(64)
    b = C.c_double(-1.0)
    assert L.smvp_tjds_transposed_describe(None, name, 64, C.byref(b)) == sm.ERR_INVALID
    assert "smvp_tjds_transposed_describe" in L.smvp_last_error().decode()
    assert b.value == -1.0
    out = C.c_void_p(12345)
    assert L.smvp_csr_create_transposed(C.byref(out), None, None) == sm.ERR_INVALID
    assert "smvp_csr_create_transposed" in L.smvp_last_error().decode()
    assert not out.value, "*out must be NULL after a failure"
    assert L.smvp_csr_create_transposed(None, None, None) == sm.ERR_INVALID
    assert "smvp_csr_create_transposed" in L.smvp_last_error().decode()
    rp, ci, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.smvp_csr_device_arrays(None, C.byref(rp), C.byref(ci), C.byref(v)) == sm.ERR_INVALID
    assert "smvp_csr_device_arrays" in L.smvp_last_error().decode()


def test_transposed_operands_accepts_contiguous_float64_of_the_right_length():
    torch = pytest.importorskip("torch")
    f64 = torch.float64
    sm.transposed_operands(torch.zeros(5, dtype=f64), torch.zeros(7, dtype=f64), 5, 7)
    sm.transposed_operands(torch.zeros(0, dtype=f64), torch.zeros(7, dtype=f64), 0, 7)
    sm.transposed_operands(torch.zeros(5, dtype=f64), torch.zeros(0, dtype=f64), 5, 0)
    wide = torch.zeros(40, dtype=f64)
    sm.transposed_operands(wide[3:8], wide[20:27], 5, 7)                 # contiguous slices of a larger buffer
    sm.transposed_operands(torch.zeros(5, 1, dtype=f64), torch.zeros(1, 7, dtype=f64), 5, 7)   # numel and contiguity are what count


@pytest.mark.parametrize("case", ["x short", "x long", "y short", "float32 x", "float32 y", "strided x", "strided y",
                                  "x not a tensor", "y is numpy"])
def test_transposed_operands_refuses_what_the_c_call_cannot_take(case):
    torch = pytest.importorskip("torch")
    f64 = torch.float64
    x, y = torch.zeros(5, dtype=f64), torch.zeros(7, dtype=f64)
    if case == "x short":
        x = torch.zeros(4, dtype=f64)
    elif case == "x long":
        x = torch.zeros(7, dtype=f64)
    elif case == "y short":
        y = torch.zeros(5, dtype=f64)
    elif case == "float32 x":
        x = torch.zeros(5, dtype=torch.float32)
    elif case == "float32 y":
        y = torch.zeros(7, dtype=torch.float32)
    elif case == "strided x":
        x = torch.zeros(10, dtype=f64)[::2]
    elif case == "strided y":
        y = torch.zeros(7, 2, dtype=f64)[:, 0]
    elif case == "x not a tensor":
        x = [0.0] * 5
    else:
        y = np.zeros(7)
    with pytest.raises(ValueError):
        sm.transposed_operands(x, y, 5, 7)


@pytest.mark.parametrize("operand", ["ones", "normal"])
@pytest.mark.parametrize("name", SAMPLES)
def test_reference_helper_equals_the_definition_as_a_python_loop(name, operand):
    """Passes without the feature: it pins what the GPU checks rest on, independently of the library's converter."""
    tc, m, n, coo = sm.mm_read_coo(ob.fixture_path(name))
    x = np.ones(m) if operand == "ones" else np.random.default_rng(21).standard_normal(m)
    want = tr.python_loop(coo, n, x)
    tr.assert_bits(tr.reference(coo, m, n, x), want, "%s %s" % (name, operand))
    # and with the entries shuffled: the column's order is (row, input index), whatever the list's order
    shuffled = coo[np.random.default_rng(22).permutation(len(coo))]
    tr.assert_bits(tr.reference(shuffled, m, n, x), tr.python_loop(shuffled, n, x), "%s %s shuffled" % (name, operand))


def test_reference_helper_keeps_repeated_pairs_in_input_order():
    # (0, 0) three times: 1e16 + 1 - 1e16 is 0 in this order and 1 with the small value last
    coo = sm.make_coo([0, 0, 0, 1], [0, 0, 0, 1], [1e16, 1.0, -1e16, 3.0])
    x = np.ones(2)
    tr.assert_bits(tr.reference(coo, 2, 2, x), np.array([0.0, 3.0]), "storage order")
    tr.assert_bits(tr.reference(coo[[0, 2, 1, 3]], 2, 2, x), np.array([1.0, 3.0]), "another order")
    tr.assert_bits(tr.python_loop(coo, 2, x), np.array([0.0, 3.0]), "python loop")
