"""GPU: the scaled power method on a handle (smvp_csr_power_method / smvp_tjds_power_method, kernel K11) against its numpy
restatement tests/power_method.py (test_power_method_host.py pins that to the oracle and to known answers).

No tolerance anywhere.  The restatement's product argument is the SAME handle's single product, so on every path whose product is
the same from run to run -- every CSR family, TJDS ROW_GATHER and TWO_PHASE -- steps, reason, index, scale, both histories and every
bit of d_x have one right answer.  Comparisons are transposed.assert_bits on the uint64 views (signed zeros count, any NaN equals any
NaN: the header leaves a NaN's sign and payload open).  Every call goes through power() below, which writes d_x into a guarded
buffer, checks the guards, and checks that the histories keep a sentinel beyond the steps done.

The reduce pass's grid is capped at 2048 workgroups of 256 lanes (kPowerGridCap, smvp_power.hip): one grid trip reads
pm.REDUCE_TRIP = 524288 elements, which is power_iteration.PEAK_LARGE's size less one."""
import ctypes as C
import functools

import numpy as np
import pytest

import power_iteration as pi
import power_method as pm
import smvp_toolkit_amd as sm
from parity import check_guards, guarded_y
from test_gpu_parity import CSR_VARIANTS
from test_gpu_transposed import inner_csr_handle
from transposed import assert_bits

pytestmark = pytest.mark.gpu

AUTO = (sm.CSR_KERNEL_AUTO, 0)
PATHS = [("csr",) + kp for kp in [AUTO] + CSR_VARIANTS] + [("tjds", sm.TJDS_MODE_ROW_GATHER, 0), ("tjds", sm.TJDS_MODE_TWO_PHASE, 0)]
BOTH = [("csr",) + AUTO, ("tjds", sm.TJDS_MODE_ROW_GATHER, 0)]
BIT_MATRICES = [("peak", pi.PEAK_SMALL[0], p, s) for p in pi.PEAK_SMALL[1] for s in (1, -1)] + \
               [("short",), ("long",), ("shuffled",), ("sym",), ("tiny_integers",)]
SENTINEL = -12345.678
assert pi.PEAK_LARGE == (pm.REDUCE_TRIP + 1, (pm.REDUCE_TRIP - 1, pm.REDUCE_TRIP))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def matrix(name, *args):
    """The matrices of power_iteration.py and power_method.py, built once and left unchanged."""
    return getattr(pm if hasattr(pm, name) else pi, name)(*args)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def fn_of(H):
    return "smvp_csr_power_method" if isinstance(H, sm.CsrMatrix) else "smvp_tjds_power_method"


# ----------------------------------------------------------------------------------- a handle and its single product, numpy to numpy
def handle(torch, M, fmt, a, b):
    """(handle, product): a CsrMatrix on kernel a / param b, or a TjdsMatrix in mode a; product(x) is one product of that handle,
    remembered by operand (the restatement asks for the same products again with every tol and check_every)."""
    if fmt == "csr":
        H = sm.CsrMatrix(M.n, M.n, *M.csr)
        if (a, b) != AUTO:
            H.set_kernel(a, b)
    else:
        H = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
        H.set_mode(a)
    seen = {}

    def product(x):
        key = np.ascontiguousarray(x, dtype=np.float64).tobytes()
        if key not in seen:
            dx = dev(torch, x)
            buf, dy = guarded_y(torch, M.n)
            if fmt == "csr":
                H.spmv(dx, dy)
            else:
                H.set_x(dx)
                H.zero_y(dy)
                H.spmv(dy)
            torch.cuda.synchronize()
            check_guards(buf, M.n)
            seen[key] = dy.cpu().numpy()
        return seen[key].copy()

    return H, product


def power(torch, H, n, x0, max_steps, tol=0.0, every=1, stream=None, alias=False, before=None):
    """One call through the C ABI -> (steps, reason, index, lambda_each, residual_each, scale, x), as power_method.run returns
    them.  alias: d_x is d_x0.  Nothing is synchronised after the call: it returns when the work has finished.
    before: called in place of the leading torch.cuda.synchronize() with the call's device vectors (stream_order.solver_hook puts
    them in flight on `stream`)."""
    buf, dx = guarded_y(torch, n)
    d0 = None
    if x0 is not None and alias:
        dx.copy_(torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)))
        d0 = dx
    elif x0 is not None:
        d0 = dev(torch, x0)
    o, r = sm.power_opts(max_steps, tol, every), sm.PowerResult()
    lam, res = np.full(max_steps, SENTINEL), np.full(max_steps, SENTINEL)
    if before is None:
        torch.cuda.synchronize()
    else:
        before(x=dx, x0=d0)
    rc = getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(d0), sm._dev_ptr(dx), C.byref(r), sm._p(lam), sm._p(res),
                                     sm._stream_ptr(stream))
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    x = dx.cpu().numpy()
    check_guards(buf, n)
    assert 0 <= r.steps <= max_steps
    assert (lam[r.steps:] == SENTINEL).all() and (res[r.steps:] == SENTINEL).all(), "a history was written beyond the steps done"
    assert not (lam[:r.steps] == SENTINEL).any() and not (res[:r.steps] == SENTINEL).any(), "a step's history was not filled"
    return r.steps, r.reason, r.index, lam[:r.steps], res[:r.steps], np.float64(r.scale), x


def same(got, want, what):
    """steps, reason, index; scale, both histories and every bit of x."""
    assert tuple(got[:3]) == tuple(want[:3]), "%s: (steps, reason, index) = %r, the restatement has %r" % (what, got[:3], want[:3])
    assert_bits([got[5]], [want[5]], what + ": scale")
    assert_bits(got[3], want[3], what + ": lambda_each")
    assert_bits(got[4], want[4], what + ": residual_each")
    assert_bits(got[6], want[6], what + ": d_x")


# ===================================================================================================== 1. bits against run()
@pytest.mark.parametrize("fmt,a,b", PATHS)
def test_every_number_is_the_restatements_on_every_reproducible_path(torch, fmt, a, b):
    for spec in BIT_MATRICES:
        M = matrix(*spec)
        H, product = handle(torch, M, fmt, a, b)
        x0 = pi.ones(M)
        for tol in (0.0, 1e-9):
            for every in (1, 4):
                what = "%s, %s %d %d, tol %g, check_every %d" % (spec, fmt, a, b, tol, every)
                want = pm.run(product, x0, 25, tol, every)
                same(power(torch, H, M.n, x0, 25, tol, every), want, what)
                if spec[0] in ("peak", "sym") and tol:
                    assert want[1] == pm.CONVERGED and want[0] < 25, "%s: the restatement did not converge" % what
        H.close()


def test_the_result_block_is_the_last_steps(torch):
    """eigenvalue, residual, scale and index of the result are those of the step the run stopped at, through the Python method."""
    M = matrix("sym")
    H, product = handle(torch, M, "csr", *AUTO)
    want = pm.run(product, pi.ones(M), 25, 1e-9, 4)
    dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
    r, lam, res = H.power_method(None, dx, 25, tol=1e-9, check_every=4)
    assert (r.steps, r.reason, r.index) == want[:3] and r.steps % 4 == 0 and r.reason == sm.POWER_CONVERGED
    assert len(lam) == len(res) == r.steps
    assert_bits([r.eigenvalue, r.residual, r.scale], [want[3][-1], want[4][-1], want[5]], "the result block")
    assert_bits(lam, want[3], "lambda_each")
    assert_bits(dx.cpu().numpy(), want[6], "d_x")
    H.close()


# ==================================================================================================== 2. the reduce pass's grid
@pytest.mark.parametrize("p", pi.PEAK_LARGE[1])
@pytest.mark.parametrize("sign", [1, -1])
def test_a_peak_on_either_side_of_the_first_grid_trip(torch, p, sign):
    """n = one element past the reduce pass's first grid trip; the largest magnitude on the trip's last element and on the only
    element of the second trip.  A reduce that dropped either names another index, and every number after it changes."""
    M = matrix("peak", pi.PEAK_LARGE[0], p, sign)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = pm.run(product, pi.ones(M), 8, 1e-2)
        assert want[2] == p and want[3][-1] == 3.0 * sign and want[1] == pm.CONVERGED
        same(power(torch, H, M.n, pi.ones(M), 8, 1e-2), want, "peak of %d at %d, sign %d, %s" % (M.n, p, sign, fmt))
        H.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_a_wavefront_and_a_workgroup(torch, n):
    M = matrix("edge", n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        for every in (1, 4):
            want = pm.run(product, pi.ones(M), 9, 1e-9, every)
            assert want[2] == (n - 1 if want[0] > 1 else 0)
            same(power(torch, H, M.n, pi.ones(M), 9, 1e-9, every), want, "edge(%d), %s, check_every %d" % (n, fmt, every))
        H.close()


# ============================================================================================================================ 3. ties
@pytest.mark.parametrize("sign", [-1.0, 1.0])
def test_equal_magnitudes_across_lanes_waves_and_workgroups_go_to_the_smallest_index(torch, sign):
    M, x0 = pm.tie_case(sign)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = pm.run(product, x0, 4)
        got = power(torch, H, M.n, x0, 4)
        same(got, want, "ties, first sign %g, %s" % (sign, fmt))
        assert got[2] == pm.TIE_AT[0] and (got[3] == 2.0 * sign).all() and got[5] == 2.0
        for k in (1, 2, 3):                                                          # ... at every step, not only the last
            assert power(torch, H, M.n, x0, k)[2] == pm.TIE_AT[0]
        H.close()


# ================================================================================================================ 4. special classes
def special_cases():
    S = matrix("short")
    M, x = pi.nan_case()
    yield "nan", M, x, None
    M, x, q = pi.overflow_case()
    yield "overflow", M, x, None
    M, x = pi.subnormal_case()
    yield "subnormal", M, x, None
    Z = matrix("square_zero")
    yield "square_zero", Z, pi.ones(Z), (2, pm.ZERO, None)
    yield "zero start vector", S, np.zeros(S.n), (1, pm.NONFINITE, 0)
    yield "all-NaN start vector", S, np.full(S.n, np.nan), (1, pm.NONFINITE, -1)


def test_nan_infinite_subnormal_and_vanishing_iterates(torch):
    for name, M, x0, expect in special_cases():
        for fmt, a, b in BOTH:
            H, product = handle(torch, M, fmt, a, b)
            for every in (1, 3):
                what = "%s, %s, check_every %d" % (name, fmt, every)
                want = pm.run(product, x0, 6, 0.0, every)
                got = power(torch, H, M.n, x0, 6, 0.0, every)
                same(got, want, what)
                if expect and every == 1:
                    assert got[:2] == expect[:2] and (expect[2] is None or got[2] == expect[2]), "%s: %r" % (what, got[:3])
            H.close()
    Z = matrix("square_zero")                               # the iterate vanished at step 2, nobody looked: step 3 divides 0 by 0
    H, product = handle(torch, Z, "csr", *AUTO)
    assert power(torch, H, Z.n, pi.ones(Z), 10, 0.0, 3)[:3] == (3, pm.NONFINITE, 0)
    H.close()


# ======================================================================================== 5. the iterates are iterate + normalize's
def test_the_iterates_are_those_of_iterate_and_normalize(torch):
    M = matrix("short")
    H, product = handle(torch, M, "csr", *AUTO)
    T, _ = handle(torch, M, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    for x0, x_arg in ((pi.ones(M), None), (pi.random_x(M), pi.random_x(M))):
        for k in pi.STEPS:
            y, ms, st = sm.csr_compute(M.coo, M.n, M.n, iters=k, x=x_arg, iterate=True, normalize=True)
            got = power(torch, H, M.n, x0, k)
            assert got[:2] == (k, pm.MAX_STEPS)
            assert_bits(got[6], y, "csr, %d steps against smvp_csr_compute" % k)
            y, ms, st = sm.tjds_compute(M.coo, M.n, M.n, iters=k, x=x_arg, iterate=True, normalize=True)
            assert_bits(power(torch, T, M.n, x0, k)[6], y, "tjds, %d steps against smvp_tjds_compute" % k)
    H.close()
    T.close()


# ==================================================================================================================== 6. operands
def test_operands(torch):
    M = matrix("sym")
    side = torch.cuda.Stream()
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        for x0 in (pi.ones(M), pi.random_x(M)):
            want = pm.run(product, x0, 25, 1e-9, 4)
            same(power(torch, H, M.n, x0, 25, 1e-9, 4), want, fmt + ", separate vectors")
            same(power(torch, H, M.n, x0, 25, 1e-9, 4, alias=True), want, fmt + ", d_x is d_x0")
            same(power(torch, H, M.n, x0, 25, 1e-9, 4, stream=side), want, fmt + ", a stream of the caller's")
            same(power(torch, H, M.n, x0, 25, 1e-9, 4), power(torch, H, M.n, x0, 25, 1e-9, 4), fmt + ", two runs")
        same(power(torch, H, M.n, None, 25, 1e-9, 4), pm.run(product, pi.ones(M), 25, 1e-9, 4), fmt + ", x0 = NULL is ones")
        H.close()


def test_a_matrix_without_rows(torch):
    A = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    T = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 0))
    for H in (A, T):
        steps, reason, index, lam, res, scale, x = power(torch, H, 0, None, 5)
        assert (steps, reason, index, scale) == (0, pm.ZERO, -1, 0.0) and len(lam) == 0
        r, lam, res = H.power_method(None, None, 5)
        assert np.isnan(r.eigenvalue) and r.residual == 0.0
        H.close()


# ====================================================================================================================== 7. refusals
def refused(torch, fn, h, n, o, result=True, x0="own", x="own"):
    """The status of one call that must be refused: d_x, *result and the histories come back untouched."""
    dx = torch.full((max(n, 1) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    d0 = dev(torch, np.ones(max(n, 1))) if isinstance(x0, str) else x0
    r = sm.PowerResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    lam, res = np.full(8, SENTINEL), np.full(8, SENTINEL)
    torch.cuda.synchronize()
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, sm._dev_ptr(d0), sm._dev_ptr(dx if isinstance(x, str) else x),
                               C.byref(r) if result else None, sm._p(lam), sm._p(res), None)
    torch.cuda.synchronize()
    assert (dx.cpu().numpy() == SENTINEL).all(), "%s wrote d_x although it refused" % fn
    assert bytes(r) == before and (lam == SENTINEL).all() and (res == SENTINEL).all(), "%s wrote its outputs although it refused" % fn
    return rc


def bad_opts():
    def o(**kw):
        v = sm.power_opts(5)
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    return [None, o(struct_size=20), o(struct_size=0), o(max_steps=0), o(max_steps=-3), o(check_every=0), o(tol=-1e-300),
            o(tol=float("nan")), o(tol=float("inf"))]


def test_invalid_arguments_are_refused_and_nothing_is_written(torch):
    M = matrix("tiny_integers")
    A, pa = handle(torch, M, "csr", *AUTO)
    T, pt = handle(torch, M, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    wide = sm.make_coo([0, 1, 2], [1, 3, 0], [1.5, -2.5, 3.5])                       # 3 x 4
    W = sm.CsrMatrix(3, 4, *sm.csr_from_coo(wide, 3))
    WT = sm.TjdsMatrix(sm.tjds_from_coo(wide, 3, 4))
    ok = sm.power_opts(5)
    for fn, H, product, Wide in (("smvp_csr_power_method", A, pa, W), ("smvp_tjds_power_method", T, pt, WT)):
        assert refused(torch, fn, None, M.n, ok) == sm.ERR_INVALID
        for o in bad_opts():
            assert refused(torch, fn, H._h, M.n, o) == sm.ERR_INVALID, "opts %r" % (o and [getattr(o, f[0]) for f in o._fields_],)
        assert refused(torch, fn, H._h, M.n, ok, result=False) == sm.ERR_INVALID
        assert refused(torch, fn, Wide._h, 4, ok) == sm.ERR_INVALID                  # rows != cols
        assert refused(torch, fn, H._h, M.n, ok, x=None) == sm.ERR_INVALID           # no d_x
        both = torch.full((M.n + 1,), SENTINEL, dtype=torch.float64, device="cuda")  # d_x0 and d_x one element apart
        assert refused(torch, fn, H._h, M.n, ok, x0=both[:M.n], x=both[1:]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, M.n, ok, x0=both[1:], x=both[:M.n]) == sm.ERR_INVALID
        assert (both.cpu().numpy() == SENTINEL).all()
        same(power(torch, H, M.n, None, 5), pm.run(product, pi.ones(M), 5), fn + ": the handle after the refusals")
    for H in (A, T, W, WT):
        H.close()


def test_unsupported_handles_are_refused_and_nothing_is_written(torch):
    M = matrix("short")
    t = sm.tjds_from_coo(M.coo, M.n, M.n)
    T = sm.TjdsMatrix(t)
    ok = sm.power_opts(5)
    inner = inner_csr_handle(T, M.n, M.n, M.nnz)                                     # a CSR handle that is not plain CSR
    assert refused(torch, "smvp_csr_power_method", inner, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ATOMIC)
    assert refused(torch, "smvp_tjds_power_method", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_ref_quirks(True)
    assert refused(torch, "smvp_tjds_power_method", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_ref_quirks(False)
    assert power(torch, T, M.n, None, 5)[:2] == (5, pm.MAX_STEPS)
    T.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(torch, fmt, a, b):
    M = matrix("tiny_integers")
    H, product = handle(torch, M, fmt, a, b)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((M.n,), SENTINEL, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    o, r, got = sm.power_opts(5), sm.PowerResult(), []
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    lam, res = np.full(5, SENTINEL), np.full(5, SENTINEL)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)                                     # (keeps the captured graph from being empty)
            got.append(getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), None, sm._dev_ptr(dx), C.byref(r), sm._p(lam), sm._p(res), s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg
    assert bytes(r) == before and (lam == SENTINEL).all() and (res == SENTINEL).all()
    g.replay()                                               # the capture stayed valid, and holds nothing of the refused call
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == SENTINEL).all()
    del g
    same(power(torch, H, M.n, None, 5, stream=s), pm.run(product, pi.ones(M), 5), "outside a capture the same stream is fine")
    H.close()


# ========================================================================================================================= 8. state
def test_the_handles_state_afterwards(torch):
    M = matrix("long")
    x = pi.random_x(M)
    for fmt, a, b in PATHS:
        H, product = handle(torch, M, fmt, a, b)
        name = H.describe()
        dx = dev(torch, x)
        before = []
        for _ in range(2):                                   # (the tile kernel's sweep direction may alternate: two products)
            buf, dy = guarded_y(torch, M.n)
            if fmt == "tjds":
                H.set_x(dx)
            H.spmv(*((dx, dy) if fmt == "csr" else (dy,)))
            torch.cuda.synchronize()
            before.append(dy.cpu().numpy())
        first = power(torch, H, M.n, pi.ones(M), 7, 1e-9, 2)
        assert H.describe() == name
        for want in before:
            buf, dy = guarded_y(torch, M.n)
            if fmt == "tjds":
                H.set_x(dx)                                  # the permuted operand is the last step's: a fresh set_x, as the header says
            H.spmv(*((dx, dy) if fmt == "csr" else (dy,)))
            torch.cuda.synchronize()
            check_guards(buf, M.n)
            assert_bits(dy.cpu().numpy(), want, "%s %d %d: a product after the call" % (fmt, a, b))
        same(power(torch, H, M.n, pi.ones(M), 7, 1e-9, 2), first, "%s %d %d: the same call again" % (fmt, a, b))
        H.close()
