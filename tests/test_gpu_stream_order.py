"""GPU: every stream-taking entry point with its operands still in flight on the stream it is given (tests/stream_order.py has
the pattern: a delay, the copies that give the operands their true content, the fills that poison the outputs, an event -- all on a
non-blocking stream `side`; until the event completes the operands hold NaN or a valid stale structure).

The header gives each of these calls a stream contract: "asynchronous on `stream`" (products, block products, transposed
products, smvp_*_diagonal, smvp_trsv_solve, smvp_ilu0_factor), "the call waits for `stream`" (smvp_csr_trsv_create,
smvp_csr_ilu0_create, smvp_csr_create_transposed) and "returns after the work on `stream` has finished" (the Krylov solvers, the
power method, smvp_vector_dot, the two *_from_coo_device).  With the device idle on both sides of a call the bits are the same
whichever stream a kernel, a memset or a copy inside the library went to; here a pass on the null stream, a helper kernel without
its stream argument, a blocking copy that does not wait for the caller's stream or a missing event around the binned plan's side
stream reads stale operands or is overwritten by the poison, and the bits differ.  Every comparison is exact: integer-valued
operands against an int64 reference on the product paths, the restatements' bits elsewhere.

The guard of every case is the event, never the delay: pending right before the call and, for the asynchronous entry points,
right after it (the call enqueued everything while its operands were pending and synchronised nothing).  Results of asynchronous
calls are read through a clone enqueued on `side` after side.synchronize() alone, then again after the whole device has settled.
Measured on the MI355X: torch.cuda._sleep runs 2.38 - 2.39 million cycles per ms (the rate is printed by every run); the 50 ms
target was enough for every case and no case raises it -- the longest asynchronous sequence is six calls (two TJDS products).

Non-blocking is not enough for a stream to run beside the null stream: the runtime maps streams onto four hardware queues, and of
ten pool streams probed five shared the null stream's queue, where a kernel launched on the wrong stream waits for the operands by
accident.  The `side` fixture therefore takes the first pool stream that is seen to run beside the null stream, and the first test
holds the whole pattern to that: work on the null stream must see the stale content."""
import functools

import numpy as np
import pytest

import adopted
import bicgstab_method as bi
import cg_method as cg
import ilu0_method as ilu
import mixed_structures as ms
import pbicgstab_method as pb
import pcg_method as pcg
import pcg_tri_method as tri
import power_method as pm
import smvp_toolkit_amd as sm
import special_values as sv
import stream_order as so
import test_gpu_bicgstab as k13
import test_gpu_cg as k12
import test_gpu_ilu0 as k17
import test_gpu_parity as gp
import test_gpu_pbicgstab as k18
import test_gpu_pcg as k14
import test_gpu_pcg_tri as k16
import test_gpu_power_method as k11
import test_gpu_transposed as gt
import test_gpu_trsv as k15
import transposed as tr
import trsv_method as tm
from parity import guarded_y
from test_gpu_mixed_structures import binned_paths
from test_gpu_special_values import Operands, csr_paths, tjds_paths
from transposed import assert_bits
from trsv_method import LOWER, STORED, UNIT, UPPER

pytestmark = pytest.mark.gpu

FORWARD = "square:0"        # mixed_structures: 20 000 x 20 000, far entries, a row beyond kOwnerMaxRow, the window plan, TJDS
KS = (1, 5, 17)             # vectors of a block product: one, an odd few, and 17 = a full pass of 16 plus vector 16 on its own


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def side(torch):
    """The caller's stream of every test: one of torch's pool streams, which are non-blocking -- nothing orders it against the null
    stream -- chosen so that it does not share the null stream's hardware queue either (stream_order.side_stream).  The delay kernel
    is measured on it once."""
    return so.side_stream(torch)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def forward_case():
    """(rows, cols, csr arrays, coo, x1, x2, xr1, xr2): FORWARD with its exact operands and a second operand pair of the same
    range, so that two products in a row have different right answers; computed once, shared, left unchanged."""
    rows, cols, row0, _ = ms.structure(FORWARD)
    assert row0 == 0
    coo, x1, xr1 = ms.operands(FORWARD, "exact")
    x2, xr2 = -np.roll(x1, 7)[::-1].copy(), -np.roll(xr1, 11)[::-1].copy()
    for a in (x2, xr2):
        a.setflags(write=False)
    return rows, cols, ms.csr_of(FORWARD, coo), coo, x1, x2, xr1, xr2


# ============================================================================================================ 1. the harness itself
def test_the_harness_sees_work_that_runs_on_another_stream(torch, side):
    """With x in flight on `side`, a torch multiplication of x on the null stream must read the stale NaN, and the same
    multiplication on `side` the true values.  If the first did not, wrong-stream work would be invisible on this machine and every
    other test of this file vacuous."""
    n = 1 << 16
    x = torch.arange(1, n + 1, dtype=torch.float64, device="cuda")
    pair = so.stage(torch, x)
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, [pair], [])
    so.pending(ev, "before the multiplications")
    early = torch.mul(x, 2.0)                                        # the null stream: nothing orders it behind `side`
    done = torch.cuda.Event()
    done.record()
    done.synchronize()                                               # (waits for the null stream alone)
    so.pending(ev, "after the null stream's multiplication had finished")
    got_early = early.cpu().numpy()
    with torch.cuda.stream(side):
        late = torch.mul(x, 2.0)
    (got_late,), _ = so.read_on(torch, side, [late])
    torch.cuda.synchronize()
    assert np.isnan(got_early).all(), "work on the null stream waited for `side`: %d of %d elements are not the stale NaN" % (
        int((~np.isnan(got_early)).sum()), n)
    assert_bits(got_late, 2.0 * np.arange(1, n + 1), "the multiplication on `side`")
    assert ev.query()


# ===================================================================================================== 2. forward products, every path
def path_families():
    rows, cols, (rp, ci, v), coo, *_ = forward_case()
    return {"csr": lambda: csr_paths(rows, cols, rp, ci, v), "binned": lambda: binned_paths(rows, cols, rp, ci, v, 0),
            "tjds": lambda: tjds_paths(rows, cols, rp, ci, v)}


@pytest.mark.parametrize("family", ["csr", "binned", "tjds"])
def test_two_forward_products_back_to_back_with_everything_in_flight(torch, side, family):
    """Per path: x1 -> y1 and x2 -> y2 enqueued on `side` with nothing in between, both x in flight, both y poisoned in flight.  The
    second product reuses the first one's scratch (bins, carries, two-phase partials, the permuted operand) behind it on the same
    stream.  Integer-valued operands: the int64 reference's bits on every path, TJDS ATOMIC included."""
    rows, cols, (rp, ci, v), coo, x1, x2, _, _ = forward_case()
    refs = adopted.reference(rp, ci, v, x1), adopted.reference(rp, ci, v, x2)
    assert (refs[0] != refs[1]).mean() > 0.9
    t1, t2 = dev(torch, x1), dev(torch, x2)                          # the staged true values
    d1, d2 = torch.empty_like(t1), torch.empty_like(t2)
    (b1, y1), (b2, y2) = guarded_y(torch, rows), guarded_y(torch, rows)
    problems, kernels, windows, paths = [], set(), 0, 0
    for label, run, _, kernel in path_families()[family]():
        what = "%s (%s)" % (label, kernel)
        d1.fill_(float("nan"))
        d2.fill_(float("nan"))
        torch.cuda.synchronize()
        ev = so.in_flight(torch, side, [(d1, t1), (d2, t2)], [y1, y2])
        so.pending(ev, "before the products of " + what)
        run(d1, y1, stream=side)
        run(d2, y2, stream=side)
        so.pending(ev, "after the products of %s had been enqueued" % what)
        got, clones = so.read_on(torch, side, [y1, y2])
        try:
            sv.check_bits(got[0], refs[0], what + ": the first product")
            sv.check_bits(got[1], refs[1], what + ": the second product")
            so.settled(torch, [y1, y2], clones, [(b1, rows), (b2, rows)], what)
        except AssertionError as e:
            problems.append(str(e)[:400])
        torch.cuda.synchronize()
        kernels.add(kernel.split("<")[0].split(":")[0])
        windows += "csr_near_window" in kernel
        paths += 1
    print("stream order: %s: %d paths, kernels %s" % (family, paths, sorted(kernels)))
    assert not problems, "%d paths gave other bits with their operands in flight:\n%s" % (len(problems), "\n".join(problems))
    if family == "csr":
        assert {"csr_stream_owner", "csr_stream_tiles", "csr_colsweep", "csr_binned"} <= kernels, kernels
    if family == "binned":
        assert windows >= 2, "the default band of %s keeps its near part on the window plan (pass A on the plan's own stream)" % FORWARD


# =================================================================================================== 3. block and transposed products
def block_operands(torch, n_in, n_out, k, columns):
    """X as a column slice of a wider block (ldx = k + 3 > k) holding `columns` (n_in x k), stale and staged; Y as a column slice of
    a wider block (ldy = k + 2) to be poisoned in flight.  -> (X, pair for in_flight, whole Y block, Y)."""
    wide = np.zeros((n_in, k + 3))
    wide[:, 1:1 + k] = columns
    bx = dev(torch, wide)
    pair = so.stage(torch, bx)
    by = torch.full((n_out, k + 2), float("nan"), dtype=torch.float64, device="cuda")
    return bx[:, 1:1 + k], pair, by, by[:, 2:2 + k]


def block_columns(x, k):
    """k integer-valued columns from one operand: column j is x rolled by 13 j, with the sign of j's parity."""
    return np.stack([np.roll(x, 13 * j) * (-1.0) ** j for j in range(k)], axis=1)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("entry", ["csr_spmm", "tjds_spmm", "tjds_spmm_transposed"])
def test_block_products_with_the_block_in_flight(torch, side, entry, k):
    """smvp_csr_spmm, smvp_tjds_spmm, smvp_tjds_spmm_transposed: X in flight as a column slice with ldx > k, Y poisoned in flight as
    one with ldy > k; the columns beside Y keep the poison.  The two forward forms build their plan in the handle's first call, which
    synchronises `stream` as the header says, so that call is made beforehand on an idle device; K9 needs no plan."""
    rows, cols, (rp, ci, v), coo, x1, x2, xr1, _ = forward_case()
    if entry == "tjds_spmm_transposed":
        n_in, n_out, cols_in = rows, cols, block_columns(xr1, k)
        ref = adopted.reference_t(rp, ci, v, cols_in, cols)
    else:
        n_in, n_out, cols_in = cols, rows, block_columns(x1, k)
        ref = adopted.reference(rp, ci, v, cols_in)
    H = sm.CsrMatrix(rows, cols, rp, ci, v) if entry == "csr_spmm" else sm.TjdsMatrix(sm.tjds_from_coo(coo, rows, cols))
    call = {"csr_spmm": "spmm", "tjds_spmm": "spmm", "tjds_spmm_transposed": "spmm_transposed"}[entry]
    if entry != "tjds_spmm_transposed":                              # the plan, from row_ptr / the TJDS arrays alone
        getattr(H, call)(dev(torch, np.ones((n_in, k))), torch.empty((n_out, k), dtype=torch.float64, device="cuda"))
    X, pair, by, Y = block_operands(torch, n_in, n_out, k, cols_in)
    assert X.stride(0) == k + 3 and Y.stride(0) == k + 2
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, [pair], [by])
    so.pending(ev, "before smvp_" + entry)
    getattr(H, call)(X, Y, stream=side)
    so.pending(ev, "after smvp_%s had returned" % entry)
    (got,), clones = so.read_on(torch, side, [by])
    assert_bits(got[:, 2:2 + k].ravel(), ref.reshape(n_out, k).ravel(), "smvp_%s, k = %d, X in flight" % (entry, k))
    assert np.isnan(got[:, :2]).all(), "the columns in front of Y were written"
    so.settled(torch, [by], clones, what="smvp_%s, k = %d" % (entry, k))
    H.close()


def test_the_transposed_product_with_x_in_flight(torch, side):
    """smvp_tjds_spmv_transposed (K8): x in flight, y poisoned in flight, the handle's first call."""
    rows, cols, (rp, ci, v), coo, _, _, xr1, xr2 = forward_case()
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, rows, cols))
    refs = [adopted.reference_t(rp, ci, v, x, cols) for x in (xr1, xr2)]
    pairs = [so.stage(torch, dev(torch, x)) for x in (xr1, xr2)]
    (b1, y1), (b2, y2) = guarded_y(torch, cols), guarded_y(torch, cols)
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, pairs, [y1, y2])
    so.pending(ev, "before smvp_tjds_spmv_transposed")
    T.spmv_transposed(pairs[0][0], y1, stream=side)
    T.spmv_transposed(pairs[1][0], y2, stream=side)
    so.pending(ev, "after both smvp_tjds_spmv_transposed had returned")
    got, clones = so.read_on(torch, side, [y1, y2])
    assert_bits(got[0], refs[0], "K8, the first product")
    assert_bits(got[1], refs[1], "K8, the second product")
    so.settled(torch, [y1, y2], clones, [(b1, cols), (b2, cols)], "K8")
    T.close()


def test_create_transposed_waits_for_adopted_values_in_flight(torch, side):
    """smvp_csr_create_transposed(stream = side) on a handle whose adopted val is in flight: on return the new handle's arrays are
    smvp_csr_from_coo's of the swapped entries, the true values among them."""
    rows, cols, (rp, ci, v), coo, *_ = forward_case()
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    A = sm.CsrMatrix(rows, cols, d_rp, d_ci, d_v)
    pair = so.stage(torch, d_v)
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, [pair], [])
    so.pending(ev, "before smvp_csr_create_transposed")
    At = A.transposed(stream=side)
    assert ev.query(), "smvp_csr_create_transposed returned before the work on its stream had finished"
    gt.assert_arrays(gt.arrays_of(torch, At), tr.transposed_csr(coo, cols), "the transposed handle of values in flight")
    torch.cuda.synchronize()
    At.close()
    A.close()


# =================================================================================================================== 4. vector kernels
@pytest.mark.parametrize("fmt", ["csr", "tjds"])
def test_the_diagonal_of_adopted_values_in_flight(torch, side, fmt):
    """smvp_csr_diagonal / smvp_tjds_diagonal: the handle's adopted val and its adopted index array (col_ind; TJDS: row_ind) in
    flight -- the stale indices are 0 everywhere, a valid structure with another diagonal -- and the output poisoned in flight."""
    M, want = k14.diagonal_case(1)
    H, v = k14.adopted(torch, M, fmt)
    index = H._keep[1] if fmt == "csr" else H._t.row_ind             # the tensors the handle adopted (k14.adopted)
    assert index.data_ptr() != v.data_ptr() and index.numel() == v.numel() and str(index.dtype) == "torch.int32"
    pairs = [so.stage(torch, v), so.stage(torch, index, so.stale_like(torch, index))]
    buf, d = guarded_y(torch, M.rows)
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, pairs, [d])
    so.pending(ev, "before the diagonal")
    assert H.diagonal(d, stream=side) is d
    so.pending(ev, "after the diagonal had returned")
    (got,), clones = so.read_on(torch, side, [d])
    assert_bits(got, want, "%s: the diagonal of values in flight" % fmt)
    so.settled(torch, [d], clones, [(buf, M.rows)], fmt + ": the diagonal")
    H.close()


def test_the_dot_with_both_vectors_in_flight(torch, side):
    """smvp_vector_dot at cg.TRIP + 1: the partials kernel's second grid trip and the finish kernel; it returns after the work."""
    a, b = k12.dot_operands(cg.TRIP + 1)
    pairs = [so.stage(torch, dev(torch, a)), so.stage(torch, dev(torch, b))]
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, pairs, [])
    so.pending(ev, "before smvp_vector_dot")
    got = sm.vector_dot(pairs[0][0], pairs[1][0], stream=side)
    assert ev.query(), "smvp_vector_dot returned before the work on its stream had finished"
    assert_bits([got], [cg.dot(a, b)], "smvp_vector_dot of vectors in flight")
    torch.cuda.synchronize()
    assert_bits(pairs[0][0].cpu().numpy(), a, "d_a afterwards")


# ============================================================================================================== 5. triangular solves
def trsv_cases():
    """(Case, uplo): the constructed wide_thin_wide schedule (wide launches and chains) as it is (LOWER) and flipped (UPPER), and
    tridiagonal(300) -- one chain of 300 levels -- both ways."""
    w = k15.chain_width()
    wide, chain = tm.wide_thin_wide(w), tm.existing_cases()[3]
    assert chain.name.startswith("tridiagonal")
    return [(wide, LOWER), (tm.flipped(wide), UPPER), (chain, LOWER), (chain, UPPER)]


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("i", range(4))
def test_a_triangular_solve_with_b_in_flight(torch, side, i, alias):
    """smvp_trsv_solve with d_b in flight and d_x poisoned in flight; alias: d_x is d_b, in flight."""
    M, uplo = trsv_cases()[i]
    H = k15.handle_of(M)
    P = H.trsv_plan(uplo, STORED)
    info = P.info()
    assert (info["launches"] > info["chains"] >= 1) if i < 2 else (info["launches"], info["chains"], info["levels"]) == (1, 1, M.n)
    b, want = M.reference(uplo, STORED)
    buf, dx = guarded_y(torch, M.n)
    if alias:
        dx.copy_(dev(torch, b))
        db, pair, outputs = dx, so.stage(torch, dx), []
    else:
        db = dev(torch, b)
        pair, outputs = so.stage(torch, db), [dx]
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, [pair], outputs)
    so.pending(ev, "before smvp_trsv_solve")
    assert P.solve(db, dx, stream=side) is dx
    so.pending(ev, "after smvp_trsv_solve had returned")
    (got,), clones = so.read_on(torch, side, [dx])
    assert_bits(got, want, "%s, uplo %d%s: b in flight" % (M.name, uplo, ", d_x is d_b" if alias else ""))
    so.settled(torch, [dx], clones, [(buf, M.n)], M.name)
    if not alias:
        assert_bits(db.cpu().numpy(), b, "d_b after the solve")
    P.close()
    H.close()


def test_symmetric_gauss_seidel_composed_on_the_side_stream(torch, side):
    """z = U^-1 (d o (L^-1 r)) on `side` with nothing in between: the lower solve, torch.mul, the upper solve; r and d in flight, the
    intermediate and z poisoned in flight; trsv_method's bits."""
    M = tm.existing_cases()[3]
    d = pcg.diagonal_csr(M.n, M.n, *M.csr)
    r = tm.rhs(M.n, 16)
    want = tm.solve(M, UPPER, STORED, tm.solve(M, LOWER, STORED, r) * d)
    H = k15.handle_of(M)
    L, U = H.trsv_plan(LOWER), H.trsv_plan(UPPER)
    pr, pd = so.stage(torch, dev(torch, r)), so.stage(torch, dev(torch, d))
    dt = torch.empty(M.n, dtype=torch.float64, device="cuda")
    buf, dz = guarded_y(torch, M.n)
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, [pr, pd], [dt, dz])
    so.pending(ev, "before the composition")
    L.solve(pr[0], dt, stream=side)
    with torch.cuda.stream(side):
        torch.mul(dt, pd[0], out=dt)
    U.solve(dt, dz, stream=side)
    so.pending(ev, "after the composition had been enqueued")
    (got,), clones = so.read_on(torch, side, [dz])
    assert_bits(got, want, "the symmetric Gauss-Seidel application on `side`")
    so.settled(torch, [dz], clones, [(buf, M.n)], "symmetric Gauss-Seidel")
    L.close()
    U.close()
    H.close()


@pytest.mark.parametrize("uplo", [LOWER, UPPER])
def test_trsv_create_waits_for_an_adopted_col_ind_in_flight(torch, side, uplo):
    """smvp_csr_trsv_create(stream = side) reads an adopted col_ind back for its analysis.  The stale col_ind holds every entry on
    its row's diagonal -- a valid structure of one level -- so info and schedule must be the true structure's; and the plan solves."""
    M = tm.existing_cases()[0]
    rp, ci, v = M.csr
    d_rp, d_ci, d_v = dev(torch, rp), dev(torch, ci), dev(torch, v)
    H = sm.CsrMatrix(M.n, M.n, d_rp, d_ci, d_v)
    stale = dev(torch, sv.row_of_entries(rp).astype(np.int32))
    pair = so.stage(torch, d_ci, stale)
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, [pair], [])
    so.pending(ev, "before smvp_csr_trsv_create")
    P = H.trsv_plan(uplo, STORED, stream=side)
    assert ev.query(), "smvp_csr_trsv_create returned before the work on its stream had finished"
    info, f = P.info(), M.facts(uplo, STORED)
    assert f["levels"] > 1
    for field in ("levels", "max_level_width", "missing_diagonals", "entries"):
        assert info[field] == f[field], "%s is %r: the true structure has %r (the stale one: one level)" % (field, info[field], f[field])
    level_ptr, order = P.schedule()
    assert level_ptr.tolist() == f["level_ptr"].tolist() and order.tolist() == f["order"].tolist()
    b, want = M.reference(uplo, STORED)
    assert_bits(k15.solve_once(torch, P, M.n, b), want, "a solve on the plan made from a col_ind in flight")
    P.close()
    H.close()


# ================================================================================================================================ 6. ILU(0)
def ilu0_case():
    Cs = ilu.grid(32)                                                # lap2d(32): 1024 rows, 63 levels
    return Cs, ilu.factor(Cs)


def test_ilu0_create_waits_for_adopted_values_in_flight(torch, side):
    """smvp_csr_ilu0_create(stream = side) on a handle whose adopted val is in flight: F is ilu0_method's on return."""
    Cs, F = ilu0_case()
    d_rp, d_ci, d_v = (dev(torch, a) for a in Cs.csr)
    A = sm.CsrMatrix(Cs.n, Cs.n, d_rp, d_ci, d_v)
    pair = so.stage(torch, d_v)
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, [pair], [])
    so.pending(ev, "before smvp_csr_ilu0_create")
    f = A.ilu0(stream=side)
    assert ev.query(), "smvp_csr_ilu0_create returned before the first factorisation had finished"
    assert_bits(gt.arrays_of(torch, f.matrix)[2], F.csr[2], "F of values in flight, read at once")
    assert_bits(k17.values_of(torch, f), F.csr[2], "F after the device has settled")
    f.close()
    A.close()


def test_ilu0_factor_and_both_solves_with_the_values_in_flight(torch, side):
    """smvp_ilu0_factor with the source's adopted val in flight and F's own values poisoned in flight, followed on `side` by the
    solves of both plans of F: F and x = U^-1 L^-1 b are the restatement's."""
    Cs, F = ilu0_case()
    d_rp, d_ci, d_v = (dev(torch, a) for a in Cs.csr)
    A = sm.CsrMatrix(Cs.n, Cs.n, d_rp, d_ci, d_v)
    f = A.ilu0()
    Lp, Up = f.plans()
    fv = k17.values_tensor(torch, f)
    b = tm.rhs(Cs.n, 21)
    want = tm.solve(F, UPPER, STORED, tm.solve(F, LOWER, UNIT, b))
    pv, pb_ = so.stage(torch, d_v), so.stage(torch, dev(torch, b))
    dt = torch.empty(Cs.n, dtype=torch.float64, device="cuda")
    buf, dx = guarded_y(torch, Cs.n)
    torch.cuda.synchronize()
    ev = so.in_flight(torch, side, [pv, pb_], [fv, dt, dx])
    so.pending(ev, "before smvp_ilu0_factor")
    f.factor(stream=side)
    Lp.solve(pb_[0], dt, stream=side)
    Up.solve(dt, dx, stream=side)
    so.pending(ev, "after the factorisation and both solves had been enqueued")
    (got_f, got_x), clones = so.read_on(torch, side, [fv, dx])
    assert_bits(got_f[:Cs.nnz], F.csr[2], "F of values in flight")
    assert_bits(got_x, want, "U^-1 L^-1 b behind the factorisation")
    so.settled(torch, [fv, dx], clones, [(buf, Cs.n)], "ILU(0) and its solves")
    for X in (Lp, Up, f, A):
        X.close()


# ============================================================================================================== 7. the blocking calls
def returned_after(seen, fn):
    """The solver returned only after the work on its stream -- the operands' event in front of it -- had finished."""
    assert len(seen) == 1 and seen[0][0].query(), "%s returned before the work on its stream had finished" % fn
    del seen[:]


@pytest.mark.parametrize("fmt,a,b", k11.BOTH)
def test_the_power_method_with_x0_in_flight(torch, side, fmt, a, b):
    M = k11.matrix("short")
    H, product = k11.handle(torch, M, fmt, a, b)
    x0 = np.random.default_rng(3).uniform(0.5, 1.5, M.n)
    want = pm.run(product, x0, 12, 1e-9, 4)
    seen = []
    got = k11.power(torch, H, M.n, x0, 12, 1e-9, 4, stream=side, before=so.solver_hook(torch, side, seen))
    returned_after(seen, "the power method")
    k11.same(got, want, "the power method, %s, x0 in flight" % fmt)
    H.close()


def test_the_power_method_on_the_binned_window_plan(torch, side):
    """The product inside the solver forks onto the binned plan's own stream and joins again: pass A reads the iterate, the near
    part writes the product, pass B waits for both -- in every step, behind an x0 that is in flight."""
    rows, cols, (rp, ci, v), *_ = forward_case()
    A = sm.CsrMatrix(rows, cols, rp, ci, v)
    A.set_kernel(sm.CSR_KERNEL_BINNED, 0)
    assert "csr_near_window" in A.describe()[0], A.describe()[0]
    ops = Operands(torch, rows, cols)
    x0 = np.random.default_rng(4).uniform(0.5, 1.5, rows)
    want = pm.run(lambda x: ops.product(lambda dx, dy: A.spmv(dx, dy), x), x0, 5, 0.0, 2)
    seen = []
    got = k11.power(torch, A, rows, x0, 5, 0.0, 2, stream=side, before=so.solver_hook(torch, side, seen))
    returned_after(seen, "smvp_csr_power_method")
    k11.same(got, want, "the power method on %s" % A.describe()[0])
    A.close()


@pytest.mark.parametrize("fmt,a,b", k12.BOTH)
def test_cg_and_pcg_with_b_x0_and_m_in_flight(torch, side, fmt, a, b):
    M, m = k14.matrix("scaled", 1003), k14.jacobi("scaled", 1003)
    H, product = k12.handle(torch, M, fmt, a, b)
    rhs, x0 = cg.rhs(M.n), k12.start_vector(M.n)
    seen = []
    hook = so.solver_hook(torch, side, seen)
    for start in (None, x0):
        what = "%s, x0 %s, everything in flight" % (fmt, "NULL" if start is None else "random")
        got = k12.solve(torch, H, M.n, rhs, start, k12.MAX_STEPS, 1e-10, 7, stream=side, before=hook)
        returned_after(seen, "cg")
        k12.same(got, cg.run(product, rhs, start, k12.MAX_STEPS, 1e-10), "cg, " + what, rhs)
        got = k14.solve(torch, H, M.n, rhs, m, start, k14.MAX_STEPS, k14.TOL, 7, stream=side, before=hook)
        returned_after(seen, "pcg")
        k14.same(got, pcg.run(product, rhs, start, m, k14.MAX_STEPS, k14.TOL), "pcg, " + what, rhs)
    H.close()


@pytest.mark.parametrize("fmt,a,b", k12.BOTH)
def test_pcg_tri_with_b_x0_and_m_in_flight(torch, side, fmt, a, b):
    M, Cs = k16.system("scaled(1003)")
    P = k16.Plans(*tri.sgs(Cs))
    H, product = k12.handle(torch, M, fmt, a, b)
    rhs, x0 = cg.rhs(M.n), k12.start_vector(M.n)
    seen = []
    got = k16.solve(torch, H, M.n, rhs, P, x0, k16.MAX_STEPS, k16.TOL, 7, stream=side, before=so.solver_hook(torch, side, seen))
    returned_after(seen, "pcg_tri")
    k16.same(got, P.run(product, rhs, x0, k16.MAX_STEPS, k16.TOL), "pcg_tri, %s, everything in flight" % fmt, rhs)
    H.close()
    P.close()


@pytest.mark.parametrize("fmt,a,b", k13.BOTH)
def test_bicgstab_with_b_and_x0_in_flight(torch, side, fmt, a, b):
    M = k13.matrix("nonsym", 1003)
    H, product = k13.handle(torch, M, fmt, a, b)
    rhs, x0 = bi.rhs(M.n), k13.start_vector(M.n)
    seen = []
    hook = so.solver_hook(torch, side, seen)
    for start in (None, x0):
        got = k13.solve(torch, H, M.n, rhs, start, k13.MAX_STEPS, 1e-10, 7, stream=side, before=hook)
        returned_after(seen, "bicgstab")
        k13.same(got, bi.run(product, rhs, start, k13.MAX_STEPS, 1e-10), "bicgstab, %s, x0 %s, everything in flight" % (
            fmt, "NULL" if start is None else "random"), rhs)
    H.close()


@pytest.mark.parametrize("fmt,a,b", k13.BOTH)
@pytest.mark.parametrize("name,kind", [("nonsym_long", "jacobi"), ("convdiff(32, 0.5)", "ilu0")])
def test_pbicgstab_with_b_x0_and_m_in_flight(torch, side, name, kind, fmt, a, b):
    """Jacobi: d_m alone, the scaling fused into the kernels that write y.  ILU(0): the plans of the library's own factor."""
    M, Cs = pb.case_of(name)
    P = k18.plans_of(torch, kind, Cs)
    assert (P.m is not None and P.first is None and P.second is None) if kind == "jacobi" else (P.first is not None and P.second is not None)
    H, product = k13.handle(torch, M, fmt, a, b)
    rhs, x0 = bi.rhs(M.n), k13.start_vector(M.n)
    seen = []
    got = k18.solve(torch, H, M.n, rhs, P, x0, k18.MAX_STEPS, k18.TOL, 3, stream=side, before=so.solver_hook(torch, side, seen))
    returned_after(seen, "pbicgstab")
    k13.same(got, P.run(product, rhs, x0, k18.MAX_STEPS, k18.TOL), "pbicgstab with %s on %s, %s, everything in flight" % (kind, name, fmt), rhs)
    H.close()
    P.close()


def test_the_device_converters_with_the_coo_in_flight(torch, side):
    """smvp_csr_from_coo_device and smvp_tjds_from_coo_device on an entry list in flight; the stale list holds (0, 0, 1.0) in every
    entry.  On return the arrays are the host converters', byte for byte."""
    rows, cols, _, coo, *_ = forward_case()
    coo = coo[np.random.default_rng(6).permutation(len(coo))]
    nnz = len(coo)
    d_coo = gp._coo_to_device(torch, coo)
    pair = so.stage(torch, d_coo, so.stale_like(torch, d_coo, "coo"))
    hrp, hci, hv = sm.csr_from_coo(coo, rows)
    h = sm.tjds_from_coo(coo, rows, cols)
    for which in ("csr", "tjds"):
        d_coo.copy_(so.stale_like(torch, d_coo, "coo"))
        torch.cuda.synchronize()
        ev = so.in_flight(torch, side, [pair], [])
        so.pending(ev, "before smvp_%s_from_coo_device" % which)
        if which == "csr":
            rp, ci, v = sm.csr_from_coo_device(d_coo, rows, cols, nnz, stream=side)
        else:
            t = sm.tjds_from_coo_device(d_coo, rows, cols, nnz, stream=side)
        assert ev.query(), "smvp_%s_from_coo_device returned before the work on its stream had finished" % which
        if which == "csr":
            assert np.array_equal(rp.cpu().numpy(), hrp) and np.array_equal(ci.cpu().numpy(), hci), "row_ptr / col_ind of a list in flight"
            assert v.cpu().numpy().tobytes() == hv.tobytes(), "val of a list in flight"
        else:
            assert (t.num_diag, t.ref_num_tjdiag, t.last_diag_single) == (h.num_diag, h.ref_num_tjdiag, h.last_diag_single)
            for field in ("perm", "start_pos", "row_ind"):
                assert np.array_equal(getattr(t, field).cpu().numpy(), getattr(h, field)), field + " of a list in flight"
            assert t.val.cpu().numpy().tobytes() == h.val.tobytes(), "val of a list in flight"
        torch.cuda.synchronize()
        assert torch.equal(d_coo, pair[1]), "the entry list afterwards"
