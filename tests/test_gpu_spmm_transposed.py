"""smvp_tjds_spmm_transposed (K9) on the GPU: Y = A^T X for k vectors from the TJDS arrays, every column of Y bit for bit the
transposed product of that column of X.  Reference: tests/transposed.py -- the host converter's CSR arrays of the swapped
entries under the oracle's serial loop, column by column (reference_block converts once and runs the loop per column, which
is tr.reference(coo, rows, cols, X[:, v]) for every v).  Every check is equality of bits (NaN = NaN), on every column.

Y always lies in test_gpu_spmm.guarded_Y: GUARD words in front of and behind it, NaN in every slot the call writes, GUARD in
the padding columns k <= v < ldy, which must keep their bits (check_Y_guards).

The special-value scenarios of tests/special_values.py are written for forward products B x on a catalogue of patterns B; they
are run here on A = B^T (the same entries with row and column swapped), for which A^T X = B X: the scenarios' operands,
conditions (sv.assert_regime on the structures sv.REGIME lists) and row classes apply unchanged.  The structures are
sv.SMALL: the two of millions of rows exist to reach the binned plan and the near window of the CSR kernels, which K9 has not.
"""
import numpy as np
import pytest

import oracle_binding as ob
import smvp_toolkit_amd as sm
import special_values as sv
import transposed as tr
from conftest import SAMPLES
from parity import G, GUARD, check_guards, check_y, guarded_y
from test_gpu_spmm import KS, check_Y_guards, dev_X, guarded_Y
from test_gpu_transposed import TJDS_MODES, coo_from_lists, dev, load, replicated

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 4, 8, 16)          # lanes per column of a pass; 64 / G columns per wavefront
BATCH = 8                          # jagged diagonals per batch (kTjdsSpmmTBatch)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def reference_block(coo, rows, cols, X):
    """A^T X column by column: the oracle's serial loop over tr.transposed_csr(coo, cols); (cols, k)."""
    X = np.asarray(X, dtype=np.float64)
    assert X.ndim == 2 and X.shape[0] == rows
    if cols == 0:
        return np.zeros((0, X.shape[1]))
    rp, ci, v = tr.transposed_csr(coo, cols)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([ob.csr_spmv(rp, ci, v, np.ascontiguousarray(X[:, c])) for c in range(X.shape[1])], axis=1)


def assert_block(Y, ref, what):
    Y, ref = np.asarray(Y), np.asarray(ref)
    assert Y.shape == ref.shape, "%s: shape %s against %s" % (what, Y.shape, ref.shape)
    for c in range(ref.shape[1]):
        tr.assert_bits(Y[:, c], ref[:, c], "%s, vector %d" % (what, c))


def k9(torch, T, X, ldx=None, ldy=None, stream=None):
    """A^T X through smvp_tjds_spmm_transposed into a guarded Y; the host copy after the guard checks."""
    k = X.shape[1]
    ldx, ldy = ldx or k, ldy or k
    dX = dev_X(torch, X, ldx)
    buf, Y = guarded_Y(torch, T.cols, k, ldy)
    T.spmm_transposed(dX, Y, stream=stream)
    torch.cuda.synchronize()
    check_Y_guards(buf, T.cols, k, ldy)
    return Y.cpu().numpy()


def run_case(torch, rows, cols, coo, X, what, ldx=None, ldy=None, routes=False):
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, rows, cols))
    Y = k9(torch, T, X, ldx, ldy)
    T.close()
    ref = reference_block(coo, rows, cols, X)
    assert_block(Y, ref, what)
    if routes:
        assert_block(Y, via_transposed_handle(torch, rows, cols, coo, X), what + ": K9 against spmm on the transposed handle")
    return Y


def via_transposed_handle(torch, rows, cols, coo, X):
    """CsrMatrix.transposed().spmm(X, Y): the second-copy route."""
    k = X.shape[1]
    A = sm.CsrMatrix(rows, cols, *sm.csr_from_coo(coo, rows))
    At = A.transposed()
    A.close()
    buf, Y = guarded_Y(torch, cols, k, k)
    At.spmm(dev_X(torch, X, k), Y)
    torch.cuda.synchronize()
    check_Y_guards(buf, cols, k, k)
    At.close()
    return Y.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------- 1. samples
@pytest.mark.parametrize("name", SAMPLES)
def test_k9_sample_matrices_every_k_operand_and_leading_dimension(torch, name):
    m, n, coo = load(name)
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n))
    kmax = max(KS)
    for operand in ("ones", "random"):
        X = np.ones((m, kmax)) if operand == "ones" else np.random.default_rng(41).standard_normal((m, kmax))
        ref = reference_block(coo, m, n, X)
        for k in KS:
            for px, py in ((0, 0), (5, 7)):                      # tight operands, and column slices of wider arrays
                Y = k9(torch, T, X[:, :k], k + px, k + py)
                assert_block(Y, ref[:, :k], "%s %s k=%d ldx=k+%d ldy=k+%d" % (name, operand, k, px, py))
        # k = 1, ldx = ldy = 1: the bits of smvp_tjds_spmv_transposed on the same handle
        buf, dy = guarded_y(torch, n)
        T.spmv_transposed(dev(torch, X[:, 0]), dy)
        torch.cuda.synchronize()
        check_guards(buf, n)
        tr.assert_bits(k9(torch, T, X[:, :1], 1, 1)[:, 0], dy.cpu().numpy(), "%s %s: K9 with one vector against K8" % (name, operand))
        if operand == "random":
            assert_block(k9(torch, T, X), via_transposed_handle(torch, m, n, coo, X), "%s: the two routes" % name)
    T.close()


# ------------------------------------------------------------------------------------------------------- 2. edge cases
def test_k9_edge_cases(torch):
    rng = np.random.default_rng(42)
    empty = sm.make_coo([], [], [])
    # an empty matrix; no rows (Y is cols x k of +0.0); no columns (Y is empty)
    for rows, cols in ((0, 0), (0, 7), (5, 0)):
        Y = run_case(torch, rows, cols, empty, -rng.random((rows, 3)), "%d x %d" % (rows, cols), ldx=4, ldy=5)
        assert Y.shape == (cols, 3) and (Y.view(np.int64) == 0).all()
    # no entries: every Y +0.0, sign bit included, whatever X holds
    Y = run_case(torch, 9, 4, empty, np.full((9, 5), -np.inf), "9 x 4 without entries", ldy=6)
    assert (Y.view(np.int64) == 0).all()
    # every column empty but one
    coo = sm.make_coo(np.arange(0, 120, 3), np.full(40, 333), rng.uniform(-1, 1, 40))
    Y = run_case(torch, 120, 1001, coo, rng.standard_normal((120, 5)), "all columns empty but one", routes=True)
    assert (np.delete(Y, 333, axis=0).view(np.int64) == 0).all() and (Y[333] != 0).all()
    # empty columns between full ones
    lists = [sorted(3 * rng.choice(100, rng.integers(1, 40), replace=False)) for _ in range(200)]
    Y = run_case(torch, 200, 300, coo_from_lists(200, lists, rng), rng.standard_normal((200, 6)), "empty columns", routes=True)
    assert (Y.view(np.int64)[np.arange(300) % 3 != 0] == 0).all()
    # one column of 50 000 entries beside 3 000 short ones
    lists = [[0] + sorted(1 + rng.choice(3000, int(rng.integers(0, 4)), replace=False)) for _ in range(50000)]
    run_case(torch, 50000, 3001, coo_from_lists(50000, lists, rng), rng.standard_normal((50000, 3)), "one long column", routes=True)
    # one row; 1 x 1
    run_case(torch, 1, 500, coo_from_lists(1, [sorted(rng.choice(500, 123, replace=False))], rng), rng.standard_normal((1, 17)), "one row")
    run_case(torch, 1, 1, sm.make_coo([0], [0], [2.5]), np.array([[-3.0, 0.5]]), "1 x 1")
    # M >> N and N >> M
    lists = [sorted(rng.choice(3, int(rng.integers(0, 3)), replace=False)) for _ in range(50000)]
    run_case(torch, 50000, 3, coo_from_lists(50000, lists, rng), rng.standard_normal((50000, 4)), "tall", routes=True)
    lists = [sorted(rng.choice(100000, int(rng.integers(0, 50)), replace=False)) for _ in range(100)]
    run_case(torch, 100, 100000, coo_from_lists(100, lists, rng), rng.standard_normal((100, 9)), "wide", routes=True)


def columns_of_lengths(lengths, rows, rng):
    """COO whose column c holds lengths[c] entries in distinct random rows."""
    r = np.concatenate([np.sort(rng.choice(rows, int(l), replace=False)) for l in lengths] + [np.zeros(0, np.int64)])
    c = np.repeat(np.arange(len(lengths)), lengths)
    coo = sm.make_coo(r, c, rng.uniform(-1, 1, len(r)))
    return coo[rng.permutation(len(coo))]


@pytest.mark.parametrize("g", GROUPS)
def test_k9_ragged_column_counts_and_ends_inside_a_batch(torch, g):
    """For every group size G (k = G, and the k just above the next smaller G): a column count that is not a multiple of the 64 / G
    columns of a wavefront nor of the 256 / G of a workgroup; a first wavefront whose columns end at different diagonals inside
    one batch (lengths 1 ... BATCH - 1 among its 64 / G longest); a number of diagonals that is not a multiple of the batch."""
    rng = np.random.default_rng(43 + g)
    per_wave = 64 // g
    for cols, longest in ((per_wave + 3, BATCH - 1), (5 * (256 // g) + per_wave // 2 + 1, 2 * BATCH + 3), (per_wave - 1 or 1, BATCH + 1)):
        rows = 4 * longest + 5
        lengths = rng.integers(0, longest + 1, cols)
        lengths[:min(cols, longest)] = np.arange(longest, longest - min(cols, longest), -1)     # every length below the longest occurs
        coo = columns_of_lengths(rng.permutation(lengths), rows, rng)
        t = sm.tjds_from_coo(coo, rows, cols)
        assert t.num_diag == longest and t.num_diag % BATCH != 0
        widths = np.diff(t.start_pos)
        first_wave = [int((widths > c).sum()) for c in range(min(per_wave, cols))]               # the lengths of its columns
        if cols > 1 and longest < BATCH:
            assert len(set(first_wave)) > 1 and max(first_wave) < BATCH, first_wave
        for k in sorted({g, g // 2 + 1}):
            X = rng.standard_normal((rows, k))
            T = sm.TjdsMatrix(t)
            assert T.spmm_transposed_describe(k)[0] == "tjds_spmm_transposed_columns<%d>" % g
            assert_block(k9(torch, T, X, k + 1, k + 2), reference_block(coo, rows, cols, X), "G=%d cols=%d k=%d" % (g, cols, k))
            T.close()


def test_k9_repeated_pairs_are_summed_in_storage_order(torch):
    # column 1 holds (2, 1) three times: 1e16 + 1 - 1e16 is 0 in storage order, 1 with the small value last
    coo = sm.make_coo([0, 2, 2, 2, 3], [0, 1, 1, 1, 1], [4.0, 1e16, 1.0, -1e16, 0.5])
    X = np.stack([np.ones(4), 2.0 * np.ones(4), -np.ones(4)], axis=1)
    Y = run_case(torch, 4, 3, coo, X, "repeated pairs", routes=True)
    assert_block(Y, np.array([[4.0, 8.0, -4.0], [0.5, 1.0, -0.5], [0.0, 0.0, 0.0]]), "the reference itself")
    other = coo[[0, 1, 3, 2, 4]]
    assert not tr.same_bits(reference_block(other, 4, 3, X), reference_block(coo, 4, 3, X)), "the values must tell the orders apart"
    run_case(torch, 4, 3, other, X, "repeated pairs, the other order", routes=True)


def test_k9_an_ended_column_leaves_its_product_out(torch):
    """A group whose column has ended reads entry 0 -- the first entry of the longest column -- and must leave the product out
    with a select.  Here that entry lies in row 0, whose elements of X are NaN, +Inf, -Inf and -0.0 in vectors 1 ... 4, and no
    other column stores an entry in row 0: only column 7 of Y may be other than finite, and only in vectors 1 ... 3."""
    rng = np.random.default_rng(52)
    rows, cols, long_col = 400, 333, 7
    lengths = rng.integers(0, 20, cols)
    lengths[long_col] = 37                                       # the longest: permuted column 0, its entries first in every diagonal
    r = np.concatenate([np.sort(rng.choice(np.arange(1, rows), int(l), replace=False)) for l in lengths])
    c = np.repeat(np.arange(cols), lengths)
    r[np.flatnonzero(c == long_col)[0]] = 0                       # its first entry is in row 0
    coo = sm.make_coo(r, c, rng.uniform(0.5, 1, len(r)))
    t = sm.tjds_from_coo(coo, rows, cols)
    assert t.perm[0] == long_col and t.row_ind[0] == 0 and (coo["row"] == 0).sum() == 1
    for k in (5, 1, 21):
        X = rng.uniform(0.5, 1, (rows, k))
        X[0, 1 % k], X[0, 2 % k], X[0, 3 % k], X[0, 4 % k] = np.nan, np.inf, -np.inf, -0.0
        if k == 1:
            X[0, 0] = np.nan
        Y = run_case(torch, rows, cols, coo, X, "entry 0 under non-finite X, k = %d" % k, k + 2, k + 1, routes=True)
        assert np.isfinite(np.delete(Y, long_col, axis=0)).all(), "a column that does not touch row 0 is not finite"
        assert not np.isfinite(Y[long_col]).all()


# --------------------------------------------------------------------------------------------------------------- 3. fuzz
@pytest.mark.parametrize("seed", range(25))
def test_k9_fuzz_random_shapes_k_and_leading_dimensions(torch, seed):
    from test_gpu_parity import _fuzz_matrix

    rows, cols, rp, ci, v, _ = _fuzz_matrix(seed)
    rng = np.random.default_rng(4400 + seed)
    k = int(rng.integers(1, 41))
    ldx, ldy = k + int(rng.integers(0, 9)), k + int(rng.integers(0, 9))
    X = rng.standard_normal((rows, k)) * 10.0 ** rng.integers(-3, 3, (rows, k))
    ordered = tr.coo_of_csr(rp, ci, v)
    coo = ordered[rng.permutation(len(ordered))]
    run_case(torch, rows, cols, coo, X, "fuzz %d: %d x %d, k=%d ldx=%d ldy=%d" % (seed, rows, cols, k, ldx, ldy), ldx, ldy, routes=True)


# ----------------------------------------------------------------------------------------------------- 4. special values
def transposed_structure(name):
    """(rows, cols, coo) of A = B^T for the pattern B = sv.structure(name), plus B itself: A^T X = B X."""
    b_rows, b_cols, rp, ci, u = sv.structure(name)
    return b_cols, b_rows, rp, ci, u


def swapped_coo(rp, ci, val, seed=45):
    """The entries of B as entries of A = B^T (row and column exchanged), shuffled: ties have no part (B repeats no pair)."""
    nnz = int(rp[-1])
    coo = sm.make_coo(np.asarray(ci)[:nnz], sv.row_of_entries(rp), np.asarray(val)[:nnz])
    return coo[np.random.default_rng(seed).permutation(nnz)]


def k9_of_b(torch, rows, cols, rp, ci, val, X, ldx=None, ldy=None):
    """B X through K9 on A = B^T, and the oracle's B X[:, v] (which is tr.reference of A's entries: checked on the first vector)."""
    coo = swapped_coo(rp, ci, val)
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, rows, cols))
    Y = k9(torch, T, X, ldx, ldy)
    T.close()
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np.stack([ob.csr_spmv(rp, ci, val, np.ascontiguousarray(X[:, c])) for c in range(X.shape[1])], axis=1).reshape(cols, X.shape[1])
        tr.assert_bits(ref[:, 0], tr.reference(coo, rows, cols, X[:, 0]), "the oracle over B against tr.reference over A")
    return Y, ref


@pytest.mark.parametrize("name", sv.SMALL)
def test_k9_scenarios_a_to_d(torch, name):
    """A: NaN / Inf in rows of X that no column touches change no bit.  B: a NaN / Inf in vector v of a touched row changes vector
    v only, and there the class is the serial loop's.  C: a stored 0.0 under an Inf makes NaN.  D: columns of -0.0 products,
    zero operands and empty columns give +0.0."""
    rows, cols, rp, ci, u = transposed_structure(name)           # (B is cols x rows: its rows are A's columns)
    o = sv.ordinary(cols, rows, rp, ci, u)
    val = o["val"]
    sv.assert_regime(name, "A", cols, rows, rp, ci, val, o["x_a"], u)
    sv.assert_regime(name, "B", cols, rows, rp, ci, val, o["x_b"])
    sv.assert_regime(name, "C", cols, rows, rp, ci, val, o["x_c"])
    keys = ("x", "x_a", "x_b", "x", "x_c", "x_a", "x")            # 7 vectors: a pass of G = 8 with one idle lane per group
    X = np.stack([o[key] for key in keys], axis=1)
    Y, ref = k9_of_b(torch, rows, cols, rp, ci, val, X, 9, 8)
    assert_block(Y, ref, name + ", A ... C")
    clean = Y[:, 0]
    assert np.isfinite(clean).all()
    for c, key in enumerate(keys):
        if key in ("x", "x_a"):                                  # untouched rows poisoned, or a neighbour vector poisoned: no bit changes
            tr.assert_bits(Y[:, c], clean, "%s: vector %d (%s) beside poisoned vectors" % (name, c, key))
        else:
            sv.check_classes(Y[:, c], sv.row_classes(rp, ci, val, o[key]), "%s: vector %d (%s)" % (name, c, key))
        sv.check_no_negative_zero(Y[:, c], "%s: vector %d" % (name, c))
    # the same with the poisoned vector alone (k = 1) and in a pass of its own (vector 16 of 17)
    for key in ("x_a", "x_b", "x_c"):
        Y1, ref1 = k9_of_b(torch, rows, cols, rp, ci, val, o[key].reshape(-1, 1), 1, 1)
        assert_block(Y1, ref1, "%s, %s alone" % (name, key))
        X17 = np.repeat(o["x"].reshape(-1, 1), 17, axis=1)
        X17[:, 16] = o[key]
        Y17, ref17 = k9_of_b(torch, rows, cols, rp, ci, val, X17)
        assert_block(Y17, ref17, "%s, %s as vector 16 of 17" % (name, key))
        for c in range(16):
            tr.assert_bits(Y17[:, c], clean, "%s: vector %d of 17 beside %s" % (name, c, key))
    # D
    for z in (np.zeros(rows), -np.zeros(rows)):
        sv.assert_regime(name, "D", cols, rows, rp, ci, val, z)
        Z = np.stack([z, -z, z], axis=1)
        Yz, refz = k9_of_b(torch, rows, cols, rp, ci, val, Z, 3, 4)
        assert_block(Yz, refz, name + ", D")
        assert (Yz.view(np.int64) == 0).all(), "%s, D: something other than +0.0" % name


@pytest.mark.parametrize("name", sv.SMALL)
def test_k9_scenarios_e_f_and_g(torch, name):
    """E: subnormal products and sums are kept.  F: sums of +-2^1020 overflow where the serial loop's do.  G: products that round
    -- a kernel that fuses the multiply into the add differs from the serial loop in most rows."""
    rows, cols, rp, ci, u = transposed_structure(name)
    for scenario, (val, x) in (("E", sv.subnormal(cols, rows, rp, ci)), ("F", sv.overflowing(cols, rows, rp, ci)),
                               ("G", sv.rounded(cols, rows, rp, ci))):
        if scenario == "G":
            sv.assert_regime(name, "G", cols, rows, rp, ci, val, x)
        X = np.stack([x, -x, 0.5 * x, x, 2.0 * x if scenario != "F" else x], axis=1)     # (exact scalings: the bits follow the oracle's)
        Y, ref = k9_of_b(torch, rows, cols, rp, ci, val, X, 6, 5)
        if scenario == "E" and int(rp[-1]) >= 100:
            assert np.count_nonzero(ref[:, 0]) > 0 and np.abs(ref[:, 0]).max() < 2.0 ** -1022
        for c in range(X.shape[1]):
            sv.assert_exact(Y[:, c], ref[:, c], "%s, %s, vector %d" % (name, scenario, c))


# ------------------------------------------------------------------------------------------------------------- 5. state
@pytest.mark.parametrize("mode", TJDS_MODES)
def test_forward_tjds_product_is_undisturbed_by_k9(torch, mode):
    m, n, coo = load("memplus.mtx")
    rng = np.random.default_rng(46)
    x, Xt = rng.standard_normal(n), rng.standard_normal((m, 8))
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n))
    T.set_mode(mode)
    info = T.plan_info()
    T.set_x(dev(torch, x))

    def forward():
        buf, dy = guarded_y(torch, m)
        T.zero_y(dy)
        T.spmv(dy)
        torch.cuda.synchronize()
        check_guards(buf, m)
        return dy.cpu().numpy()

    y1 = forward()
    assert_block(k9(torch, T, Xt), reference_block(coo, m, n, Xt), "K9 between two forward products")
    y2 = forward()                                        # no new set_x
    if mode == sm.TJDS_MODE_ATOMIC:                       # (its order of summation varies: the bound, not the bits)
        rp, ci, v = sm.csr_from_coo(coo, m)
        scale = ob.csr_spmv(rp, ci, np.abs(v), np.abs(x))
        check_y(y2, ob.csr_spmv(rp, ci, v, x), scale, np.diff(rp))
        check_y(y1, ob.csr_spmv(rp, ci, v, x), scale, np.diff(rp))
    else:
        tr.assert_bits(y2, y1, "forward product after K9")
    assert T.plan_info() == info
    T.close()


def test_k9_is_the_same_under_every_setting_and_twice(torch):
    m, n, coo = load("memplus.mtx")
    X = np.random.default_rng(47).standard_normal((m, 17))
    ref = reference_block(coo, m, n, X)
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n))
    first = k9(torch, T, X)                               # before any set_x, mode or plan
    assert_block(first, ref, "first call")
    assert_block(k9(torch, T, X), first, "second call")
    T.set_x(dev(torch, np.full(n, np.nan)))               # the permuted operand is not read
    assert_block(k9(torch, T, X), first, "after set_x")
    for mode in TJDS_MODES:
        T.set_mode(mode)
        assert_block(k9(torch, T, X), first, "mode %d" % mode)
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    for tile in (256, 1024, 2048):
        T.set_tile(tile)
        assert_block(k9(torch, T, X), first, "tile %d" % tile)
    for min_tiles in (0, 4, 2):
        T.set_value_cache(min_tiles)
        assert_block(k9(torch, T, X), first, "value cache %d" % min_tiles)
    T.set_ref_quirks(True)
    assert_block(k9(torch, T, X), first, "ref-quirks")
    T.set_ref_quirks(False)
    assert_block(k9(torch, T, X), first, "ref-quirks off again")
    T.close()


# ------------------------------------------------------------------------------------------------------ 6. graph capture
def test_k9_is_captured_as_the_first_call_on_a_fresh_handle(torch):
    m, n, coo = load("memplus.mtx")
    k, ldx, ldy = 8, 10, 11
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n))
    dX = dev_X(torch, np.zeros((m, k)), ldx)
    buf, dY = guarded_Y(torch, n, k, ldy)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            T.spmm_transposed(dX, dY, stream=s)            # the handle's first call of any kind
    torch.cuda.synchronize()
    assert np.isnan(dY.cpu().numpy()).all(), "a captured call ran"
    rng = np.random.default_rng(48)
    for _ in range(2):
        X = rng.standard_normal((m, k))
        dX.copy_(torch.from_numpy(X))
        dY.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check_Y_guards(buf, n, k, ldy)
        assert_block(dY.cpu().numpy(), reference_block(coo, m, n, X), "graph replay")
    del g
    runs = [k9(torch, T, X, ldx, ldy) for _ in range(2)]
    assert_block(runs[0], reference_block(coo, m, n, X), "plain run after the graph")
    assert_block(runs[1], runs[0], "second plain run")
    T.close()


# --------------------------------------------------------------------------------------------------------------- 7. errors
def test_k9_invalid_arguments_write_nothing(torch):
    m, n, coo = load("curtis54.mtx")
    coo = coo[coo["row"] < m - 4]                               # (rows != cols below: X and Y differ in length)
    m -= 4
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n))
    L = sm.lib()
    k = 4
    X = np.ones((m, k))
    dX = dev_X(torch, X, k)
    buf, Y = guarded_Y(torch, n, k, k)
    both = torch.full(((2 * m + n) * k,), float("nan"), dtype=torch.float64, device="cuda")
    xp, yp, bp = dX.data_ptr(), Y.data_ptr(), both.data_ptr()
    cases = {"k = 0": (0, xp, k, yp, k), "k < 0": (-3, xp, k, yp, k), "ldx < k": (k, xp, k - 1, yp, k), "ldy < k": (k, xp, k, yp, k - 1),
             "null X": (k, None, k, yp, k), "null Y": (k, xp, k, None, k), "X is Y": (k, yp, k, yp, k),
             "Y begins on the last element of X": (k, bp, k, bp + 8 * (m * k - 1), k),
             "X begins on the last element of Y": (k, bp + 8 * (n * k - 1), k, bp, k),
             # X with leading dimension 2 k spans (m - 1) 2 k + k doubles: a Y that starts inside that span overlaps it
             "Y inside the span of a strided X": (k, bp, 2 * k, bp + 8 * ((m - 1) * 2 * k + k - 1), k)}
    assert (m - 1) * 2 * k + k - 1 + n * k <= both.numel()
    torch.cuda.synchronize()
    for what, (kk, x, ldx, y, ldy) in cases.items():
        rc = L.smvp_tjds_spmm_transposed(T._h, kk, x, ldx, y, ldy, None)
        assert rc == sm.ERR_INVALID, (what, rc)
        assert "smvp_tjds_spmm_transposed:" in L.smvp_last_error().decode(), what
    assert L.smvp_tjds_spmm_transposed(None, k, xp, k, yp, k, None) == sm.ERR_INVALID
    torch.cuda.synchronize()
    check_Y_guards(buf, n, k, k)
    assert np.isnan(Y.cpu().numpy()).all(), "a refused call wrote Y"
    assert torch.isnan(both).all()
    # adjacent, not overlapping: accepted (X in front of Y, and X with a leading dimension whose span ends where Y begins)
    both[:m * k] = 1.0
    assert L.smvp_tjds_spmm_transposed(T._h, k, bp, k, bp + 8 * m * k, k, None) == sm.OK
    torch.cuda.synchronize()
    ref = reference_block(coo, m, n, X)
    assert_block(both[m * k:(m + n) * k].view(n, k).cpu().numpy(), ref, "X and Y side by side")
    # the binding's checks on device tensors
    with pytest.raises(ValueError):
        T.spmm_transposed(dX[:-1], Y)
    with pytest.raises(ValueError):
        T.spmm_transposed(dX, Y.cpu())
    with pytest.raises(ValueError):
        T.spmm_transposed(dX, Y[:, :k - 1])
    with pytest.raises(sm.SmvpError):
        T.spmm_transposed_describe(0)
    torch.cuda.synchronize()
    check_Y_guards(buf, n, k, k)
    assert np.isnan(Y.cpu().numpy()).all(), "a refused call wrote Y"
    T.close()


# ------------------------------------------------------------------------------------------------------------ 8. describe
def test_k9_describe(torch):
    m, n, coo = load("memplus.mtx")
    t = sm.tjds_from_coo(coo, m + 3, n)                         # (rows != cols: the formula tells them apart)
    T = sm.TjdsMatrix(t)
    one = "tjds_spmm_transposed_columns<%d>"
    for k, name in ((1, one % 1), (16, one % 16), (17, " + ".join((one % 16, one % 1))), (40, " + ".join((one % 16, one % 16, one % 8)))):
        got, alg = T.spmm_transposed_describe(k)
        assert got == name
        assert alg == 12.0 * len(coo) + 4.0 * (t.num_diag + 1) + 4.0 * n + 8.0 * k * ((m + 3) + n)
    assert T.spmm_transposed_describe(1)[1] == T.transposed_describe()[1]      # K8's figure at k = 1
    got, alg = T.spmm_transposed_describe(2 ** 31 - 1)          # the largest k: the name stops at the buffer, the bytes are the formula's
    assert got.startswith(one % 16 + " + ") and len(got) == 255
    assert alg == 12.0 * len(coo) + 4.0 * (t.num_diag + 1) + 4.0 * n + 8.0 * (2 ** 31 - 1) * ((m + 3) + n)
    T.close()


# -------------------------------------------------------------------------------------------------------------- 9. at size
def at_size(torch, rows, cols, rp, ci, v, t_arrays, X, what):
    """K9 on the TJDS that smvp_tjds_from_coo_device builds against the oracle on the reference arrays t_arrays of A^T."""
    from test_gpu_parity import _coo_to_device

    k = X.shape[1]
    trp, tci, tv = t_arrays
    d_coo = _coo_to_device(torch, tr.coo_of_csr(rp, ci, v))
    t = sm.tjds_from_coo_device(d_coo, rows, cols, int(rp[-1]))
    del d_coo
    T = sm.TjdsMatrix(t)
    dX = dev(torch, X)
    buf, Y = guarded_Y(torch, cols, k, k)
    T.spmm_transposed(dX, Y)
    torch.cuda.synchronize()
    check_Y_guards(buf, cols, k, k)
    got = Y.cpu().numpy()
    T.close()
    for c in range(k):
        tr.assert_bits(got[:, c], ob.csr_spmv(trp, tci, tv, np.ascontiguousarray(X[:, c])), "%s, vector %d" % (what, c))


def test_k9_memplus_replicated_944_times_k16(torch):
    m, n, coo = load("memplus.mtx")
    copies = 944
    rp, ci, v = sm.csr_from_coo(coo, m)
    big = replicated(rp, ci, v, m, n, copies)
    t_big = replicated(*tr.transposed_csr(coo, n), n, m, copies)      # (I x A)^T = I x A^T
    X = np.random.default_rng(49).standard_normal((m * copies, 16))
    at_size(torch, m * copies, n * copies, *big, t_big, X, "memplus x944, k = 16")


def test_k9_config4_first_2_20_rows_k8(torch):
    N = 10_000_000
    M = 1 << 20
    rp, ci, v = sm.synth_csr(sm.SYNTH_UNIFORM, 12345, N, N, 32, row_end=M)
    X = np.random.default_rng(50).random((M, 8))
    at_size(torch, M, N, rp, ci, v, tr.transposed_csr(tr.coo_of_csr(rp, ci, v), N), X, "config 4, first 2^20 rows, k = 8")


def test_k9_offsets_into_x_and_y_beyond_2_31_elements(torch):
    """2^22 rows and columns, k = 3 as a slice of operands with a leading dimension of 1030: rows * ldx = cols * ldy = 2^32 +
    2^24.6 elements (34.6 GB each).  Few entries per column, half of them in rows and columns past 2^21, where row * ldx and
    perm * ldy no longer fit 31 bits, and some hundreds past 2^32 / 1030, where they no longer fit 32 (a leading dimension of
    1024 would stop one element short of that); the last row and the last column hold entries.  Y is compared by bits on the
    columns that hold entries; the others are +0.0; the padding columns and the guards keep their bits (all checked on the
    device)."""
    n = 1 << 22
    k, ld = 3, 1030
    rng = np.random.default_rng(51)
    used = np.unique(np.concatenate([rng.choice(n, 20000, replace=False), [0, n - 1, (1 << 21) - 1, 1 << 21]]))
    c = np.concatenate([used, rng.choice(used, 80000)])
    r = np.concatenate([rng.integers(0, n, len(c) - 2), [n - 1, 0]])
    coo = sm.make_coo(r, c, rng.uniform(-1, 1, len(c)))
    assert (r > 1 << 21).sum() > 10000 and (used > 1 << 21).sum() > 5000
    assert (r.astype(np.int64) * ld >= 2 ** 32).sum() > 300 and (used.astype(np.int64) * ld >= 2 ** 32).sum() > 50
    Xh = rng.standard_normal((n, k))
    ref = reference_block(coo, n, n, Xh)
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, n, n))
    Xfull = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
    Xfull[:, :k] = torch.from_numpy(Xh)
    buf = torch.empty(n * ld + 2 * G, dtype=torch.float64, device="cuda")
    buf.view(torch.int64).fill_(int(GUARD))
    Yfull = buf[G:G + n * ld].view(n, ld)
    Y = Yfull[:, :k]
    Y.fill_(float("nan"))
    T.spmm_transposed(Xfull[:, :k], Y)
    torch.cuda.synchronize()
    bits = buf.view(torch.int64)
    assert bool((bits[:G] == int(GUARD)).all()) and bool((bits[-G:] == int(GUARD)).all()), "wrote outside Y"
    for c0 in range(k, ld, 128):                                     # (in slabs: a mask of the whole block would be 4 GB)
        assert bool((Yfull[:, c0:c0 + 128].view(torch.int64) == int(GUARD)).all()), "a padding column k <= v < ldy was written"
    got = Y.cpu().numpy()
    T.close()
    del Xfull, buf, Yfull, Y
    torch.cuda.empty_cache()
    assert_block(got[used], ref[used], "columns that hold entries")
    assert (np.delete(got, used, axis=0).view(np.int64) == 0).all(), "a column without entries is not +0.0"
    assert_block(got, ref, "every column")
