"""smvp_tjds_spmm (K10) on the GPU: Y = A X for k vectors from a TJDS handle, every column of Y bit for bit the oracle's serial
TJDS loop on that column of X (tests/tjds_spmm.py: a row is summed in ascending TJDS position).  Every check is equality of bits
(NaN = NaN), on every column.

Y always lies in test_gpu_spmm.guarded_Y: GUARD words in front of and behind it, NaN in every slot the call writes, GUARD in
the padding columns k <= v < ldy, which must keep their bits (check_Y_guards).
"""
import ctypes as C

import numpy as np
import pytest

import adopted as ad
import oracle_binding as ob
import smvp_toolkit_amd as sm
import special_values as sv
import spmm_cases as sc
import transposed as tr
from conftest import SAMPLES
from parity import G, GUARD, check_guards, guarded_y
from test_gpu_spmm import KS, check_Y_guards, dev_X, guarded_Y
from test_gpu_transposed import TJDS_MODES, coo_from_lists, dev, load, replicated
from tjds_spmm import assert_block, reference_block

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 4, 8, 16)          # lanes per row of a pass; 64 / G rows per wavefront
BATCH = 8                          # entries per batch (kTjdsSpmmU)
ONE = "tjds_spmm_rows<%d>"


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def k10(torch, T, X, ldx=None, ldy=None, stream=None):
    """A X through smvp_tjds_spmm into a guarded Y; the host copy after the guard checks."""
    k = X.shape[1]
    ldx, ldy = ldx or k, ldy or k
    dX = dev_X(torch, X, ldx)
    buf, Y = guarded_Y(torch, T.rows, k, ldy)
    T.spmm(dX, Y, stream=stream)
    torch.cuda.synchronize()
    check_Y_guards(buf, T.rows, k, ldy)
    return Y.cpu().numpy()


def run_case(torch, rows, cols, coo, X, what, ldx=None, ldy=None):
    t = sm.tjds_from_coo(coo, rows, cols)
    T = sm.TjdsMatrix(t)
    Y = k10(torch, T, X, ldx, ldy)
    T.close()
    assert_block(Y, reference_block(t, X), what)
    return Y


def shuffled(coo, seed):
    """The same entries in another storage order: the TJDS order of a row is then not its CSR order."""
    return coo[np.random.default_rng(seed).permutation(len(coo))]


@pytest.fixture(scope="module")
def memplus():
    """memplus, its TJDS arrays, an operand of 17 vectors and the reference: computed once, left unchanged (the reference is
    read-only; the operand only goes through dev_X, which copies it to the device)."""
    m, n, coo = load("memplus.mtx")
    t = sm.tjds_from_coo(coo, m, n)
    X = np.random.default_rng(61).standard_normal((n, 17))
    ref = reference_block(t, X)
    ref.setflags(write=False)
    return m, n, coo, t, X, ref


# ----------------------------------------------------------------------------------------------------------- 1. samples
@pytest.mark.parametrize("name", SAMPLES)
def test_k10_sample_matrices_every_k_and_leading_dimension(torch, name):
    m, n, coo = load(name)
    t = sm.tjds_from_coo(coo, m, n)
    T = sm.TjdsMatrix(t)
    X = np.random.default_rng(62).standard_normal((n, max(KS)))
    ref = reference_block(t, X)
    for k in KS:
        for px, py in ((0, 0), (5, 7)):                          # tight operands, and column slices of wider arrays
            Y = k10(torch, T, X[:, :k], k + px, k + py)
            assert_block(Y, ref[:, :k], "%s k=%d ldx=k+%d ldy=k+%d" % (name, k, px, py))
    T.close()


# ------------------------------------------------------------------------------------------------------- 2. edge cases
def test_k10_edge_cases(torch):
    rng = np.random.default_rng(63)
    empty = sm.make_coo([], [], [])
    # no entries, rows > 0: every Y +0.0, sign bit included, whatever X holds -- and a NULL X is accepted
    Y = run_case(torch, 9, 4, empty, np.full((4, 5), -np.inf), "9 x 4 without entries", ldy=6)
    assert Y.shape == (9, 5) and (Y.view(np.int64) == 0).all()
    T = sm.TjdsMatrix(sm.tjds_from_coo(empty, 9, 4))
    buf, dY = guarded_Y(torch, 9, 3, 4)
    assert sm.lib().smvp_tjds_spmm(T._h, 3, None, 3, dY.data_ptr(), 4, None) == sm.OK
    torch.cuda.synchronize()
    check_Y_guards(buf, 9, 3, 4)
    assert (dY.cpu().numpy().view(np.int64) == 0).all()
    T.close()
    # no rows (Y is empty); no columns (every row +0.0); neither
    for rows, cols in ((0, 7), (5, 0), (0, 0)):
        Y = run_case(torch, rows, cols, empty, -rng.random((cols, 3)), "%d x %d" % (rows, cols), ldx=4, ldy=5)
        assert Y.shape == (rows, 3) and (Y.view(np.int64) == 0).all()
    # 1 x 1
    Y = run_case(torch, 1, 1, sm.make_coo([0], [0], [2.5]), np.array([[-3.0, 0.5]]), "1 x 1")
    assert Y.tolist() == [[-7.5, 1.25]]
    # one column
    lists = [[0] * int(rng.integers(0, 2)) for _ in range(777)]
    run_case(torch, 777, 1, coo_from_lists(777, lists, rng), rng.standard_normal((1, 4)), "one column")
    # one row of 1000 entries: alone, and among 300 short ones
    run_case(torch, 1, 1500, coo_from_lists(1, [sorted(rng.choice(1500, 1000, replace=False))], rng), rng.standard_normal((1500, 17)),
             "one row of 1000 entries")
    lists = [sorted(rng.choice(1500, int(rng.integers(0, 6)), replace=False)) for _ in range(300)]
    lists[123] = sorted(rng.choice(1500, 1000, replace=False))
    run_case(torch, 300, 1500, shuffled(coo_from_lists(300, lists, rng), 1), rng.standard_normal((1500, 9)), "a row of 1000 among short ones")
    # empty rows between full ones
    lists = [sorted(rng.choice(300, rng.integers(1, 40), replace=False)) if r % 3 else [] for r in range(200)]
    Y = run_case(torch, 200, 300, shuffled(coo_from_lists(200, lists, rng), 2), rng.standard_normal((300, 6)), "empty rows")
    assert (Y.view(np.int64)[np.arange(200) % 3 == 0] == 0).all()
    # M >> N and N >> M
    lists = [sorted(rng.choice(3, int(rng.integers(0, 4)), replace=False)) for _ in range(50000)]
    run_case(torch, 50000, 3, shuffled(coo_from_lists(50000, lists, rng), 3), rng.standard_normal((3, 4)), "tall")
    lists = [sorted(rng.choice(100000, int(rng.integers(0, 50)), replace=False)) for _ in range(100)]
    run_case(torch, 100, 100000, shuffled(coo_from_lists(100, lists, rng), 4), rng.standard_normal((100000, 9)), "wide")


# -------------------------------------------------------------------------------------------------------- 3. ragged rows
@pytest.mark.parametrize("g", GROUPS)
def test_k10_ragged_rows_every_remainder_of_the_batch(torch, g):
    """k = G vectors and 3 * (64 / G) + 1 rows -- three full wavefronts' worth and one row more -- whose lengths run through
    0 ... 17: every remainder of the batch of 8, rows that end inside the first, second and third batch, empty rows, a partial last
    wavefront.  Twice, the second run of lengths starting at 9, so that every length occurs for every G (13 rows at G = 16)."""
    rows, cols = 3 * (64 // g) + 1, 40
    seen = set()
    for start in (0, 9):
        rng = np.random.default_rng(64 + g + start)
        lengths = [(r + start) % 18 for r in range(rows)]
        seen |= set(lengths)
        lists = [sorted(rng.choice(cols, l, replace=False)) for l in lengths]
        coo = shuffled(coo_from_lists(rows, lists, rng), 5)
        t = sm.tjds_from_coo(coo, rows, cols)
        X = rng.standard_normal((cols, g))
        T = sm.TjdsMatrix(t)
        assert T.spmm_describe(g)[0] == ONE % g
        assert_block(k10(torch, T, X, g + 1, g + 2), reference_block(t, X), "G=%d rows=%d lengths from %d" % (g, rows, start))
        T.close()
    assert seen == set(range(18)) and {l % BATCH for l in seen} == set(range(BATCH))


# ------------------------------------------------------------------------------------------------------------- 4. passes
@pytest.mark.parametrize("k", (17, 33))
def test_k10_passes_of_16_vectors_and_a_rest(torch, memplus, k):
    m, n, coo, t, _, _ = memplus
    X = np.random.default_rng(65 + k).standard_normal((n, k))
    T = sm.TjdsMatrix(t)
    assert T.spmm_describe(k)[0] == " + ".join([ONE % 16] * (k // 16) + [ONE % 1])
    assert_block(k10(torch, T, X, k + 3, k + 1), reference_block(t, X), "memplus, k = %d" % k)
    T.close()


# ----------------------------------------------------------------------------------------------------- 5. repeated pairs
def test_k10_repeated_pairs_are_summed_in_tjds_storage_order(torch):
    # row 2 holds (2, 1) three times: 1e16 + 1 - 1e16 is 0 in storage order, 1 with the small value last
    coo = sm.make_coo([0, 2, 2, 2, 3], [0, 1, 1, 1, 1], [4.0, 1e16, 1.0, -1e16, 0.5])
    X = np.stack([np.ones(3), 2.0 * np.ones(3), -np.ones(3)], axis=1)
    Y = run_case(torch, 4, 3, coo, X, "repeated pairs")
    assert_block(Y, np.array([[4.0, 8.0, -4.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5, 1.0, -0.5]]), "the reference itself")
    other = coo[[0, 1, 3, 2, 4]]
    assert not tr.same_bits(reference_block(sm.tjds_from_coo(other, 4, 3), X), reference_block(sm.tjds_from_coo(coo, 4, 3), X)), \
        "the values must tell the orders apart"
    Y = run_case(torch, 4, 3, other, X, "repeated pairs, the other order")
    assert Y[2].tolist() == [1.0, 2.0, -1.0]


# ----------------------------------------------------------------------------------------------------- 6. special values
def k10_of(torch, rows, cols, rp, ci, val, X, ldx=None, ldy=None, seed=66):
    """A X through K10 on the TJDS of the pattern's entries in a shuffled storage order, and the reference over the same arrays."""
    nnz = int(rp[-1])
    coo = shuffled(sm.make_coo(sv.row_of_entries(rp), np.asarray(ci)[:nnz], np.asarray(val)[:nnz]), seed)
    t = sm.tjds_from_coo(coo, rows, cols)
    T = sm.TjdsMatrix(t)
    Y = k10(torch, T, X, ldx, ldy)
    T.close()
    return Y, reference_block(t, X)


@pytest.mark.parametrize("name", sv.SMALL)
def test_k10_scenarios_a_to_d(torch, name):
    """A: NaN / Inf in columns of X that no entry uses change no bit of Y.  B: a NaN / Inf in vector v of a used column changes
    vector v only, and there the class of a row is the serial loop's.  C: a stored 0.0 under an Inf gives NaN.  D: rows of -0.0
    products, zero operands and empty rows give +0.0."""
    rows, cols, rp, ci, u = sv.structure(name)
    o = sv.ordinary(rows, cols, rp, ci, u)
    val = o["val"]
    sv.assert_regime(name, "A", rows, cols, rp, ci, val, o["x_a"], u)
    sv.assert_regime(name, "B", rows, cols, rp, ci, val, o["x_b"])
    sv.assert_regime(name, "C", rows, cols, rp, ci, val, o["x_c"])
    keys = ("x", "x_a", "x_b", "x", "x_c", "x_a", "x")            # 7 vectors: a pass of G = 8 with one idle lane per group
    X = np.stack([o[key] for key in keys], axis=1)
    Y, ref = k10_of(torch, rows, cols, rp, ci, val, X, 9, 8)
    assert_block(Y, ref, name + ", A ... C")
    clean = Y[:, 0]
    assert np.isfinite(clean).all()
    for c, key in enumerate(keys):
        if key in ("x", "x_a"):                                  # unused columns poisoned, or a neighbour vector poisoned: no bit changes
            tr.assert_bits(Y[:, c], clean, "%s: vector %d (%s) beside poisoned vectors" % (name, c, key))
        else:
            sv.check_classes(Y[:, c], sv.row_classes(rp, ci, val, o[key]), "%s: vector %d (%s)" % (name, c, key))
        sv.check_no_negative_zero(Y[:, c], "%s: vector %d" % (name, c))
    # the poisoned vector alone (k = 1) and in a pass of its own (vector 16 of 17)
    for key in ("x_a", "x_b", "x_c"):
        Y1, ref1 = k10_of(torch, rows, cols, rp, ci, val, o[key].reshape(-1, 1), 1, 1)
        assert_block(Y1, ref1, "%s, %s alone" % (name, key))
        X17 = np.repeat(o["x"].reshape(-1, 1), 17, axis=1)
        X17[:, 16] = o[key]
        Y17, ref17 = k10_of(torch, rows, cols, rp, ci, val, X17)
        assert_block(Y17, ref17, "%s, %s as vector 16 of 17" % (name, key))
        for c in range(16):
            tr.assert_bits(Y17[:, c], clean, "%s: vector %d of 17 beside %s" % (name, c, key))
    # D
    for z in (np.zeros(cols), -np.zeros(cols)):
        sv.assert_regime(name, "D", rows, cols, rp, ci, val, z)
        Z = np.stack([z, -z, z], axis=1)
        Yz, refz = k10_of(torch, rows, cols, rp, ci, val, Z, 3, 4)
        assert_block(Yz, refz, name + ", D")
        assert (Yz.view(np.int64) == 0).all(), "%s, D: something other than +0.0" % name


@pytest.mark.parametrize("name", sv.SMALL)
def test_k10_scenarios_e_f_and_g(torch, name):
    """E: subnormal products and sums are kept.  F: sums of +-2^1020 overflow where the serial loop's do.  G: products that round
    -- a kernel that fuses the multiply into the add differs from the serial loop in most rows."""
    rows, cols, rp, ci, u = sv.structure(name)
    for scenario, (val, x) in (("E", sv.subnormal(rows, cols, rp, ci)), ("F", sv.overflowing(rows, cols, rp, ci)),
                               ("G", sv.rounded(rows, cols, rp, ci))):
        if scenario == "G":
            sv.assert_regime(name, "G", rows, cols, rp, ci, val, x)
        X = np.stack([x, -x, 0.5 * x, x, 2.0 * x if scenario != "F" else x], axis=1)     # (exact scalings: the bits follow the oracle's)
        Y, ref = k10_of(torch, rows, cols, rp, ci, val, X, 6, 5)
        if scenario == "E" and int(rp[-1]) >= 100:
            assert np.count_nonzero(ref[:, 0]) > 0 and np.abs(ref[:, 0]).max() < 2.0 ** -1022
        for c in range(X.shape[1]):
            sv.assert_exact(Y[:, c], ref[:, c], "%s, %s, vector %d" % (name, scenario, c))


def test_k10_a_slot_past_a_rows_end_never_multiplies(torch):
    """The last batch of a row re-reads the row's last entry in its unused slots and must leave them out with a select.  Every value
    is positive and X is +Inf in the column of the last entry (in TJDS order) of every third row: such a row sums to +Inf, and a
    kernel that multiplied the unused slots by 0.0 would add 0 * Inf = NaN to it.  Lengths 1 ... 17: every number of unused slots."""
    rng = np.random.default_rng(67)
    rows, cols = 180, 4000
    lists = [sorted(rng.choice(cols, 1 + r % 17, replace=False)) for r in range(rows)]
    coo = shuffled(coo_from_lists(rows, lists, rng), 6)
    coo["val"] = np.abs(coo["val"]) + 0.5
    t = sm.tjds_from_coo(coo, rows, cols)
    diag = np.searchsorted(t.start_pos, np.arange(t.nnz), side="right") - 1
    col_of = t.perm[np.arange(t.nnz) - t.start_pos[diag]]
    last = np.full(rows, -1)
    last[t.row_ind] = np.arange(t.nnz)                            # (ascending positions: the last write is the row's last entry)
    poisoned = col_of[last[np.arange(0, rows, 3)]]
    for k in (1, 2, 4, 8, 16):
        X = rng.uniform(0.5, 1.0, (cols, k))
        X[poisoned, k - 1] = np.inf
        T = sm.TjdsMatrix(t)
        Y = k10(torch, T, X, k + 1, k + 2)
        T.close()
        assert_block(Y, reference_block(t, X), "k = %d" % k)
        assert not np.isnan(Y).any() and (Y[::3, k - 1] == np.inf).all() and np.isfinite(Y[:, :k - 1]).all()
        assert {(len(l) % BATCH) for l in lists[::3]} == set(range(BATCH))


# ------------------------------------------------------------------------------------------------------- 7. independence
def test_k10_is_the_same_under_every_setting_and_twice(torch, memplus):
    m, n, coo, t, X, ref = memplus
    T = sm.TjdsMatrix(t)
    first = k10(torch, T, X)                               # before any set_x or change of mode
    assert_block(first, ref, "first call")
    assert_block(k10(torch, T, X), first, "second call")
    T.set_x(dev(torch, np.full(n, np.nan)))                # the permuted operand is not read
    assert_block(k10(torch, T, X), first, "after set_x")
    for mode in TJDS_MODES:
        T.set_mode(mode)
        assert_block(k10(torch, T, X), first, "mode %d" % mode)
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    for tile in (256, 1024, 2048):
        T.set_tile(tile)
        assert_block(k10(torch, T, X), first, "tile %d" % tile)
    for min_tiles in (0, 4, 2):
        T.set_value_cache(min_tiles)
        assert_block(k10(torch, T, X), first, "value cache %d" % min_tiles)
    T.set_ref_quirks(True)
    assert_block(k10(torch, T, X), first, "ref-quirks")
    T.set_ref_quirks(False)
    assert_block(k10(torch, T, X), first, "ref-quirks off again")
    T.close()
    # a handle whose first K10 call comes after the settings: the plan is built from the true arrays then too
    T = sm.TjdsMatrix(t)
    T.set_mode(sm.TJDS_MODE_TWO_PHASE)
    T.set_ref_quirks(True)
    assert_block(k10(torch, T, X), first, "first call under TWO_PHASE and ref-quirks")
    T.close()


@pytest.mark.parametrize("mode", TJDS_MODES)
def test_forward_tjds_product_is_undisturbed_by_k10(torch, mode):
    """spmv before and after a K10 call, no new set_x: identical bits in every mode.  The operands are adopted.py's integers, whose
    sums are exact in every order, so ATOMIC -- whose order varies from run to run -- has one answer too."""
    M = ad.mixed()
    coo = ad.coo(M.row_ptr, M.cols_a, M.val0)
    t = sm.tjds_from_coo(coo, M.rows, M.cols)
    T = sm.TjdsMatrix(t)
    T.set_mode(mode)
    info = T.plan_info()
    T.set_x(dev(torch, np.array(M.x)))

    def forward():
        buf, dy = guarded_y(torch, M.rows)
        T.zero_y(dy)
        T.spmv(dy)
        torch.cuda.synchronize()
        check_guards(buf, M.rows)
        return dy.cpu().numpy()

    y1 = forward()
    tr.assert_bits(y1, ad.reference(M.row_ptr, M.cols_a, M.val0, M.x), "forward product before K10")
    X = np.array(M.X)
    Y = k10(torch, T, X, 4, 5)
    assert_block(Y, reference_block(t, X), "K10 between two forward products")
    assert_block(Y, ad.reference(M.row_ptr, M.cols_a, M.val0, M.X), "K10 against the exact reference")
    tr.assert_bits(forward(), y1, "forward product after K10")                # no new set_x
    assert T.plan_info() == info
    T.close()


# ------------------------------------------------------------------------------------------------------ 8. graph capture
def test_k10_capture_is_refused_on_a_fresh_handle_and_replays_after_a_warm_call(torch, memplus):
    m, n, coo, t, _, _ = memplus
    k, ldx, ldy = 8, 10, 11
    T = sm.TjdsMatrix(t)
    dX = dev_X(torch, np.zeros((n, k)), ldx)
    buf, dY = guarded_Y(torch, m, k, ldy)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    # before any call: refused at once, nothing enqueued, no plan half-built, and the capture ends valid (dZ keeps it from being empty)
    refused = []
    with torch.cuda.stream(s):
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            dZ.add_(1.0)
            refused.append(sm.lib().smvp_tjds_spmm(T._h, k, dX.data_ptr(), ldx, dY.data_ptr(), ldy, s.cuda_stream))
    assert refused == [sm.ERR_INVALID]
    err = sm.lib().smvp_last_error().decode()
    assert err.startswith("smvp_tjds_spmm:") and "capture" in err
    assert T.spmm_describe(k)[2] == {"plan_bytes": 0.0, "build_ms": 0.0}
    g0.replay()                                                  # the capture is a valid graph: it holds the one add
    torch.cuda.synchronize()
    assert dZ.cpu().tolist() == [1.0] * 16
    del g0
    check_Y_guards(buf, m, k, ldy)
    assert np.isnan(dY.cpu().numpy()).all(), "a refused call wrote Y"
    # one call outside a capture, then a one-stream graph replayed twice with new operands
    with torch.cuda.stream(s):
        T.spmm(dX, dY, stream=s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            T.spmm(dX, dY, stream=s)
    rng = np.random.default_rng(68)
    for _ in range(2):
        X = rng.standard_normal((n, k))
        dX.copy_(torch.from_numpy(X))
        dY.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check_Y_guards(buf, m, k, ldy)
        assert_block(dY.cpu().numpy(), reference_block(t, X), "graph replay")
    del g
    T.close()


# --------------------------------------------------------------------------------------------------------------- 9. errors
def test_k10_invalid_arguments_write_nothing(torch):
    m, n, coo = load("curtis54.mtx")
    coo = coo[coo["row"] < m - 4]                               # (rows != cols below: X and Y differ in length)
    m -= 4
    t = sm.tjds_from_coo(coo, m, n)
    T = sm.TjdsMatrix(t)
    L = sm.lib()
    k = 4
    X = np.ones((n, k))
    dX = dev_X(torch, X, k)
    buf, Y = guarded_Y(torch, m, k, k)
    both = torch.full(((2 * n + m) * k,), float("nan"), dtype=torch.float64, device="cuda")
    xp, yp, bp = dX.data_ptr(), Y.data_ptr(), both.data_ptr()
    cases = {"k = 0": (0, xp, k, yp, k), "k < 0": (-3, xp, k, yp, k), "ldx < k": (k, xp, k - 1, yp, k), "ldy < k": (k, xp, k, yp, k - 1),
             "null X": (k, None, k, yp, k), "null Y": (k, xp, k, None, k), "X is Y": (k, yp, k, yp, k),
             "Y begins on the last element of X": (k, bp, k, bp + 8 * (n * k - 1), k),
             "X begins on the last element of Y": (k, bp + 8 * (m * k - 1), k, bp, k),
             # X with leading dimension 2 k spans (n - 1) 2 k + k doubles: a Y that starts inside that span overlaps it
             "Y inside the span of a strided X": (k, bp, 2 * k, bp + 8 * ((n - 1) * 2 * k + k - 1), k)}
    assert (n - 1) * 2 * k + k - 1 + m * k <= both.numel()
    torch.cuda.synchronize()
    for what, (kk, x, ldx, y, ldy) in cases.items():
        rc = L.smvp_tjds_spmm(T._h, kk, x, ldx, y, ldy, None)
        assert rc == sm.ERR_INVALID, (what, rc)
        assert L.smvp_last_error().decode().startswith("smvp_tjds_spmm:"), what
    assert L.smvp_tjds_spmm(None, k, xp, k, yp, k, None) == sm.ERR_INVALID
    assert L.smvp_last_error().decode().startswith("smvp_tjds_spmm:")
    torch.cuda.synchronize()
    check_Y_guards(buf, m, k, k)
    assert np.isnan(Y.cpu().numpy()).all(), "a refused call wrote Y"
    assert torch.isnan(both).all()
    assert T.spmm_describe(k)[2]["plan_bytes"] == 0              # nothing was built either
    # adjacent, not overlapping: accepted (X in front of Y, the span of X ending where Y begins)
    both[:n * k] = 1.0
    assert L.smvp_tjds_spmm(T._h, k, bp, k, bp + 8 * n * k, k, None) == sm.OK
    torch.cuda.synchronize()
    assert_block(both[n * k:(n + m) * k].view(m, k).cpu().numpy(), reference_block(t, X), "X and Y side by side")
    # the binding's checks on device tensors
    with pytest.raises(ValueError):
        T.spmm(dX[:-1], Y)
    with pytest.raises(ValueError):
        T.spmm(dX, Y.cpu())
    with pytest.raises(ValueError):
        T.spmm(dX, Y[:, :k - 1])
    with pytest.raises(sm.SmvpError):
        T.spmm_describe(0)
    torch.cuda.synchronize()
    check_Y_guards(buf, m, k, k)
    assert np.isnan(Y.cpu().numpy()).all(), "a refused call wrote Y"
    T.close()


# ------------------------------------------------------------------------------------------------------ 10. adopted arrays
def test_k10_over_adopted_arrays_sees_val_changed_in_place_and_leaves_them_alone(torch):
    from test_gpu_adopted import bits_equal, coo_to_device

    M = ad.mixed()
    coo = ad.coo(M.row_ptr, M.cols_a, M.val0)
    t_host = sm.tjds_from_coo(coo, M.rows, M.cols)
    t_dev = sm.tjds_from_coo_device(coo_to_device(torch, coo), M.rows, M.cols, len(coo))
    tensors = (t_dev.perm, t_dev.start_pos, t_dev.row_ind, t_dev.val)
    clones = [a.clone() for a in tensors]
    X = np.array(M.X)
    T = sm.TjdsMatrix(t_dev)
    Y = k10(torch, T, X, 5, 4)                                           # builds the plan
    assert_block(Y, reference_block(t_host, X), "adopted, the serial TJDS loop")
    assert_block(Y, ad.reference(M.row_ptr, M.cols_a, M.val0, M.X), "adopted, the exact reference")
    for a, c in zip(tensors, clones):
        assert bits_equal(torch, a, c), "the plan build modified an adopted array"
    t_dev.val.mul_(-3.0)                                                 # in place; no call on the handle before the next product
    torch.cuda.synchronize()
    assert_block(k10(torch, T, X, 5, 4), ad.reference(M.row_ptr, M.cols_a, -3.0 * M.val0, M.X), "val scaled in place")
    t_dev.val.copy_(clones[3])
    torch.cuda.synchronize()
    assert_block(k10(torch, T, X, 5, 4), Y, "val put back")
    T.close()
    for a, c in zip(tensors, clones):
        assert bits_equal(torch, a, c), "an adopted array was modified or freed"
    T = sm.TjdsMatrix(t_dev)                                             # the arrays are alive: a new handle over them
    assert_block(k10(torch, T, X), Y, "a new handle over the same arrays")
    T.close()


# ----------------------------------------------------------------------------------------------------------- 11. describe
def test_k10_describe(torch):
    m, n, coo = load("memplus.mtx")
    t = sm.tjds_from_coo(coo, m + 3, n)                         # (rows != cols: the formulas tell them apart)
    T = sm.TjdsMatrix(t)
    rows, nnz = m + 3, len(coo)
    alg_of = lambda k: 12.0 * nnz + 4.0 * (t.num_diag + 1) + 4.0 * n + 8.0 * k * (rows + n)
    names = ((1, ONE % 1), (2, ONE % 2), (3, ONE % 4), (8, ONE % 8), (16, ONE % 16), (17, " + ".join((ONE % 16, ONE % 1))),
             (40, " + ".join((ONE % 16, ONE % 16, ONE % 8))))
    before = T.plan_info()
    for k, name in names:
        got, alg, plan = T.spmm_describe(k)
        assert got == name and alg == alg_of(k)
        assert plan == {"plan_bytes": 0.0, "build_ms": 0.0}
    X = np.random.default_rng(69).standard_normal((n, 3))
    assert_block(k10(torch, T, X), reference_block(t, X), "memplus with three empty rows")
    for k, name in names:
        got, alg, plan = T.spmm_describe(k)
        assert got == name and alg == alg_of(k)
        assert plan["plan_bytes"] == 4.0 * (rows + 1) + 8.0 * nnz + 4.0 * rows and plan["build_ms"] > 0
    after = T.plan_info()
    assert after == before and set(after) == {"matrix_bytes", "plan_bytes", "build_ms"}
    with pytest.raises(sm.SmvpError):
        T.spmm_describe(0)
    got, alg, _ = T.spmm_describe(2 ** 31 - 1)                  # the largest k: the name stops at the buffer, the bytes are the formula's
    assert got.startswith(ONE % 16 + " + ") and len(got) == 255
    assert alg == alg_of(2 ** 31 - 1)
    name = C.create_string_buffer(8)                                  # cut at cap
    assert sm.lib().smvp_tjds_spmm_describe(T._h, 17, name, 8, None, None) == sm.OK
    assert name.value == (ONE % 16)[:7].encode()
    T.close()


# ---------------------------------------------------------------------------------------------- 12. beyond one sorted block
def test_k10_memplus_replicated_64_times_k16(torch):
    """kron(I_64, memplus): 64 x 17758 rows, many sorted blocks of 4096 rows, k = 16.  A copy's rows keep their TJDS order under
    replication, so every copy's block of Y has the bits of the single matrix's reference on that copy's block of X."""
    m, n, coo = load("memplus.mtx")
    copies = 64
    t_one = sm.tjds_from_coo(coo, m, n)
    rp, ci, v = sm.csr_from_coo(coo, m)
    big = tr.coo_of_csr(*replicated(rp, ci, v, m, n, copies))
    t = sm.tjds_from_coo(big, m * copies, n * copies)
    X = np.random.default_rng(70).standard_normal((n * copies, 16))
    T = sm.TjdsMatrix(t)
    Y = k10(torch, T, X)
    T.close()
    for c in range(copies):
        assert_block(Y[c * m:(c + 1) * m], reference_block(t_one, X[c * n:(c + 1) * n]), "copy %d" % c)


# ------------------------------------------------------------------------------------------ 13. offsets past 2^31 elements
def test_k10_offsets_into_x_and_y_beyond_2_31_elements(torch):
    """2^22 rows and columns, k = 3 as a slice of operands with a leading dimension of 1030: cols * ldx = rows * ldy = 2^32 +
    2^24.6 elements (34.6 GB each).  Few entries per row, half of them in rows and columns past 2^21, where col * ldx and
    row * ldy no longer fit 31 bits, and some hundreds past 2^32 / 1030, where they no longer fit 32; the last row and the last
    column hold entries.  Y is compared by bits on the rows that hold entries; the others are +0.0; the padding columns and the
    guards keep their bits (all checked on the device)."""
    n = 1 << 22
    k, ld = 3, 1030
    rng = np.random.default_rng(71)
    used = np.unique(np.concatenate([rng.choice(n, 20000, replace=False), [0, n - 1, (1 << 21) - 1, 1 << 21]]))
    r = np.concatenate([used, rng.choice(used, 80000)])
    c = np.concatenate([rng.integers(0, n, len(r) - 2), [n - 1, 0]])
    coo = sm.make_coo(r, c, rng.uniform(-1, 1, len(r)))
    assert (c > 1 << 21).sum() > 10000 and (used > 1 << 21).sum() > 5000
    assert (c.astype(np.int64) * ld >= 2 ** 32).sum() > 300 and (used.astype(np.int64) * ld >= 2 ** 32).sum() > 50
    Xh = rng.standard_normal((n, k))
    t = sm.tjds_from_coo(coo, n, n)
    ref = reference_block(t, Xh)
    T = sm.TjdsMatrix(t)
    Xfull = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
    Xfull[:, :k] = torch.from_numpy(Xh)
    buf = torch.empty(n * ld + 2 * G, dtype=torch.float64, device="cuda")
    buf.view(torch.int64).fill_(int(GUARD))
    Yfull = buf[G:G + n * ld].view(n, ld)
    Y = Yfull[:, :k]
    Y.fill_(float("nan"))
    T.spmm(Xfull[:, :k], Y)
    torch.cuda.synchronize()
    bits = buf.view(torch.int64)
    assert bool((bits[:G] == int(GUARD)).all()) and bool((bits[-G:] == int(GUARD)).all()), "wrote outside Y"
    for c0 in range(k, ld, 128):                                     # (in slabs: a mask of the whole block would be 4 GB)
        assert bool((Yfull[:, c0:c0 + 128].view(torch.int64) == int(GUARD)).all()), "a padding column k <= v < ldy was written"
    got = Y.cpu().numpy()
    T.close()
    del Xfull, buf, Yfull, Y
    torch.cuda.empty_cache()
    assert_block(got[used], ref[used], "rows that hold entries")
    assert (np.delete(got, used, axis=0).view(np.int64) == 0).all(), "a row without entries is not +0.0"
    assert_block(got, ref, "every row")


# -------------------------------------------------------------------------------------- 14. row counts at the launch edges
def test_k10_row_counts_at_the_launch_edges(torch):
    """K7's launch arithmetic is K10's: row counts around 256 / G (a workgroup), 8 * 256 / G (one round of workgroups over the
    XCDs) and 4096 (a sorted block) for every G, the entries of spmm_cases.row_count_case in a shuffled storage order.  A wrong
    `group`, a truncated last round or a block left out of the plan leaves rows NaN at some count and not at others.  One fresh
    handle per count serves every k: its plan is built by the first call."""
    for rows in sc.ROW_COUNTS:
        n, cols, rp, ci, val, X = sc.row_count_case(rows)
        t = sm.tjds_from_coo(shuffled(tr.coo_of_csr(rp, ci, val), rows), rows, cols)
        ref = reference_block(t, X)
        T = sm.TjdsMatrix(t)
        for k in sc.ROW_COUNT_KS:
            assert_block(k10(torch, T, X[:, :k], k + 1, k + 2), ref[:, :k], "%d rows, k = %d" % (rows, k))
        T.close()


# --------------------------------------------------------------------------------------------------------------- 15. fuzz
@pytest.mark.parametrize("seed", sc.FUZZ_SEEDS)
def test_k10_fuzz_random_shapes_k_and_leading_dimensions(torch, seed):
    """Random shapes across up to four sorted blocks, every style of row lengths, k = 1 ... 40 and padded leading dimensions,
    the entries in a shuffled storage order: the serial TJDS loop's bits on every column, and the same bits from a second call
    on the same handle (the plan built by the first)."""
    rows, cols, rp, ci, val, k, ldx, ldy, X = sc.block_fuzz(seed)
    what = "fuzz %d: %d x %d, k=%d ldx=%d ldy=%d" % (seed, rows, cols, k, ldx, ldy)
    t = sm.tjds_from_coo(shuffled(tr.coo_of_csr(rp, ci, val), seed), rows, cols)
    T = sm.TjdsMatrix(t)
    first = k10(torch, T, X, ldx, ldy)
    second = k10(torch, T, X, ldx, ldy)
    T.close()
    assert_block(first, reference_block(t, X), what)
    assert_block(second, first, what + ", second call")
