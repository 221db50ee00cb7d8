"""Host checks of tests/special_values.py: the row-class rule against a plain Python loop in several orders of summation, the
conditions every scenario's input has to meet, and -- the point of the file -- that the assertions test_gpu_special_values.py
uses reject numpy models of the wrong kernels they are there for, and accept the oracle's own result."""
import numpy as np
import pytest

import oracle_binding as ob
import parity
import smvp_toolkit_amd as sm
import special_values as sv


def python_loop(row_ptr, col_ind, val, x, rng=None, seed_first=False, skip_zeros=False, flush=False):
    """acc = 0.0; acc += val[j] * x[col[j]] per row in plain Python, the row's entries in storage order or shuffled by rng.
    The flags turn it into the wrong kernels: accumulator seeded with the first product, stored zeros skipped, subnormal
    products flushed to zero."""
    y = np.zeros(len(row_ptr) - 1)
    tiny = np.finfo(np.float64).tiny
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(y)):
            js = np.arange(row_ptr[r], row_ptr[r + 1])
            if rng is not None:
                js = rng.permutation(js)
            acc, first = np.float64(0.0), True
            for j in js:
                if skip_zeros and val[j] == 0:
                    continue
                p = np.float64(val[j]) * np.float64(x[col_ind[j]])
                if flush and abs(p) < tiny:
                    p = np.float64(0.0)
                acc = p if (seed_first and first) else acc + p
                first = False
            y[r] = acc
    return y


def small(name="fuzz:0"):
    rows, cols, rp, ci, u = sv.structure(name)
    return rows, cols, rp, ci, u, sv.ordinary(rows, cols, rp, ci, u)


def scale_terms(rp, ci, val, x):
    with np.errstate(invalid="ignore"):
        return ob.csr_spmv(rp, ci, np.abs(val), np.abs(x)), np.diff(rp)


# ------------------------------------------------------------------------------------------------------------ the helpers
def test_check_bits_is_the_transposed_suites_and_tells_zeros_apart():
    import transposed

    assert sv.check_bits is transposed.assert_bits
    sv.check_bits(np.array([0.0, np.nan, -np.inf]), np.array([0.0, -np.nan, -np.inf]), "any NaN equals any NaN")
    for y, ref in (([-0.0], [0.0]), ([0.0], [-0.0]), ([1.0], [np.nan]), ([np.inf], [-np.inf]), ([5e-324], [0.0])):
        with pytest.raises(AssertionError):
            sv.check_bits(np.array(y), np.array(ref), "differs")
    with pytest.raises(AssertionError):
        sv.check_no_negative_zero(np.array([1.0, -0.0]))
    sv.check_no_negative_zero(np.array([1.0, 0.0, -1.0, np.nan]))


@pytest.mark.parametrize("name", ["fuzz:0", "fuzz:1", "fuzz:2", "edge:exactly_33_per_row", "edge:leading_and_trailing_empty_rows"])
def test_row_classes_equal_the_serial_loop_in_every_order(name):
    """Fact 1: with small finite products the class of a row does not depend on the order of its sum."""
    rows, cols, rp, ci, u, o = small(name)
    for key in ("x_b", "x_c", "x_a", "x"):
        want = sv.row_classes(rp, ci, o["val"], o[key])
        assert np.array_equal(sv.classes_of(ob.csr_spmv(rp, ci, o["val"], o[key])), want), key
        assert np.array_equal(sv.classes_of(python_loop(rp, ci, o["val"], o[key])), want), key
        for seed in range(3):
            shuffled = python_loop(rp, ci, o["val"], o[key], rng=np.random.default_rng(seed))
            assert np.array_equal(sv.classes_of(shuffled), want), (key, seed)
    if name == "fuzz:0":
        cls = sv.row_classes(rp, ci, o["val"], o["x_b"])
        assert all((cls == c).sum() >= 10 for c in (sv.NAN, sv.PINF, sv.NINF)) and (cls == sv.FINITE).mean() > 0.9


def test_python_loop_is_the_oracle():
    rows, cols, rp, ci, u, o = small("fuzz:1")
    sv.check_bits(python_loop(rp, ci, o["val"], o["x_b"]), ob.csr_spmv(rp, ci, o["val"], o["x_b"]), "plain Python against the oracle")


# ---------------------------------------------------------------------------------------------------------------- regimes
@pytest.mark.parametrize("name", sv.SMALL)
def test_every_scenario_reaches_its_regime(name):
    """The conditions of every scenario on the structures that bear them (special_values.REGIME), from the oracle alone; every
    finite product stays below 1e3; the exact scenarios are exact: the oracle's result does not depend on the order."""
    rows, cols, rp, ci, u, o = small(name)
    nnz = int(rp[-1])
    assert not np.isin(ci[:nnz], u).any() and (len(u) >= 16) == (cols >= sv.MIN_COLS_A)
    held = {"A": sv.assert_regime(name, "A", rows, cols, rp, ci, o["val"], o["x_a"], u)["held"],
            "B": sv.assert_regime(name, "B", rows, cols, rp, ci, o["val"], o["x_b"])["held"],
            "C": sv.assert_regime(name, "C", rows, cols, rp, ci, o["val"], o["x_c"])["held"]}
    d = [sv.assert_regime(name, "D", rows, cols, rp, ci, o["val"], z)["held"] for z in (np.zeros(cols), -np.zeros(cols))]
    held["D"] = all(d)
    held["G"] = sv.assert_regime(name, "G", rows, cols, rp, ci, *sv.rounded(rows, cols, rp, ci))["held"]
    for s in "ABCDG":
        assert held[s] or name not in sv.REGIME[s]
    for key in ("x", "x_a", "x_b", "x_c"):
        with np.errstate(invalid="ignore"):
            p = o["val"] * o[key][ci[:nnz]] if nnz else np.zeros(0)
        assert np.all(np.abs(p[np.isfinite(p)]) <= 1e3)
    # A: the clean product is finite everywhere and the poison changes nothing in the oracle either
    sv.assert_unreferenced(ob.csr_spmv(rp, ci, o["val"], o["x_a"]), ob.csr_spmv(rp, ci, o["val"], o["x"]), name)
    # D: never -0.0, whatever the sign of the zeros
    for z in (np.zeros(cols), -np.zeros(cols)):
        sv.assert_exact(ob.csr_spmv(rp, ci, o["val"], z), np.zeros(rows), name + ", scenario D")
    # E and F: exact in the oracle and in a shuffled plain loop (small structures only: the loop is Python)
    for label, (val, x) in (("E", sv.subnormal(rows, cols, rp, ci)), ("F", sv.overflowing(rows, cols, rp, ci))):
        ref = ob.csr_spmv(rp, ci, val, x)
        sv.check_no_negative_zero(ref, label)
        if nnz <= 30_000:
            sv.check_bits(python_loop(rp, ci, val, x, rng=np.random.default_rng(5)), ref, "%s, scenario %s shuffled" % (name, label))
        if label == "E" and nnz:
            assert np.abs(ref).max() < 2.0 ** -1022 and (nnz < 100 or np.count_nonzero(ref) > 0)
        if label == "F" and nnz:
            lens = np.diff(rp)
            assert np.array_equal(np.isinf(ref), lens >= 16) and np.array_equal(np.abs(ref[lens < 16]), lens[lens < 16] * 2.0 ** 1020)


def test_every_scenario_has_structures_that_bear_it():
    for s, names in sv.REGIME.items():
        assert len(names) >= 6 and set(names) <= set(sv.STRUCTURES), s
    narrow = [n for n in sv.STRUCTURES if n not in sv.REGIME["A"]]
    assert all(sv.structure(n)[1] < sv.MIN_COLS_A for n in narrow) and len(narrow) == 4   # A is refused there, not passed silently
    with pytest.raises(AssertionError):
        rows, cols, rp, ci, u, o = small("fuzz:3")
        sv.assert_regime("fuzz:0", "B", rows, cols, rp, ci, o["val"], o["x"])               # nothing poisoned: no regime
    lens = np.array(sv.STRADDLE_LENS)
    assert {15, 16, 32, 33, 256, 257, 1024, 1025} <= set(lens.tolist())


# ------------------------------------------------------------------------------- the checks catch the kernels they are for
def test_a_catches_padding_multiplied_by_zero_and_a_staged_tail_that_reads_too_far():
    """(i) a padding entry computed as 0.0 * x[0] and added; (ii) the tail of the last column block staged from x instead of
    0.0, so that the last element of x meets a padding value of 0.0 in the last row.  Both give NaN where x holds NaN or Inf
    and nothing at all on finite operands -- which is all the parity suite feeds."""
    rows, cols, rp, ci, u, o = small("fuzz:0")
    clean = ob.csr_spmv(rp, ci, o["val"], o["x"])
    good = ob.csr_spmv(rp, ci, o["val"], o["x_a"])
    sv.assert_unreferenced(good, clean, "the oracle")
    assert not np.isfinite(o["x_a"][0]) and not np.isfinite(o["x_a"][cols - 1])
    with np.errstate(invalid="ignore"):
        wrong_i = good + 0.0 * o["x_a"][0]
        wrong_ii = good.copy()
        wrong_ii[-1] += 0.0 * o["x_a"][cols - 1]
    for wrong in (wrong_i, wrong_ii):
        with pytest.raises(AssertionError):
            sv.assert_unreferenced(wrong, clean, "model")
        # ... and the finite operand lets both through: the gap this suite closes
        same = wrong.copy()
        same[np.isnan(same)] = clean[np.isnan(same)]
        sv.assert_unreferenced(same, clean, "on finite operands")


def test_d_catches_an_accumulator_seeded_with_the_first_product():
    """(iii): the serial loop starts from +0.0, so a row of -0.0 products sums to +0.0; a kernel that starts from the row's
    first product gives -0.0 -- equal under np.array_equal, a different line in the report."""
    rows, cols, rp, ci, u, o = small("fuzz:0")
    for z in (np.zeros(cols), -np.zeros(cols)):
        good = ob.csr_spmv(rp, ci, o["val"], z)
        sv.assert_exact(good, np.zeros(rows), "the oracle")
        wrong = python_loop(rp, ci, o["val"], z, seed_first=True)
        assert np.array_equal(wrong, good)                                   # what the existing exact checks see
        with pytest.raises(AssertionError):
            sv.assert_exact(wrong, np.zeros(rows), "model")
    # without stored zeros and on ordinary operands the two loops agree to the bit: no test on such inputs can tell them apart
    v = np.where(o["val"] == 0, 0.5, o["val"])
    sv.check_bits(python_loop(rp, ci, v, o["x"], seed_first=True), ob.csr_spmv(rp, ci, v, o["x"]), "ordinary operands")


def test_c_catches_stored_zeros_that_are_skipped():
    """(iv): 0.0 * Inf is NaN and the row must say so; a kernel that drops val == 0 entries leaves it finite (or +-Inf)."""
    rows, cols, rp, ci, u, o = small("fuzz:0")
    val, x = o["val"], o["x_c"]
    ref = ob.csr_spmv(rp, ci, val, x)
    scale, terms = scale_terms(rp, ci, val, x)
    cls = sv.row_classes(rp, ci, val, x)
    sv.assert_against_oracle(ref, ref, scale, terms, cls, "the oracle", serial=np.ones(rows, bool))
    wrong = python_loop(rp, ci, val, x, skip_zeros=True)
    assert (np.isnan(ref) & ~np.isnan(wrong)).sum() >= 10
    with pytest.raises(AssertionError):
        sv.assert_against_oracle(wrong, ref, scale, terms, cls, "model")
    with pytest.raises(AssertionError):
        parity.check_y(wrong, ref, scale, terms)                             # (check_y alone catches it too)
    # zeros under ordinary operands change nothing
    sv.check_bits(python_loop(rp, ci, val, o["x"], skip_zeros=True), ob.csr_spmv(rp, ci, val, o["x"]), "ordinary operands")


def test_e_catches_subnormal_products_flushed_to_zero():
    """(v)."""
    rows, cols, rp, ci, u, _ = small("fuzz:0")
    val, x = sv.subnormal(rows, cols, rp, ci)
    ref = ob.csr_spmv(rp, ci, val, x)
    sv.assert_exact(ref, ref, "the oracle")
    sv.assert_exact(python_loop(rp, ci, val, x, rng=np.random.default_rng(1)), ref, "a shuffled loop")
    assert np.count_nonzero(ref) > 0.3 * rows
    with pytest.raises(AssertionError):
        sv.assert_exact(python_loop(rp, ci, val, x, flush=True), ref, "model")


def test_g_catches_a_fused_multiply_add():
    """(vi): with full mantissas fma(a, x, acc) and round(a x) + acc differ in at least half the rows of two entries or more."""
    rows, cols, rp, ci, u, _ = small("fuzz:4")
    val, x = sv.rounded(rows, cols, rp, ci)
    ref = ob.csr_spmv(rp, ci, val, x)
    sv.check_bits(python_loop(rp, ci, val, x), ref, "plain Python against the oracle")
    pick = np.flatnonzero(np.diff(rp) >= 2)[:300]
    fused = sv.fma_serial(rp, ci, val, x, pick)
    assert (fused != ref[pick]).mean() >= 0.5
    scale, terms = scale_terms(rp, ci, val, x)
    wrong = ref.copy()
    wrong[pick] = fused
    parity.check_y(wrong, ref, scale, terms)                                 # inside the rounding bound: only the bits tell
    with pytest.raises(AssertionError):
        sv.assert_against_oracle(wrong, ref, scale, terms, np.zeros(rows, int), "model", serial=np.ones(rows, bool))
    sv.assert_against_oracle(ref, ref, scale, terms, np.zeros(rows, int), "the oracle", serial=np.ones(rows, bool))
    # fma_serial itself: on exactly representable products it is the plain loop
    vi, xi = np.round(val * 8), np.round(x * 8)
    sv.check_bits(sv.fma_serial(rp, ci, vi, xi, pick), ob.csr_spmv(rp, ci, vi, xi)[pick], "fma of exact products")


# ----------------------------------------------------------------------------------------------- the reader and the report
def test_matrix_market_reader_on_infinity_and_nan_tokens(tmp_path):
    """The CLI test writes inf / -inf / nan values into a Matrix Market file: the reader must give what strtod gives."""
    toks = ["inf", "-inf", "nan", "0", "-0", "Infinity", "NaN", "-nan", "1.5"]
    p = tmp_path / "special.mtx"
    p.write_text("%%MatrixMarket matrix coordinate real general\n9 9 9\n" + "".join("%d %d %s\n" % (i + 1, i + 1, t) for i, t in enumerate(toks)))
    want = np.array([float(t) for t in toks])
    for threads in (1, 4):
        sm.set_option("mm_threads", threads)
        tc, m, n, coo = sm.mm_read_coo(str(p))
        assert (m, n, len(coo)) == (9, 9, 9)
        sv.check_bits(coo["val"], want, "reader, %d threads" % threads)      # (a NaN's sign and payload are not part of it)
    assert ob.fmt_g(np.array([np.inf, -np.inf, 0.0, -0.0])) == ["inf", "-inf", "0", "-0"]
