"""Host checks of tests/power_iteration.py: the host chain over the oracle's product with normalise() is the oracle's own power
iteration bit for bit, and every constructed regime really occurs -- the largest magnitude of every peak iterate at the chosen
index, an exactly zero iterate from step 2, exactly one +Inf row, a subnormal maximum, NaN rows that are neither none nor all,
partial sums below 2^53 -- so that test_gpu_power_iteration.py compares the library with inputs that are what they claim."""
import numpy as np
import pytest

import power_iteration as pi
from transposed import assert_bits

ORDINARY = {"short": pi.short, "long": pi.long, "shuffled": pi.shuffled}
PEAKS = [(pi.PEAK_SMALL[0], p, s) for p in pi.PEAK_SMALL[1] for s in (1, -1)] + \
        [(pi.PEAK_LARGE[0], p, s) for p in pi.PEAK_LARGE[1] for s in (1, -1)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------- the pure functions
def test_normalise_by_cases():
    nan, inf = np.nan, np.inf
    assert_bits(pi.normalise([1.0, -4.0, 2.0]), [0.25, -1.0, 0.5], "a negative entry holds the maximum")
    assert_bits(pi.normalise([nan, 3.0, -1.5]), [nan, 1.0, -0.5], "NaN entries take no part in the maximum")
    assert_bits(pi.normalise([1.0, -2.0, inf, -inf, 0.0, -0.0]), [0.0, -0.0, nan, nan, 0.0, -0.0], "an infinite maximum")
    assert_bits(pi.normalise([0.0, -0.0, 0.0]), [0.0, -0.0, 0.0], "a zero maximum leaves the vector alone")
    assert_bits(pi.normalise([nan, nan]), [nan, nan], "nothing to take a maximum of")
    assert_bits(pi.normalise([]), [], "no elements")
    assert_bits(pi.normalise([15e-324, -40e-324, 5e-324]), [0.375, -1.0, 0.125], "a subnormal maximum")
    y = np.array([1.0, 3.0])
    out = pi.normalise(y)
    assert out is not y and y[1] == 3.0 and out[0] == 1.0 / 3.0


def test_host_chain_feeds_every_result_back():
    seen = []

    def product(x):
        seen.append(x.copy())
        return np.array([x[1] * 2.0, -x[0] * 4.0])

    raw, its = pi.host_chain(product, [1.0, 1.0], 3, normalize=True)
    assert [r.tolist() for r in raw] == [[2.0, -4.0], [-2.0, -2.0], [-2.0, 4.0]]
    assert [i.tolist() for i in its] == [[0.5, -1.0], [-1.0, -1.0], [-0.5, 1.0]]
    assert [s.tolist() for s in seen] == [o.tolist() for o in pi.operands([1.0, 1.0], its)]
    raw, its = pi.host_chain(product, [1.0, 1.0], 2, normalize=False)
    assert [i.tolist() for i in its] == [r.tolist() for r in raw] == [[2.0, -4.0], [-8.0, -8.0]]
    assert its[0] is not raw[0]


# ------------------------------------------------------------------------------------------- the chain is the oracle's iteration
@pytest.mark.parametrize("name", sorted(ORDINARY))
@pytest.mark.parametrize("normalize", [False, True])
def test_chain_over_the_oracle_product_is_the_oracle_iteration(name, normalize):
    M = ORDINARY[name]()
    for x0 in (pi.ones(M), pi.random_x(M)):
        raw, its = pi.host_chain(M.spmv, x0, max(pi.STEPS), normalize)
        for steps in pi.STEPS:
            assert_bits(its[steps - 1], M.iterate(x0, steps, normalize), "%s, %d steps, normalize %s" % (name, steps, normalize))


@pytest.mark.parametrize("n,p,sign", [t for t in PEAKS if t[0] == pi.PEAK_SMALL[0]][:4] + [t for t in PEAKS if t[0] == pi.PEAK_LARGE[0]][:2])
@pytest.mark.parametrize("normalize", [False, True])
def test_chain_over_the_oracle_product_is_the_oracle_iteration_on_peaks(n, p, sign, normalize):
    M = pi.peak(n, p, sign)
    raw, its = pi.host_chain(M.spmv, pi.ones(M), max(pi.STEPS), normalize)
    for steps in pi.STEPS:
        assert_bits(its[steps - 1], M.iterate(pi.ones(M), steps, normalize), "peak %d at %d, %d steps" % (n, p, steps))


# ------------------------------------------------------------------------------------------------------------------ the matrices
@pytest.mark.parametrize("name", sorted(ORDINARY))
def test_ordinary_matrices_keep_six_steps_in_range(name):
    M = ORDINARY[name]()
    for x0 in (pi.ones(M), pi.random_x(M)):
        raw, its = pi.host_chain(M.spmv, x0, 6, normalize=False)
        assert all(pi.in_range(v) for v in its), "an un-normalised iterate overflowed or went subnormal"
        assert all(np.abs(v).max() > 0 for v in its)
        assert pi.in_range(M.scale(x0))
    mant = np.frexp(M.val)[0]
    assert (mant * 2.0 ** 20 != np.round(mant * 2.0 ** 20)).mean() > 0.99, "the values are not dyadic"
    assert (M.val > 0).any() and (M.val < 0).any()


def test_shapes_of_the_ordinary_matrices():
    S, L, H = pi.short(), pi.long(), pi.shuffled()
    assert S.n == 1003 and S.terms.min() == 0 and S.terms.max() == 8 and (S.terms == 0).sum() >= 50
    assert S.n % 2 and S.n % 8                                                     # rows % ranks != 0
    assert L.n == 700 and (L.terms == 700).sum() == 3 and np.sort(L.terms)[-4] <= 40 and (L.terms == 0).any()
    for M in (S, L):                                                               # columns strictly ascending in every row
        row = np.repeat(np.arange(M.n), M.terms)
        assert (np.diff(M.col_ind.astype(np.int64))[np.diff(row) == 0] > 0).all()
        assert np.array_equal(M.coo["row"], row) and np.array_equal(M.coo["col"], M.col_ind)
    assert H.n == S.n and H.nnz == S.nnz + 25
    key = H.coo["row"].astype(np.int64) * H.n + H.coo["col"]
    assert len(np.unique(key)) == S.nnz                                            # 25 pairs twice
    assert (np.diff(key) < 0).mean() > 0.4                                          # the storage order is neither by row nor by column
    assert not np.array_equal(H.spmv(pi.ones(H)), S.spmv(pi.ones(S)))              # the repeated entries count


@pytest.mark.parametrize("n,p,sign", PEAKS)
def test_peak_iterates_have_their_largest_magnitude_at_p(n, p, sign):
    M = pi.peak(n, p, sign)
    assert M.n == n and M.terms.min() >= 1 and M.terms.max() <= 3 and M.terms[p] == 1
    assert M.col_ind[M.row_ptr[p]] == p and M.val[M.row_ptr[p]] == 3.0 * sign
    sums = M.scale(pi.ones(M))
    assert np.delete(sums, p).max() <= 1.5
    for normalize in (False, True):
        raw, its = pi.host_chain(M.spmv, pi.ones(M), 3, normalize)
        for k, (r, v) in enumerate(zip(raw, its), 1):
            a = np.abs(r)
            assert a.argmax() == p and (np.delete(a, p) < a[p]).all(), "the raw product's maximum is at p alone"
            assert v[p] == (float(sign) ** k if normalize else (3.0 * sign) ** k)
            if normalize:                                                          # without element p the divisor is too small
                assert_bits(v, M.iterate(pi.ones(M), k, True), "peak")
                assert np.abs(np.delete(r, p)).max() <= 0.5 * a[p]
    if n == pi.PEAK_LARGE[0]:
        assert 900_000 <= M.nnz <= 1_200_000
        assert p // (2048 * 256) == (0 if p == pi.PEAK_LARGE[1][0] else 1)         # which trip of the grid-stride loop reads p


def test_square_zero_is_exactly_zero_from_step_two():
    M = pi.square_zero()
    assert M.n == 300 and M.coo["row"].max() < 150 and M.coo["col"].min() >= 150
    raw, its = pi.host_chain(M.spmv, pi.ones(M), 3, normalize=True)
    assert np.abs(its[0]).max() == 1.0 and (its[0][150:] == 0).all()
    assert (M.val < 0).any()                                                       # products of -0.0 are among what step 2 sums
    for k in (1, 2):
        assert (bits(raw[k]) == 0).all() and (bits(its[k]) == 0).all(), "+0.0 in every element, no NaN from 0 / 0"
        assert_bits(its[k], M.iterate(pi.ones(M), k + 1, True), "square_zero")


def test_small_integers_stay_exact_in_any_order():
    M = pi.small_integers()
    assert set(np.unique(M.val)) == {-2.0, -1.0, 1.0, 2.0} and M.n == 1003
    assert pi.partial_sum_bound(M, pi.ones(M), 5) < 2.0 ** 53
    for k in range(1, 6):
        v = M.iterate(pi.ones(M), k)
        assert (v == np.round(v)).all() and np.abs(v).max() > 0
    T = pi.tiny_integers()
    assert T.n == 5 and T.terms.min() >= 1 and (T.val == np.round(T.val)).all()
    assert np.abs(T.spmv(pi.ones(T))).max() > 0


# ------------------------------------------------------------------------------------------------------------ the start vectors
def test_nan_start_vector_reaches_some_rows_and_not_all():
    M, x = pi.nan_case()
    assert np.isnan(x).sum() == 1
    y = M.spmv(x)
    assert 3 <= np.isnan(y).sum() <= M.n // 2
    v = pi.normalise(y)
    assert np.array_equal(np.isnan(v), np.isnan(y)) and np.nanmax(np.abs(v)) == 1.0
    assert np.isnan(M.spmv(v)).sum() > np.isnan(y).sum()                          # ... and spreads with the second step
    assert_bits(pi.host_chain(M.spmv, x, 2, True)[1][1], M.iterate(x, 2, True), "nan_case")


def test_overflow_start_vector_makes_exactly_one_infinite_row():
    M, x, q = pi.overflow_case()
    y = M.spmv(x)
    assert np.isposinf(y[q]) and np.isfinite(np.delete(y, q)).all() and not np.isnan(y).any()
    assert np.isfinite(np.delete(M.scale(x), q)).all()                            # no other row overflows in any order of summation
    others = np.delete(y, q)
    assert (others > 0).sum() > 50 and (others < 0).sum() > 50
    v = pi.normalise(y)
    assert np.isnan(v[q]) and (np.delete(v, q) == 0).all()
    assert np.array_equal(np.signbit(np.delete(v, q)), np.signbit(others)), "a finite element over Inf keeps its sign"
    assert (M.col_ind == q).any()                                                  # the NaN reaches other rows in step 2
    assert_bits(pi.host_chain(M.spmv, x, 2, True)[1][1], M.iterate(x, 2, True), "overflow_case")


def test_subnormal_start_vector_gives_a_subnormal_maximum():
    M, x = pi.subnormal_case()
    y = M.spmv(x)
    m = np.abs(y).max()
    assert 0.0 < m < pi.TINY and (y == np.round(y / 5e-324) * 5e-324).all()
    assert m <= pi.partial_sum_bound(M, x, 1) < pi.TINY                            # exact in any order
    v = pi.normalise(y)
    assert np.abs(v).max() == 1.0 and len(np.unique(np.abs(v))) > 5
    want = np.round(y / 5e-324) / np.round(m / 5e-324)                             # the same quotients from the integers
    assert_bits(v, want, "subnormal / subnormal is the quotient of the two integers")
    assert_bits(pi.host_chain(M.spmv, x, 2, True)[1][1], M.iterate(x, 2, True), "subnormal_case")
