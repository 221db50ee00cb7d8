"""The GPU parity tests' own checks (tests/parity.py), on the host: check_y must catch what a wrong kernel leaves behind and
pass every correctly rounded order of summation; the guards must catch a write next to y; the matrices of the binned
plan's spill tests must still reach their regimes under the plan's constants."""
import math

import numpy as np
import pytest

import oracle_binding as ob
import parity
from parity import U, check_y


def _rows(rng, lens, cancel=False):
    """Random rows of products (10^+-8 spread) for the given lengths; with `cancel`, every row's sum cancels to ~1e-15 of its
    terms (the row is the products and their negations, plus a tiny remainder)."""
    out = []
    for n in lens:
        p = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        if cancel and n >= 3:
            h = n // 2
            p[h:2 * h] = -p[:h]
            p[-1] = 1e-15 * np.abs(p[:-1]).sum() if n % 2 else p[-1]
            rng.shuffle(p)
        out.append(p)
    return out


def _serial(p):
    acc = 0.0
    for v in p:
        acc += v
    return acc


def _pairwise(p):
    if len(p) <= 2:
        return _serial(p)
    h = len(p) // 2
    return _pairwise(p[:h]) + _pairwise(p[h:])


def _blocked(p, b=64):
    acc = 0.0
    for i in range(0, len(p), b):
        acc += _serial(p[i:i + b])
    return acc


ORDERS = {"serial": _serial, "reversed": lambda p: _serial(p[::-1]), "pairwise": _pairwise, "blocked": _blocked,
          "fsum": math.fsum}


def _case(seed, cancel):
    rng = np.random.default_rng(seed)
    lens = [1, 2, 3, 7, 31, 33, 64, 1000, 4097, 40_000] + rng.integers(1, 300, 40).tolist()
    rows = _rows(rng, lens, cancel)
    ref = np.array([_serial(p) for p in rows])
    scale = np.array([_serial(np.abs(p)) for p in rows])
    return rows, np.array(lens), ref, scale


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("cancel", [False, True])
def test_check_y_passes_every_summation_order(order, cancel):
    rows, terms, ref, scale = _case(5 + cancel, cancel)
    y = np.array([ORDERS[order](p) for p in rows])
    check_y(y, ref, scale, terms)
    if cancel:      # the rows do cancel: the error allowed is far above |y| there
        assert np.median(np.abs(ref[terms >= 3]) / scale[terms >= 3]) < 1e-12


def test_check_y_through_the_oracle_with_a_shuffled_row():
    """The oracle's serial loop against fsum of the same products, with x spread over 10^+-3 (what the fuzz tests do)."""
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 60, 2000)
    lens[:3] = (0, 40_000, 1)
    cols = 50_000
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col_ind = rng.integers(0, cols, int(row_ptr[-1])).astype(np.int32)
    val = rng.uniform(-1, 1, len(col_ind)) * 10.0 ** rng.integers(-8, 8, len(col_ind))
    x = rng.standard_normal(cols) * 10.0 ** rng.integers(-3, 3, cols)
    ref = ob.csr_spmv(row_ptr, col_ind, val, x)
    scale = ob.csr_spmv(row_ptr, col_ind, np.abs(val), np.abs(x))
    prod = val * x[col_ind]
    y = np.array([math.fsum(rng.permutation(prod[a:b])) for a, b in zip(row_ptr[:-1], row_ptr[1:])])
    check_y(y, ref, scale, np.diff(row_ptr))
    assert y[0] == 0.0 and ref[0] == 0.0


def test_check_y_fails_on_a_nan_row():
    rows, terms, ref, scale = _case(1, False)
    y = ref.copy()
    y[17] = np.nan
    with pytest.raises(AssertionError, match="1 rows beyond.*first bad row 17"):
        check_y(y, ref, scale, terms)


def test_check_y_fails_on_an_empty_row_left_nan():
    ref, scale, terms = np.array([1.5, 0.0, -2.0]), np.array([1.5, 0.0, 2.0]), np.array([1, 0, 1])
    check_y(np.array([1.5, 0.0, -2.0]), ref, scale, terms)
    with pytest.raises(AssertionError, match="first bad row 1"):
        check_y(np.array([1.5, np.nan, -2.0]), ref, scale, terms)
    with pytest.raises(AssertionError):
        check_y(np.array([1.5, 1e-300, -2.0]), ref, scale, terms)      # an empty row is exactly what the oracle has


def test_check_y_passes_signed_zeros_on_empty_rows():
    ref, scale, terms = np.zeros(4), np.zeros(4), np.zeros(4)
    check_y(np.array([0.0, -0.0, 0.0, -0.0]), ref, scale, terms)
    check_y(np.array([-0.0, 0.0, -0.0, 0.0]), -ref, scale, terms)


@pytest.mark.parametrize("n", [1, 7, 40, 1000, 40_000])
def test_check_y_fails_just_past_the_tight_bound(n):
    """An error of 3 (n + 2) 2^-53 sum|a x| is 1.5 times what is allowed; 1.9 (n + 2) 2^-53 sum|a x| passes."""
    ref, scale = np.array([0.25, 3.0]), np.array([1.0, 5.0])
    terms = np.array([n, n])
    for k in (0, 1):
        y = ref.copy()
        y[k] += 1.9 * (n + 2) * U * scale[k]
        check_y(y, ref, scale, terms)
        y[k] = ref[k] - 3.0 * (n + 2) * U * scale[k]
        with pytest.raises(AssertionError, match="worst \\|y - ref\\| / bound 1\\.[45]"):   # (the error itself is rounded)
            check_y(y, ref, scale, terms)


def test_check_y_fails_on_a_dropped_entry():
    """One product left out of a row of 1000 (terms 10^+-8): caught once it exceeds the bound, although it is far below
    the old 1e-9 of the row's sum of terms."""
    rng = np.random.default_rng(3)
    p = rng.standard_normal(1000) * 10.0 ** rng.integers(-8, 8, 1000)
    scale, ref = np.abs(p).sum(), math.fsum(p)
    small = np.argsort(np.abs(p))
    i = next(int(j) for j in small if np.abs(p[j]) > 10 * parity.bound(1000) * scale)
    assert np.abs(p[i]) < parity.TOL * scale                 # invisible to the old check
    y = math.fsum(np.delete(p, i))
    with pytest.raises(AssertionError, match="1 rows beyond"):
        check_y(np.array([y]), np.array([ref]), np.array([scale]), np.array([1000]))


def test_check_y_bound_is_never_looser_than_tol():
    assert parity.bound(10 ** 9) == parity.TOL
    assert parity.bound(7) == pytest.approx(18 * U)
    ref, scale = np.array([1.0]), np.array([1.0])
    with pytest.raises(AssertionError):
        check_y(ref + 2e-9, ref, scale, 10 ** 9)


def test_check_y_exact_and_shape():
    check_y(np.array([1.0, 2.0]), np.array([1.0, 2.0]), 0, 0, exact=True)
    with pytest.raises(AssertionError):
        check_y(np.array([1.0, np.nextafter(2.0, 3.0)]), np.array([1.0, 2.0]), 0, 0, exact=True)
    with pytest.raises(AssertionError, match="shape"):
        check_y(np.zeros(3), np.zeros(4), 0, 0)


def test_check_y_non_finite_references():
    ref = np.array([np.inf, np.nan, 1.0])
    check_y(np.array([np.inf, np.nan, 1.0]), ref, np.array([np.inf, np.inf, 1.0]), 2)
    with pytest.raises(AssertionError):
        check_y(np.array([-np.inf, np.nan, 1.0]), ref, np.array([np.inf, np.inf, 1.0]), 2)


@pytest.mark.parametrize("rows", [1, 5, 1000])
def test_guards_catch_writes_next_to_y(rows):
    torch = pytest.importorskip("torch")
    buf, y = parity.guarded_y(torch, rows, device="cpu")
    assert y.data_ptr() - buf.data_ptr() == 8 * parity.G and bool(y.isnan().all())
    y.fill_(1.0)
    parity.check_guards(buf, rows)
    buf[parity.G + rows] = 0.0                                   # one element just past the end
    with pytest.raises(AssertionError, match="past its last row"):
        parity.check_guards(buf, rows)
    buf, y = parity.guarded_y(torch, rows, device="cpu")
    buf[parity.G - 1] = 0.0                                      # one just before the start
    with pytest.raises(AssertionError, match="in front of row 0"):
        parity.check_guards(buf, rows)
    buf, y = parity.guarded_y(torch, rows, device="cpu")
    buf.view(torch.int64)[parity.G + rows + 3] ^= 1              # one bit of a NaN-free guard
    with pytest.raises(AssertionError):
        parity.check_guards(buf.numpy(), rows)


@pytest.mark.parametrize("kind", parity.SPILL_KINDS)
def test_spill_matrices_reach_their_regimes(kind):
    """The matrices of the binned spill tests (test_gpu_parity.py) against the plan's constants, on the host."""
    rows, cols, band, row_ptr, col_ind, val = parity.spill_matrix(kind)
    assert len(row_ptr) == rows + 1 and len(col_ind) == len(val) == row_ptr[-1] and 0 <= col_ind.min() and col_ind.max() < cols
    g = parity.assert_spill_regime(kind, rows, cols, band, row_ptr, col_ind)
    assert g["cells"] <= g["nrb"] and g["runs"] <= g["ncb"]
    if kind == "cells":
        assert g["ncb"] == 64 and g["q"] == 1
    if kind == "runs":
        assert g["ncb"] == 1221 and g["q"] == 20


def test_binned_regime_on_a_small_matrix():
    """binned_regime by hand: 3 rows, band 2 -- row 0 has two far entries in column blocks 0 and 1, row 2 one far entry."""
    row_ptr = np.array([0, 3, 4, 6], np.int32)
    col_ind = np.array([0, 5, 20000, 1, 2, 40000], np.int32)
    g = parity.binned_regime(row_ptr, col_ind, 40001, band=2)
    assert (g["nf"], g["ncb"], g["q"], g["nrb"]) == (3, 3, 1, 1)
    assert (g["cells"], g["runs"], g["span"], g["long_rows"], g["capped_rows"]) == (1, 3, 2, 0, 0)
    none = parity.binned_regime(row_ptr, col_ind, 40001, band=50000)
    assert none["nf"] == 0 and none["runs"] == 0
