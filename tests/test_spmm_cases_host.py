"""The structures of tests/spmm_cases.py reach what they are for, and the assertions the GPU tests call reject the wrong
kernels they are meant to catch: conditions on the inputs and numpy models (spmm_cases.batch_model), all on the host.  The
reference is the one the GPU tests use: the oracle's serial loop on every column (test_gpu_spmm.oracle)."""
import numpy as np
import pytest

import spmm_cases as sc
from test_gpu_spmm import oracle


def ref_of(row_ptr, col_ind, val, X):
    with np.errstate(invalid="ignore", over="ignore"):
        return oracle(row_ptr, col_ind, val, X)


@pytest.fixture(scope="module")
def fuzz():
    """The 25 fuzz cases, generated once and left unchanged."""
    return [sc.block_fuzz(seed) for seed in sc.FUZZ_SEEDS]


def check_csr(rows, cols, row_ptr, col_ind, val):
    """Valid CSR arrays: every index a kernel forms from them is in range."""
    assert row_ptr.dtype == np.int32 and col_ind.dtype == np.int32 and val.dtype == np.float64
    assert len(row_ptr) == rows + 1 and row_ptr[0] == 0 and (np.diff(row_ptr) >= 0).all()
    assert len(col_ind) == len(val) == row_ptr[-1]
    assert len(col_ind) == 0 or (0 <= col_ind.min() and col_ind.max() < cols)
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(row_ptr))
    assert len(np.unique(row_of * cols + col_ind)) == len(col_ind), "a row repeats a column"


# ---------------------------------------------------------------------------------------------------------------- ragged
def test_ragged_has_every_length_and_every_remainder_for_every_group():
    assert sc.RAGGED_STARTS == (0, 9)
    for g in sc.GROUPS:
        seen = set()
        for start in sc.RAGGED_STARTS:
            rows, cols, rp, ci, val, X = sc.ragged(g, start)
            check_csr(rows, cols, rp, ci, val)
            assert rows == 3 * (64 // g) + 1 and cols == 40 and X.shape == (cols, g)
            lens = np.diff(rp)
            assert lens.tolist() == [(r + start) % 18 for r in range(rows)]
            assert all((np.diff(ci[rp[r]:rp[r + 1]]) > 0).all() for r in range(rows)), "columns not sorted"
            seen |= set(lens.tolist())
        assert seen == set(range(18)), "g = %d: lengths %r" % (g, sorted(seen))
        assert {l % sc.BATCH for l in seen} == set(range(sc.BATCH))


# ------------------------------------------------------------------------------------------------------------- slot case
def test_slot_case_poisons_the_re_read_entry_of_every_number_of_unused_slots():
    rows, cols, rp, ci, val, last_col = sc.slot_case()
    check_csr(rows, cols, rp, ci, val)
    assert (rows, cols) == (180, 4000)
    lens = np.diff(rp)
    assert lens.tolist() == [1 + r % 17 for r in range(rows)]
    assert (val >= 0.5).all() and (val < 1.5).all()
    assert last_col.tolist() == [int(ci[rp[r + 1] - 1]) for r in range(rows)]
    assert {int(l) % sc.BATCH for l in lens[::3]} == set(range(sc.BATCH))
    for k in (1, 2, 4, 8, 16):
        X = sc.slot_operand(k, last_col)
        assert X.shape == (cols, k) and (X[np.isfinite(X)] >= 0.5).all() and (X[np.isfinite(X)] < 1.0).all()
        assert set(np.flatnonzero(~np.isfinite(X[:, k - 1])).tolist()) == set(last_col[::3].tolist()) and np.isfinite(X[:, :k - 1]).all()
        ref = ref_of(rp, ci, val, X)
        assert not np.isnan(ref).any() and (ref[::3, k - 1] == np.inf).all() and np.isfinite(ref[:, :k - 1]).all()
        sc.assert_slot_rows(ref, "the oracle, k = %d" % k)


# ------------------------------------------------------------------------------------------------------------ row counts
def test_row_counts_sit_on_the_launch_edges_of_every_group():
    counts = set(sc.ROW_COUNTS)
    assert sc.ROW_COUNTS == tuple(sorted(counts))
    for g in sc.GROUPS:
        per_wg = sc.WORKGROUP // g
        assert {per_wg - 1, per_wg, per_wg + 1} <= counts, g
        if 8 * per_wg < 12289:
            assert {8 * per_wg - 1, 8 * per_wg, 8 * per_wg + 1} <= counts, g
    for block in (sc.BLOCK_ROWS, 2 * sc.BLOCK_ROWS):
        assert {block - 1, block, block + 1} <= counts
    assert max(counts) > 3 * sc.BLOCK_ROWS and max(counts) % sc.BLOCK_ROWS
    assert set(sc.ROW_COUNT_KS) == {1, 2, 3, 4, 8, 16} and {sc.first_pass_group(k) for k in sc.ROW_COUNT_KS} == set(sc.GROUPS)


@pytest.mark.parametrize("rows", sc.ROW_COUNTS)
def test_row_count_case_is_what_it_says(rows):
    n, cols, rp, ci, val, X = sc.row_count_case(rows)
    check_csr(n, cols, rp, ci, val)
    assert n == rows and cols == 97 and X.shape == (cols, 16)
    lens = np.diff(rp)
    assert lens[:-1].tolist() == [(7 * r) % 11 for r in range(rows - 1)]
    assert lens[-1] == max((7 * (rows - 1)) % 11, 1) >= 1
    for r in {0, rows // 2, rows - 1}:
        assert ci[rp[r]:rp[r + 1]].tolist() == [(r + 13 * j) % 97 for j in range(int(lens[r]))]
    if rows >= 11:
        assert set(lens.tolist()) == set(range(11))
    assert (val != 0).all()


# ------------------------------------------------------------------------------------------------------------------ fuzz
def test_block_fuzz_crosses_sorted_blocks_with_every_group(fuzz):
    assert len(fuzz) == 25
    rows_of = [c[0] for c in fuzz]
    ks = [c[5] for c in fuzz]
    assert sum(r > sc.BLOCK_ROWS for r in rows_of) >= 8 and sum(r > 2 * sc.BLOCK_ROWS for r in rows_of) >= 3
    assert max(rows_of) <= sc.FUZZ_MAX_ROWS
    assert sum(k > 16 for k in ks) >= 5 and all(1 <= k <= 40 for k in ks)
    groups = [sc.first_pass_group(k) for k in ks]
    for g in sc.GROUPS:
        assert groups.count(g) >= 2, "first-pass G = %d occurs %d times" % (g, groups.count(g))
    assert sum(c[2][1] == 0 for c in fuzz) >= 3, "empty first rows"
    assert sum(c[2][-1] == c[2][-2] for c in fuzz) >= 3, "empty last rows"
    styles = set()
    for seed, (rows, cols, rp, ci, val, k, ldx, ldy, X) in zip(sc.FUZZ_SEEDS, fuzz):
        check_csr(rows, cols, rp, ci, val)
        assert int(rp[-1]) <= sc.FUZZ_MAX_ENTRIES, "seed %d: %d entries" % (seed, rp[-1])
        assert 0 <= ldx - k <= 8 and 0 <= ldy - k <= 8 and X.shape == (cols, k) and np.isfinite(X).all()
        styles.add(seed % 5)
    assert styles == set(range(5))
    assert sum(ldx > k for _, _, _, _, _, k, ldx, _, _ in fuzz) >= 5 and sum(ldy > k for _, _, _, _, _, k, _, ldy, _ in fuzz) >= 5
    mags = np.concatenate([np.abs(c[4][c[4] != 0]) for c in fuzz])
    assert np.log10(mags.max() / mags.min()) > 10, "values over several decades"
    again = sc.block_fuzz(7)
    assert all(np.array_equal(a, b) for a, b in zip(again, fuzz[7])), "not reproducible"


# ------------------------------------------------------------------------------------------------------------- the model
MODEL_FUZZ_SEEDS = (0, 3, 6)


def model_cases(fuzz):
    for g in sc.GROUPS:
        for start in sc.RAGGED_STARTS:
            rows, cols, rp, ci, val, X = sc.ragged(g, start)
            yield "ragged(%d, %d)" % (g, start), rp, ci, val, X
    rows, cols, rp, ci, val, last_col = sc.slot_case()
    yield "slot_case", rp, ci, val, sc.slot_operand(4, last_col)
    rows, cols, rp, ci, val, X = sc.row_count_case(4097)
    yield "row_count_case(4097)", rp, ci, val, X
    for seed in MODEL_FUZZ_SEEDS:
        rows, cols, rp, ci, val, k, ldx, ldy, X = fuzz[seed]
        yield "fuzz %d" % seed, rp, ci, val, X


def test_batch_model_without_a_fault_gives_the_oracles_bits(fuzz):
    n = 0
    for what, rp, ci, val, X in model_cases(fuzz):
        sc.assert_bits(sc.batch_model(rp, ci, val, X), ref_of(rp, ci, val, X), what)
        n += 1
    assert n == 2 * len(sc.GROUPS) + 2 + len(MODEL_FUZZ_SEEDS)
    assert any(fuzz[s][0] > sc.BLOCK_ROWS for s in MODEL_FUZZ_SEEDS), "no model case crosses a sorted block"


def test_zero_mask_leaves_a_nan_on_the_slot_case():
    rows, cols, rp, ci, val, last_col = sc.slot_case()
    for k in (1, 2, 4, 8, 16):
        X = sc.slot_operand(k, last_col)
        sc.assert_slot_rows(sc.batch_model(rp, ci, val, X), "the model, k = %d" % k)
        Y = sc.batch_model(rp, ci, val, X, "zero_mask")
        assert np.isnan(Y).any()
        with pytest.raises(AssertionError, match="NaN"):
            sc.assert_slot_rows(Y, "zero_mask")
        with pytest.raises(AssertionError):
            sc.assert_bits(Y, ref_of(rp, ci, val, X), "zero_mask")
        # every poisoned row with unused slots in its last batch, and only the poisoned vector
        partial = np.diff(rp)[::3] % sc.BATCH != 0
        assert np.isnan(Y[::3, k - 1][partial]).all() and (Y[::3, k - 1][~partial] == np.inf).all() and not np.isnan(Y[:, :k - 1]).any()


@pytest.mark.parametrize("fault", ("drop_tail", "next_entry"))
@pytest.mark.parametrize("g", sc.GROUPS)
def test_a_wrong_last_batch_differs_from_the_oracle_on_ragged(g, fault):
    for start in sc.RAGGED_STARTS:
        rows, cols, rp, ci, val, X = sc.ragged(g, start)
        with pytest.raises(AssertionError, match="differ"):
            sc.assert_bits(sc.batch_model(rp, ci, val, X, fault), ref_of(rp, ci, val, X), "%s on ragged(%d, %d)" % (fault, g, start))


@pytest.mark.parametrize("rows", (4097, 8193, 12289))
def test_a_lost_last_block_leaves_nan_on_the_row_counts(rows):
    n, cols, rp, ci, val, X = sc.row_count_case(rows)
    ref = ref_of(rp, ci, val, X)
    assert np.isfinite(ref).all()
    Y = sc.batch_model(rp, ci, val, X, "lost_block")
    assert np.isnan(Y[rows // sc.BLOCK_ROWS * sc.BLOCK_ROWS:]).all() and np.isfinite(Y[:rows // sc.BLOCK_ROWS * sc.BLOCK_ROWS]).all()
    with pytest.raises(AssertionError, match="differ"):
        sc.assert_bits(Y, ref, "lost_block at %d rows" % rows)
    # one written row fewer is enough: the last row always holds an entry, so NaN there is never the product
    Y = sc.batch_model(rp, ci, val, X)
    Y[-1] = np.nan
    with pytest.raises(AssertionError, match="row %d" % (rows - 1)):
        sc.assert_bits(Y, ref, "last row unwritten")
