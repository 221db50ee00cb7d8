"""CPU: what tests/test_gpu_packed_values.py rests on -- the structures and value sets of tests/packed_values.py are what their names
say, the family's constant, plan option and header text exist, and the code layout (smvp::col16_slot order) is a permutation."""
import os

import numpy as np
import pytest

import packed_values as pv
import smvp_toolkit_amd as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_base_structure_is_the_one_the_issue_asks_for():
    rows, cols, rp, ci = pv.base()
    lens = np.diff(rp)
    assert rp[-1] == 6 * pv.TILE + 700 and 1500 <= rows <= 2000 and lens.min() >= 1 and lens.max() <= 40
    assert list(pv.packable_tiles(rp, ci)) == [True] * 6 + [False]
    assert np.all(np.diff(ci.astype(np.int64))[np.diff(np.repeat(np.arange(rows), lens)) == 0] > 0)      # ascending inside a row
    assert ci.min() >= 0 and ci.max() < cols


def test_the_value_sets_are_what_their_names_say():
    rows, cols, rp, ci = pv.base()
    counts = {k: np.concatenate([p for p in pv.escapes_per_wavefront(rp, ci, pv.values(k, rp, ci)) if p is not None]) for k in pv.KINDS}
    assert counts["hot64"].sum() == 0 and counts["few"].sum() == 0
    assert np.all(counts["distinct"] == pv.WAVE)
    half = counts["half"].reshape(6, 4)
    assert half[2, 0] == 0 and half[2, 1] == pv.WAVE and (half % 2 == 1).any() and (half % 2 == 0).any()
    assert pv.escape_share(rp, ci, pv.values("third", rp, ci)) < 0.45 and 0.65 < pv.escape_share(rp, ci, pv.values("distinct", rp, ci))
    assert not np.array_equal(pv.values("half", rp, ci), pv.values("half", rp, ci, seed=6))


def test_the_wide_tile_and_the_giant_row():
    rows, cols, rp, ci = pv.with_wide_tile(*pv.base())
    assert list(pv.packable_tiles(rp, ci)) == [True, True, True, False, True, True, False] and ci.max() < cols
    rows, cols, rp, ci = pv.with_long_and_giant_rows()
    lens = np.diff(rp)
    giant = int(np.argmax(lens))
    assert rp[giant] // pv.TILE == 2 and rp[giant + 1] - 3 * pv.TILE > pv.OVER and np.sum(lens > pv.LONG_ROW) >= 2
    assert np.all(pv.packable_tiles(rp, ci)[:6]) and ci.max() < cols and ci.min() >= 0


def test_hot_table_keys_on_the_bit_pattern():
    v = np.array([0.0] * 5 + [-0.0] * 4 + [np.nan] * 3, dtype=np.float64)
    v[-1] = np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)[0]
    assert len(pv.hot_table(v)) == 4        # +0.0, -0.0 and the two NaNs are four entries


def test_constant_option_and_header():
    assert sm.CSR_KERNEL_STREAM_PACKED == 6
    header = open(os.path.join(ROOT, "include", "smvp_amd.h")).read()
    assert "SMVP_CSR_KERNEL_STREAM_PACKED = 6" in header
    old = sm.get_option("csr_packed")
    for v, back in ((1, 1), (0, 0), (None, -1)):
        with sm.option("csr_packed", v):
            assert sm.get_option("csr_packed") == back
        assert sm.get_option("csr_packed") == old
    with pytest.raises(sm.SmvpError):
        sm.set_option("csr_packed_values", 1)
