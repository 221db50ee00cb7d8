"""tests/timed_runs.py on the host: the structures meet the regimes they are named after, the Python mirror of the launch
arithmetic is the library's, the exact reference is the oracle's and rejects the wrong products it is there to catch.  CPU only."""
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import timed_runs as tr
from special_values import check_bits
from test_tile_map import compile_check


@pytest.mark.parametrize("tile", tr.TILES)
@pytest.mark.parametrize("name", sorted(tr.NAMED))
def test_named_structures_meet_their_regime(name, tile):
    rows, cols, row_ptr, col_ind = tr.structure(name, tile)
    nnz = int(row_ptr[-1])
    tiles, grid, shards = tr.NAMED[name]
    for fmt in ("csr", "tjds"):
        g = tr.regime(nnz, tile, fmt)
        assert (g["ntiles"], g["grid"], g["shards"]) == (tiles, grid, shards), (fmt, g)
        assert sum(g["members"]) == grid and len(g["members"]) == shards
    assert nnz <= 1_450_000 and cols <= 60000
    if name == "t641":
        assert g["members"] == [45] * 16
    if name == "t705":
        assert g["members"] == [50] * 8 + [49] * 8           # shards with unequal numbers of members
    if name == "t1":
        assert g["members"] == [8] and nnz == tile           # 7 of the 8 workgroups own no tile
    # the shape of the rows
    lens = np.diff(row_ptr)
    assert len(lens) == rows and lens[0] == 0 and lens[1] == 0 and np.all(lens[-3:] == 0) and lens[-4] > 0
    assert set(tr.LENGTH_MIX) <= set(lens.tolist())
    if nnz >= tr.LONG_ROW + 2 * sum(tr.LENGTH_MIX):
        (r,) = np.flatnonzero(lens == tr.LONG_ROW)
        assert row_ptr[r] // tile != (row_ptr[r + 1] - 1) // tile and row_ptr[r] % 256 != 0     # it crosses a tile edge
    assert nnz % tile != 0 or name == "t1"
    # columns ascending and distinct inside every row, inside [0, cols)
    assert col_ind.min() >= 0 and col_ind.max() < cols
    inner = np.ones(nnz, dtype=bool)
    inner[row_ptr[:-1][lens > 0]] = False
    assert np.all(np.diff(col_ind.astype(np.int64), prepend=-1)[inner] > 0)


def test_tjds_structures_are_sized_for_the_tile_the_plan_picks():
    """A TJDS run cannot name its tile: the structures the GPU tests give it must meet their regime at the plan's own choice."""
    for name, tile in (("t1", 256), ("t25", 256), ("t640", 256), ("t640", 1024)):
        nnz = int(tr.structure(name, tile)[2][-1])
        assert tr.default_tile(nnz, "tjds") == tile and tr.default_tile(nnz, "csr") == tile
        assert tr.regime(nnz, tile, "tjds")["ntiles"] == tr.NAMED[name][0]


def test_launch_arithmetic_mirrors_the_library(tmp_path):
    """tile_group_of / tile_grid_of against csrc/smvp_tile_map.h itself (compiled by the host compiler, as test_tile_map.py does)
    for every tile count from 1 to 5000, CSR's group and TJDS's."""
    exe = str(tmp_path / "tile_map_check")
    p = compile_check(exe, False)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe, "grids"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    table = np.array([line.split() for line in r.stdout.splitlines()], dtype=np.int64)
    assert table.shape == (5000, 5) and np.array_equal(table[:, 0], np.arange(1, 5001))
    for ntiles, g_csr, grid_csr, g_tjds, grid_tjds in table.tolist():
        for fmt, g, grid in (("csr", g_csr, grid_csr), ("tjds", g_tjds, grid_tjds)):
            got = tr.tile_group_of(ntiles, tr.WANTED_GROUP[fmt])
            assert (got, tr.tile_grid_of(ntiles, got)) == (g, grid), (ntiles, fmt)
    # the edges of the shard rule, as the launcher writes it: grid <= 24 ? 1 : grid <= 640 ? 8 : 16
    assert [tr.shards_of(g) for g in (8, 24, 32, 640, 648, 720, 4096)] == [1, 1, 8, 8, 16, 16, 16]


@pytest.mark.parametrize("name,tile", [("t1", 256), ("t25", 256), ("t25", 2048), ("t705", 256)])
def test_exact_reference_has_the_oracles_bits(name, tile):
    rows, cols, row_ptr, col_ind = tr.structure(name, tile)
    val, x = tr.exact_operands(int(row_ptr[-1]), cols)
    ref = tr.exact_reference(row_ptr, col_ind, val, x)
    check_bits(ref, ob.csr_spmv(row_ptr, col_ind, val, x), "int64 reference against the oracle's serial loop")
    check_bits(tr.exact_reference(row_ptr, col_ind, val, np.ones(cols)), ob.csr_spmv(row_ptr, col_ind, val, np.ones(cols)), "x = ones")
    lens = np.diff(row_ptr)
    assert np.all(ref.view(np.int64)[lens == 0] == 0), "+0.0 for empty rows"
    assert (ref[lens > 0] == 0).any() and (ref[lens > 0] != 0).mean() > 0.5, "rows that cancel, and mostly rows that do not"


def test_exact_reference_rejects_wrong_products():
    tile = 256
    rows, cols, row_ptr, col_ind = tr.structure("t25", tile)
    val, x = tr.exact_operands(int(row_ptr[-1]), cols)
    ref = tr.exact_reference(row_ptr, col_ind, val, x)
    lens = np.diff(row_ptr)
    # (1) the last row that starts in a tile is dropped (left at +0.0)
    first_tile = row_ptr[:-1] // tile
    last_of_tile = np.flatnonzero((lens > 0) & (np.append(first_tile[1:], -1) != first_tile) & (ref != 0))
    assert len(last_of_tile) >= 5
    y = ref.copy()
    y[last_of_tile[2]] = 0.0
    with pytest.raises(AssertionError):
        check_bits(y, ref, "dropped row")
    # (2) a row is left at the NaN the entry points poison y with
    y = ref.copy()
    y[np.flatnonzero(lens > 0)[7]] = np.frombuffer(b"\xff" * 8, dtype=np.float64)[0]
    with pytest.raises(AssertionError):
        check_bits(y, ref, "poisoned row")
    # (3) -0.0 for an empty row
    y = ref.copy()
    y[0] = -0.0
    assert y[0] == ref[0]                    # equal as numbers ...
    with pytest.raises(AssertionError):
        check_bits(y, ref, "negative zero")   # ... but not the reference's bits
    check_bits(ref.copy(), ref, "the reference itself")


def test_edge_structures_and_the_pinned_outcomes():
    for name in tr.EDGES:
        rows, cols, row_ptr, col_ind, val, x = tr.edge(name)
        assert len(row_ptr) == rows + 1 and len(x) == cols and len(val) == row_ptr[-1]
    assert tr.edge("no_rows")[0] == 0 and tr.edge("empty_matrix")[2][-1] == 0
    refused = {(n, p) for n in tr.EDGES for p in ("csr_auto", "csr_stream", "tjds") if tr.device_timing_is_refused(n, p)}
    assert refused == {("no_rows", "csr_auto"), ("no_rows", "csr_stream"), ("no_rows", "tjds"), ("one_row_of_16385", "csr_auto")}


def test_check_times_rejects_what_it_is_there_for():
    import smvp_toolkit_amd as sm

    class Info:
        timing, wall_ms, device_clock_khz, repeat_launches = sm.TIMING_DEVICE, 1.0, 100000.0, 1

    ms = np.array([317, 290, 305, 1], dtype=np.float64) / 100000.0
    tr.check_times(ms, sm.time_stats(ms), Info, 4)
    for bad in (ms[:3], ms * 1.0001, np.where(np.arange(4) == 3, 0.0, ms), np.where(np.arange(4) == 1, np.inf, ms),
                np.where(np.arange(4) == 1, 2.0, ms), ms * 1000):      # a time missing, no whole ticks, 0, inf, > wall, sum > wall
        with pytest.raises(AssertionError):
            tr.check_times(bad, sm.time_stats(bad), Info, 4)
    st = sm.time_stats(ms)
    st.time_stdev *= 1.001
    with pytest.raises(AssertionError):
        tr.check_times(ms, st, Info, 4)
