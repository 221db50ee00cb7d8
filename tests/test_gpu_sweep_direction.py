"""The tile kernel sweeps its tiles forward and backward in turn (plan option "csr_sweep_alternate"): the products must not
notice.

A handle on the tile kernel (csr_stream_owner: CSR STREAM, the TJDS one-kernel product) flips the direction of its sweep with
every plain launch, so that a product starts on what the one before it left in the Infinity Cache.  Backward, workgroup b of
the padded grid takes the tile that workgroup grid - 1 - b takes forward (csrc/smvp_tile_map.h; tests/test_tile_map.py checks
the map itself on the host).  By default a plan alternates only where one product's bytes exceed the Infinity Cache -- far more
than a test matrix holds -- so the option is set to 1 here (alternate whatever the size).  Four consecutive products on one
handle -- both directions at least twice -- each into a freshly NaN-poisoned guarded buffer; a tile never visited leaves NaN in
its rows, a write outside y breaks a guard, and all four must be the exact int64 reference bit for bit (integer operands: every
sum is exact in any order, tests/adopted.py).  The same with the option at 0 and at its default, and across a re-plan between
two products.

Matrices: tile counts 1, 7, 8, 9, 63, 64, 65, 129, 513, 4095, 4096, 4097 and 4609 -- the edges of the launcher's group
(tile_group: 1 below 128 tiles, tiles / 64 up to 64) and of the grid's padding to 8 * group -- with a last partial tile, rows
that cross tile ends, a row of 700 entries finished through the overflow area, a giant row (more than 1024 entries past its
tile's end), and rows without entries at the start, in the middle and at the end.
"""
import contextlib
import functools

import numpy as np
import pytest

import smvp_toolkit_amd as sm
from adopted import coo, int_values, reference
from parity import check_guards, guarded_y
from test_gpu_parity import TJDS_GATHER_VARIANTS, tjds_gather_matrix

pytestmark = pytest.mark.gpu

OPTION = "csr_sweep_alternate"
TILE_COUNTS = (1, 7, 8, 9, 63, 64, 65, 129, 513, 4095, 4096, 4097, 4609)
TILES = (256, 1024, 2048)
OVER = 1024                             # kStreamOver: entries past its end a tile finishes its last row with
EMPTY_FRONT, EMPTY_BACK = 3, 4


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()                        # (a copy: the fixtures are read-only)


# ------------------------------------------------------------------------------------------------------------- the matrices
def row_lengths(ntiles, tile, seed):
    """Row lengths that add up to (ntiles - 1) * tile + tile // 2 + 3 entries: a last partial tile.  Lengths 0 ... 24 (a third
    of the rows empty or short, so rows without entries lie everywhere and most tile ends fall inside a row); from 7 tiles on
    one giant row of tile + OVER + 300 entries that starts in the middle of a tile and, where the entries allow it (12 tiles of
    256, 7 of the larger ones), one row of 700 entries (it ends in its tile's overflow area or in the tile); EMPTY_FRONT /
    EMPTY_BACK rows without entries in front and at the back."""
    rng = np.random.default_rng(seed)
    nnz = (ntiles - 1) * tile + tile // 2 + 3
    n = nnz // 6 + 64
    lens = rng.integers(0, 25, n)
    lens[rng.random(n) < 0.3] //= 8
    special, giant = {}, tile + OVER + 300
    if nnz >= giant + 64:
        special[5] = giant
    if nnz >= giant + 700 + 2 * tile:
        special[11] = 700
    for r, length in special.items():
        lens[r] = length
    keep = int(np.searchsorted(np.cumsum(lens), nnz, side="left")) + 1  # the first rows that hold nnz entries or more
    assert keep <= n and (not special or max(special) < keep - 1)
    lens = lens[:keep]
    lens[-1] -= lens.sum() - nnz
    assert lens[-1] >= 0 and lens.sum() == nnz
    return np.concatenate([np.zeros(EMPTY_FRONT, dtype=np.int64), lens, np.zeros(EMPTY_BACK, dtype=np.int64)]), special


@functools.lru_cache(maxsize=2)
def matrix(ntiles, tile):
    """(rows, cols, row_ptr, col_ind, val, x, the exact y): ntiles tiles of `tile` entries; entry j of row r lies in column
    r + 2 j + (r & 1), so a tile's columns span far fewer than 65536 (the 16-bit column offsets are taken where asked for)."""
    lens, special = row_lengths(ntiles, tile, 1000 * ntiles + tile)
    rows = len(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(row_ptr[-1])
    assert -(-nnz // tile) == ntiles and nnz % tile != 0
    row = np.repeat(np.arange(rows, dtype=np.int64), lens)
    j = np.arange(nnz, dtype=np.int64) - row_ptr[row]
    col_ind = (row + 2 * j + (row & 1)).astype(np.int32)
    cols = rows + 2 * int(lens.max()) + 2
    # what the matrix must hold: empty rows in front, at the back and in the middle, rows that cross tile ends, the two long rows
    assert lens[0] == 0 and lens[-1] == 0 and (lens[EMPTY_FRONT:-EMPTY_BACK] == 0).any()
    first, last = row_ptr[:-1][lens > 0], row_ptr[1:][lens > 0] - 1
    crossing = first // tile != last // tile
    assert ntiles == 1 or crossing.any() and (ntiles < 63 or crossing.sum() >= ntiles // 2)
    assert bool(special) == (ntiles >= 7), "every matrix of 7 tiles or more holds the giant row"
    if special:
        giant = EMPTY_FRONT + 5
        past = int(row_ptr[giant + 1]) - (int(row_ptr[giant]) // tile + 1) * tile
        assert past > OVER and int(row_ptr[giant]) % tile != 0, "the giant row reaches more than kStreamOver past its tile's end"
    rng = np.random.default_rng(ntiles + 7)
    val, x = int_values(rng, nnz, 1, 8), int_values(rng, cols, 1, 8)
    out = (rows, cols, row_ptr, col_ind, val, x, reference(row_ptr, col_ind, val, x))
    for a in out[2:]:
        a.setflags(write=False)
    return out


# --------------------------------------------------------------------------------------------------------------- the checks
@contextlib.contextmanager
def options(opts):
    with contextlib.ExitStack() as stack:
        for name, value in opts.items():
            stack.enter_context(sm.option(name, value))
        yield


def products_are_the_reference(torch, product, rows, want, label, n=4):
    """n consecutive products, each into a freshly poisoned guarded y: the guards whole, every row the reference's bits."""
    first = None
    for i in range(n):
        buf, dy = guarded_y(torch, rows)
        product(dy)
        torch.cuda.synchronize()
        check_guards(buf, rows)
        got = dy.cpu().numpy()
        bad = np.flatnonzero(got.view(np.int64) != want.view(np.int64))
        assert not len(bad), "%s, product %d: %d rows differ from the exact sums (%d of them NaN: never written); first row %d: %r against %r" % (
            label, i, len(bad), np.isnan(got[bad]).sum(), bad[0], got[bad[0]], want[bad[0]])
        first = got if first is None else first
        assert np.array_equal(got.view(np.int64), first.view(np.int64)), "%s: product %d differs from product 0" % (label, i)


def state(A):
    return A.describe(), A.plan_info()["plan_bytes"], A.plan_info()["matrix_bytes"]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("ntiles", TILE_COUNTS)
def test_stream_sweeps_both_ways(torch, ntiles, tile):
    """STREAM at this tile size under csr_col16 1 | 0 and csr_rowrel default | 0, the option at 1 and at 0 (and at its default under the default
    plan options)."""
    rows, cols, row_ptr, col_ind, val, x, want = matrix(ntiles, tile)
    dx = dev(torch, x)
    arrays = dev(torch, row_ptr), dev(torch, col_ind), dev(torch, val)
    states = {}
    for col16 in (1, 0):
        for rowrel in (None, 0):
            for alternate in (1, 0, None) if (col16, rowrel) == (1, None) else (1, 0):
                label = "%d tiles of %d, csr_col16 %r, csr_rowrel %r, %s %r" % (ntiles, tile, col16, rowrel, OPTION, alternate)
                opts = {"csr_col16": col16, "csr_rowrel": rowrel, OPTION: alternate}
                with options(opts):
                    A = sm.CsrMatrix(rows, cols, *arrays)
                    A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
                try:
                    name = A.describe()[0]
                    assert name == "csr_stream_owner<%d, %d, false>" % (tile // 256, 5 if col16 and tile >= 1024 else 0), label
                    assert A.launches() == 1
                    # describe(), plan_info() and launches() do not know the option
                    states.setdefault((col16, rowrel), state(A))
                    assert state(A) == states[(col16, rowrel)], label
                    products_are_the_reference(torch, lambda dy: A.spmv(dx, dy), rows, want, label)
                    # a re-plan between two products (the direction starts over): the next two are right
                    products_are_the_reference(torch, lambda dy: A.spmv(dx, dy), rows, want, label + ", one product", n=1)
                    with options(opts):
                        A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
                    products_are_the_reference(torch, lambda dy: A.spmv(dx, dy), rows, want, label + ", after a re-plan", n=2)
                finally:
                    A.close()


TJDS_CASES = [("default", 0)] + TJDS_GATHER_VARIANTS


@functools.lru_cache(maxsize=1)
def tjds_arrays(ntiles):
    rows, cols, row_ptr, col_ind, val, x, want = matrix(ntiles, 256)
    return sm.tjds_from_coo(coo(row_ptr, col_ind, val), rows, cols)


@pytest.mark.parametrize("ntiles", TILE_COUNTS)
def test_tjds_sweeps_both_ways(torch, ntiles):
    """The TJDS default mode and every stream form / tile size of the one-kernel product on the 256-entry-tile matrices (up to
    1.2 M entries; the forms with larger tiles then run a quarter and an eighth as many tiles, the TJDS group is up to 32)."""
    rows, cols, row_ptr, col_ind, val, x, want = matrix(ntiles, 256)
    t = tjds_arrays(ntiles)
    dx = dev(torch, x)
    for index, tile in TJDS_CASES:
        states = []
        for alternate in (1, 0, None):
            label = "TJDS %s tile %d on %d tiles of 256, %s %r" % (index, tile, ntiles, OPTION, alternate)
            with sm.option(OPTION, alternate):
                T = sm.TjdsMatrix(t) if index == "default" else tjds_gather_matrix(t, index, tile)
            try:
                T.set_x(dx)
                states.append(state(T))
                assert states[-1] == states[0], label

                def product(dy):
                    T.zero_y(dy)
                    T.spmv(dy)

                assert T.describe()[0].startswith("csr_stream_owner<"), label      # the one-kernel product: it overwrites y
                products_are_the_reference(torch, product, rows, want, label)
                with sm.option(OPTION, alternate):            # a re-plan after an odd number of products
                    products_are_the_reference(torch, product, rows, want, label + ", one product", n=1)
                    T.set_tile(tile if tile else 1024)
                    T.set_x(dx)
                products_are_the_reference(torch, product, rows, want, label + ", after a re-plan", n=2)
            finally:
                T.close()
