"""The tile kernel's lane layout (csr_stream_owner, the row-ordered flavours Csr, Csr16 and TjdsK at 1024- and 2048-entry tiles):
neighbouring lanes take neighbouring entries, and y must not notice.

In phase 1 a wavefront takes 64 * VPT consecutive entries of its tile; its lane l holds, of every 128-entry slab m of them, the
two entries 2 l and 2 l + 1 (tile_layout.lane_entry restates the kernel's formula), loads them with one 16-byte value load and one
4-byte word of two 16-bit column offsets (or 8 bytes of col_ind / pos), gathers x for them and stores each product at its
row-major place in the tile's LDS array.  Everything after that barrier is as before, so every sum keeps its order:

  rows of at most 32 entries (kLongRow) are summed left to right by one lane: y must have the bits of the serial loop, which
      is computed here with a plain Python loop;
  longer rows are summed by a wavefront: y must lie within parity.check_y's row-wise bound of the oracle's csr_spmv.

The operand is a seeded random x (a product at the wrong place changes a sum), y is poisoned with NaN between guards before every
product.  The matrices are the smallest that reach every branch of the changed code at both tile sizes, with 256-entry tiles
(VPT == 1, unchanged) on the same matrices as a control; test_tile_layout_host.py checks on the host that they do, and that the
formula gives every entry of a full and of a partial tile to exactly one (lane, k).

What these tests can and cannot tell: every yardstick here is one the old layout met as well, so they guard y against a wrong
layout, they do not show which layout ran.  tile_layout.lane_entry is a hand copy of owner_body's lane_entry: whoever changes
the kernel's formula must change that function (and test_tile_layout_host.py's expectations) with it.  That the option
csr_sweep_alternate = 1 makes the second product of a handle sweep backward is the engine's rule, checked by
test_gpu_sweep_direction.py no more directly than here: nothing observable says which direction a launch took.
"""
import numpy as np
import pytest

import smvp_toolkit_amd as sm
from parity import check_guards, check_y, guarded_y
from tile_layout import CONTROL, KINDS, LONG_ROW, TILES, built_for, expected_flavor, matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()                        # (a copy: the matrices are read-only)


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def check_product(m, y, what):
    """Short rows: the serial loop's bits.  Long rows: the oracle within the row-wise bound.  No NaN anywhere."""
    short = m["lens"] <= LONG_ROW
    bad = np.flatnonzero(y[short].view(np.int64) != m["serial"][short].view(np.int64))
    assert not len(bad), "%s: %d rows of at most %d entries differ from the serial sum (%d NaN); first row %d: %r against %r" % (
        what, len(bad), LONG_ROW, np.isnan(y[short][bad]).sum(), np.flatnonzero(short)[bad[0]], y[short][bad[0]], m["serial"][short][bad[0]])
    check_y(y, m["oracle"], m["scale"], m["lens"])


def product(torch, A, dx, rows):
    buf, dy = guarded_y(torch, rows)
    A.spmv(dx, dy)
    torch.cuda.synchronize()
    check_guards(buf, rows)
    return dy.cpu().numpy()


@pytest.mark.parametrize("tile", TILES + (CONTROL,))
@pytest.mark.parametrize("kind", KINDS)
def test_csr_products(torch, kind, tile):
    """STREAM at this tile size on every structure: the kernel form the plan must resolve to, then y."""
    m = matrix(kind, built_for(tile))
    A = sm.CsrMatrix(m["rows"], m["cols"], m["row_ptr"], m["col_ind"], m["val"])
    try:
        A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
        assert A.describe()[0] == "csr_stream_owner<%d, %d, false>" % (tile // 256, expected_flavor(kind, tile))
        y = product(torch, A, dev(torch, m["x"]), m["rows"])
        check_product(m, y, "%s, tiles of %d" % (kind, tile))
        with sm.option("csr_col16", 0):              # the same matrix through col_ind alone
            A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
        assert A.describe()[0] == "csr_stream_owner<%d, 0, false>" % (tile // 256)
        y32 = product(torch, A, dev(torch, m["x"]), m["rows"])
        assert bits_equal(y32, y), "32-bit columns and 16-bit offsets give different bits"
    finally:
        A.close()


@pytest.mark.parametrize("tile", TILES + (CONTROL,))
@pytest.mark.parametrize("kind", ("tail", "giant"))
def test_tjds_row_gather(torch, kind, tile):
    """The row-ordered one-kernel TJDS product (TjdsK) against the CSR product on the same tile size.  It adds a row's products
    in ascending TJDS position, not in column order, so the yardstick is the row-wise bound on every row (a product at the
    wrong place is off by about sum|a x|, 10^13 bounds away) -- and its own bits when it runs again."""
    m = matrix(kind, built_for(tile))
    A = sm.CsrMatrix(m["rows"], m["cols"], m["row_ptr"], m["col_ind"], m["val"])
    with sm.option("tjds_index", 2):
        T = sm.TjdsMatrix(sm.tjds_from_coo(m["coo"], m["rows"], m["cols"]))
    try:
        T.set_tile(tile)
        assert T.describe()[0] == "csr_stream_owner<%d, 2, false>" % (tile // 256)
        A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
        want = product(torch, A, dev(torch, m["x"]), m["rows"])
        check_product(m, want, "%s, tiles of %d" % (kind, tile))
        T.set_x(dev(torch, m["x"]))
        ys = []
        for _ in range(2):
            buf, dy = guarded_y(torch, m["rows"])
            T.spmv(dy)
            torch.cuda.synchronize()
            check_guards(buf, m["rows"])
            ys.append(dy.cpu().numpy())
        check_y(ys[0], want, m["scale"], m["lens"])
        check_y(ys[0], m["oracle"], m["scale"], m["lens"])
        assert bits_equal(ys[0][m["lens"] <= 1], want[m["lens"] <= 1]), "rows of one entry or none: the CSR product's bits"
        assert bits_equal(ys[1], ys[0]), "the TJDS product by rows differs from itself"
    finally:
        T.close()
        A.close()


@pytest.mark.parametrize("tile", TILES)
def test_forward_and_backward_sweeps(torch, tile):
    """Option csr_sweep_alternate = 1: consecutive products of one handle sweep the tiles forward, backward, forward; all the
    first one's bits, and the bits of a handle that never alternates."""
    for kind in ("tail", "giant"):
        m = matrix(kind, tile)
        dx = dev(torch, m["x"])
        ys = []
        for alternate in (1, 0):
            with sm.option("csr_sweep_alternate", alternate):
                A = sm.CsrMatrix(m["rows"], m["cols"], m["row_ptr"], m["col_ind"], m["val"])
                A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
            try:
                ys += [product(torch, A, dx, m["rows"]) for _ in range(3)]
            finally:
                A.close()
        check_product(m, ys[0], "%s, tiles of %d, the first product" % (kind, tile))
        for i, y in enumerate(ys[1:]):
            assert bits_equal(y, ys[0]), "%s, tiles of %d: product %d differs from the first" % (kind, tile, i + 1)


@pytest.mark.parametrize("tile", TILES)
def test_repeating_launch(torch, tile):
    """One device-timed run of the entry point on the smallest matrix: three products in one repeating launch
    (csr_stream_owner_repeat walks the same body); y is the single launch's."""
    m = matrix("exact_less_one", tile)
    A = sm.CsrMatrix(m["rows"], m["cols"], m["row_ptr"], m["col_ind"], m["val"])
    try:
        A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
        want = product(torch, A, dev(torch, m["x"]), m["rows"])
    finally:
        A.close()
    check_product(m, want, "exact_less_one, tiles of %d" % tile)
    y, ms, st = sm.csr_compute(m["coo"], m["rows"], m["cols"], iters=3, x=m["x"], timing=sm.TIMING_DEVICE,
                               kernel=sm.CSR_KERNEL_STREAM, param=tile)
    info = sm.last_run_info()
    assert (info.timing, info.repeat_launches, info.graph_replays, info.repeat_gave_up) == (sm.TIMING_DEVICE, 1, 0, 0)
    assert len(ms) == 3 and np.isfinite(ms).all() and (ms > 0).all()
    assert bits_equal(y, want), "the repeating launch's y differs from the single launch's"
