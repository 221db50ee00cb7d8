"""GPU: SMVP_CSR_KERNEL_STREAM_PACKED -- the tile kernel reading frequent values as 1-byte codes (csr_stream_owner<8, 6, .>).

Every product is compared with STREAM's at 2048-entry tiles on the same arrays, bit for bit (int64 views), for x = ones and for a
random x: the packed form multiplies the very doubles val holds and sums every row as STREAM does, so there is no tolerance
anywhere.  tests/packed_values.py has the structures (six full tiles and a partial one; one tile; less than one; a wide tile in
the middle; a long row and a giant row) and the value sets, and computes on the host what the plan must find -- the hot table, the
escapes per wavefront, the escape share.  y lies in a guarded buffer.  The contract tests hold include/smvp_amd.h's sentences on the
family: it keeps a copy of the values, smvp_csr_get_kernel names it, AUTO picks it by its rule only.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import packed_values as pv
import smvp_toolkit_amd as sm
from parity import check_guards, guarded_y

pytestmark = pytest.mark.gpu

PACKED, STREAM = sm.CSR_KERNEL_STREAM_PACKED, sm.CSR_KERNEL_STREAM
S = 0.55     # AUTO's bound on the escape share (kPackedMaxEscapeShare, csrc/smvp_engine.hip)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


STRUCTURES = {
    "six tiles and a tail": lambda: pv.base(),
    "one tile": lambda: pv.base(tiles=1, tail=0, seed=12, cols=700),
    "less than one tile": lambda: pv.base(tiles=0, tail=1500, seed=13, cols=500),
    "a wide tile": lambda: pv.with_wide_tile(*pv.base()),
    "long and giant rows": lambda: pv.with_long_and_giant_rows(),
}
_built = {}


def matrix(name):
    if name not in _built:
        rows, cols, rp, ci = STRUCTURES[name]()
        for a in (rp, ci):
            a.setflags(write=False)
        _built[name] = (rows, cols, rp, ci)
    return _built[name]


def operands(cols):
    return {"ones": np.ones(cols), "random": np.random.default_rng(67890).random(cols) - 0.25}


def product(torch, A, x, rows):
    buf, y = guarded_y(torch, rows)
    A.spmv(torch.from_numpy(x).cuda(), y, stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    check_guards(buf, rows)
    return y.cpu().numpy().view(np.int64)


def both(torch, rows, cols, rp, ci, val):
    """{x: (STREAM 2048's y, STREAM_PACKED's y)} as int64, from one handle planned twice; asserts what the handle says of itself."""
    out = {}
    A = sm.CsrMatrix(rows, cols, rp, ci, val)
    try:
        for x_name, x in operands(cols).items():
            A.set_kernel(STREAM, 2048)
            assert A.get_kernel() == (STREAM, 2048) and A.describe()[0] == "csr_stream_owner<8, 5, false>"
            want = product(torch, A, x, rows)
            A.set_kernel(PACKED, 0)
            assert A.get_kernel() == (PACKED, 2048) and A.describe()[0] == "csr_stream_owner<8, 6, false>"
            assert A.launches() == 1
            got = product(torch, A, x, rows)
            again = product(torch, A, x, rows)
            assert np.array_equal(got, again), "two runs of the packed product differ (x = %s)" % x_name
            out[x_name] = (want, got)
    finally:
        A.close()
    return out


def assert_same_bits(pairs, what, mask=None):
    for x_name, (want, got) in pairs.items():
        w, g = (want, got) if mask is None else (want[mask], got[mask])
        bad = np.flatnonzero(w != g)
        assert bad.size == 0, "%s, x = %s: %d rows differ from STREAM 2048, first row %d: %#x against %#x" % (
            what, x_name, bad.size, bad[0], g[bad[0]], w[bad[0]])


# ------------------------------------------------------------------------------------------------------------- the products
@pytest.mark.parametrize("kind", pv.KINDS)
@pytest.mark.parametrize("name", ["six tiles and a tail", "one tile", "less than one tile"])
def test_bits_of_stream_on_every_value_set(torch, name, kind):
    rows, cols, rp, ci = matrix(name)
    val = pv.values(kind, rp, ci)
    per = [p for p in pv.escapes_per_wavefront(rp, ci, val) if p is not None]
    if name == "six tiles and a tail":     # the value sets are what their names say (computed from the hot table the plan must find)
        counts = np.concatenate(per)
        if kind in ("hot64", "few"):
            assert counts.sum() == 0
        if kind == "few":
            assert len(np.unique(pv.bits(val))) < pv.HOT
        if kind == "distinct":
            assert np.all(counts == pv.WAVE)
        if kind == "half":
            assert (counts % 2 == 1).any() and (counts % 2 == 0).any() and per[2][0] == 0 and per[2][1] == pv.WAVE
            assert 0.3 < pv.escape_share(rp, ci, val) < 0.7
        if kind.startswith("special"):
            special = ~np.isfinite(val) | (val == 0) | (np.abs(val) < 1e-300)
            hot = np.isin(pv.bits(val), pv.hot_table(val))
            full = np.arange(len(val)) < len(val) // pv.TILE * pv.TILE
            assert np.all(hot[special]) if kind == "special_hot" else not np.any(hot[special])
            assert len(np.unique(pv.bits(val[special & full]))) == 7
    pairs = both(torch, rows, cols, rp, ci, val)
    # special values: the rows whose bits the tile kernel defines are those one lane sums left to right (at most 32 entries); on the
    # others the two forms must still agree on what is a NaN
    if kind.startswith("special"):
        short = np.diff(rp) <= pv.LONG_ROW
        assert_same_bits(pairs, "%s, %s" % (name, kind), short)
        for x_name, (want, got) in pairs.items():
            assert np.array_equal(np.isnan(want.view(np.float64)), np.isnan(got.view(np.float64))), x_name
    else:
        assert_same_bits(pairs, "%s, %s" % (name, kind))
        for want, got in pairs.values():
            assert not np.isnan(got.view(np.float64)).any()


@pytest.mark.parametrize("kind", ["half", "distinct"])
def test_a_wide_tile_reads_val_and_its_neighbours_stay_packed(torch, kind):
    rows, cols, rp, ci = matrix("a wide tile")
    val = pv.values(kind, rp, ci)
    ok = pv.packable_tiles(rp, ci)
    assert list(ok) == [True, True, True, False, True, True, False]
    assert_same_bits(both(torch, rows, cols, rp, ci, val), "a wide tile, " + kind)


@pytest.mark.parametrize("kind", ["half", "hot64"])
def test_long_and_giant_rows(torch, kind):
    rows, cols, rp, ci = matrix("long and giant rows")
    lens = np.diff(rp)
    assert (lens > pv.LONG_ROW).any() and lens.max() > pv.OVER
    val = pv.values(kind, rp, ci)
    assert_same_bits(both(torch, rows, cols, rp, ci, val), "long and giant rows, " + kind)


def test_the_stamped_form_through_csr_compute(torch):
    """One timed run through smvp_csr_compute with the family set: single stamped launches (the family has no repeating form)."""
    rows, cols, rp, ci = matrix("six tiles and a tail")
    val = pv.values("half", rp, ci)
    coo = sm.make_coo(np.repeat(np.arange(rows), np.diff(rp)), ci, val)
    x = operands(cols)["random"]
    want, ms0, _ = sm.csr_compute(coo, rows, cols, iters=3, kernel=STREAM, param=2048, x=x, timing=sm.TIMING_DEVICE)
    got, ms, _ = sm.csr_compute(coo, rows, cols, iters=3, kernel=PACKED, param=0, x=x, timing=sm.TIMING_DEVICE)
    assert np.array_equal(want.view(np.int64), got.view(np.int64))
    assert np.all(ms > 0) and np.all(ms < 50.0)


# --------------------------------------------------------------------------------------------------------------- the contract
def test_val_changed_in_place_is_seen_after_set_kernel(torch):
    rows, cols, rp, ci = matrix("six tiles and a tail")
    val0, val1 = pv.values("half", rp, ci), pv.values("half", rp, ci, seed=6)
    assert not np.array_equal(val0, val1)
    x = operands(cols)["random"]
    d_rp, d_ci, d_val = (torch.from_numpy(np.array(a)).cuda() for a in (rp, ci, val0))
    A = sm.CsrMatrix(rows, cols, d_rp, d_ci, d_val)
    try:
        ys = {}
        for label, v in (("val0", val0), ("val1", val1), ("val0 again", val0)):
            d_val.copy_(torch.from_numpy(v))
            A.set_kernel(STREAM, 2048)
            want = product(torch, A, x, rows)
            A.set_kernel(PACKED, 0)
            assert A.get_kernel()[0] == PACKED
            ys[label] = product(torch, A, x, rows)
            assert np.array_equal(ys[label], want), label
        assert np.array_equal(ys["val0"], ys["val0 again"]) and not np.array_equal(ys["val0"], ys["val1"])
    finally:
        A.close()


def auto_pick(rows, cols, rp, ci, val, packed=None):
    with sm.option("csr_packed", packed):
        A = sm.CsrMatrix(rows, cols, rp, ci, val)
    try:
        return A.get_kernel(), A.describe()[0]
    finally:
        A.close()


def test_auto_picks_the_family_by_its_rule_only(torch):
    rows, cols, rp, ci = matrix("six tiles and a tail")
    under, over = pv.values("third", rp, ci), pv.values("distinct", rp, ci)
    assert pv.escape_share(rp, ci, under) < S - 0.1 and S + 0.1 < pv.escape_share(rp, ci, over)
    # a small matrix: STREAM by default, whatever its values
    for val in (under, over, pv.values("hot64", rp, ci)):
        assert auto_pick(rows, cols, rp, ci, val)[0][0] == STREAM
    # csr_packed 1 waives the size, not the share
    assert auto_pick(rows, cols, rp, ci, under, 1) == ((PACKED, 2048), "csr_stream_owner<8, 6, false>")
    assert auto_pick(rows, cols, rp, ci, over, 1) == auto_pick(rows, cols, rp, ci, over)
    assert auto_pick(rows, cols, rp, ci, over, 1)[0][0] == STREAM
    # csr_packed 0: never
    assert auto_pick(rows, cols, rp, ci, under, 0)[0][0] == STREAM
    # AUTO under csr_packed 1 multiplies like STREAM 2048, and re-planning on AUTO keeps the rule
    x = operands(cols)["random"]
    with sm.option("csr_packed", 1):
        A = sm.CsrMatrix(rows, cols, rp, ci, under)
        try:
            got = product(torch, A, x, rows)
            A.set_kernel(STREAM, 2048)
            want = product(torch, A, x, rows)
            A.set_kernel(sm.CSR_KERNEL_AUTO, 0)
            assert A.get_kernel()[0] == PACKED
        finally:
            A.close()
    assert np.array_equal(got, want)


def test_auto_attaches_to_a_standing_plan_and_stops_at_the_count_over_the_bound(torch):
    """From 12 M entries on AUTO's STREAM plan already has 2048-entry tiles with 16-bit offsets: under csr_packed 1 (which waives only
    the 1 GiB) AUTO then attaches the packed arrays to the standing plan, as it does by its default rule on a matrix of more than
    1 GiB -- or, where the share is over the bound, stops at the exact count and keeps the plan as it stands.  A band of 8 entries per
    row, 12.6 M entries: the smallest matrix that takes this path."""
    n = 12 * 1024 * 1024 // 8 + 40000
    rp = (np.arange(n + 1, dtype=np.int64) * 8).astype(np.int32)
    ci = np.minimum(np.arange(n, dtype=np.int64)[:, None] + np.arange(8), n - 1).astype(np.int32).ravel()   # (the last rows repeat column n - 1)
    x = np.random.default_rng(3).random(n)
    rng = np.random.default_rng(4)
    under = rng.integers(1, 17, 8 * n) / 16.0                       # 16 values: no escapes
    over = 1.0 + np.arange(8 * n) / float(1 << 32)                   # all different: every entry of a full tile escapes
    for val, want_kernel in ((under, PACKED), (over, STREAM)):
        plain = sm.CsrMatrix(n, n, rp, ci, val)
        with sm.option("csr_packed", 1):
            A = sm.CsrMatrix(n, n, rp, ci, val)
        try:
            assert plain.get_kernel() == (STREAM, 2048) and plain.describe()[0] == "csr_stream_owner<8, 5, false>"
            assert A.get_kernel() == (want_kernel, 2048)
            assert A.describe()[0] == ("csr_stream_owner<8, 6, false>" if want_kernel == PACKED else "csr_stream_owner<8, 5, false>")
            extra = A.plan_info()["plan_bytes"] - plain.plan_info()["plan_bytes"]
            ntiles = -(-8 * n // pv.TILE)
            assert extra == (8 * n + 8 * pv.HOT + 4 * (4 * ntiles + 1) if want_kernel == PACKED else 0)      # no escape slot / nothing kept
            assert np.array_equal(product(torch, A, x, n), product(torch, plain, x, n))
        finally:
            A.close()
            plain.close()


def test_refused_where_the_offsets_are_not_in_use(torch):
    rows, cols, rp, ci = matrix("six tiles and a tail")
    val = pv.values("half", rp, ci)
    with sm.option("csr_col16", 0):
        A = sm.CsrMatrix(rows, cols, rp, ci, val)
        try:
            with pytest.raises(sm.SmvpError):
                A.set_kernel(PACKED, 0)
            assert A.get_kernel()[0] == STREAM       # the handle stays usable, on STREAM
            product(torch, A, operands(cols)["ones"], rows)
            with pytest.raises(sm.SmvpError):
                A.set_kernel(PACKED, 1024)           # no such tile size
        finally:
            A.close()


def test_plan_bytes_count_the_packed_arrays(torch):
    rows, cols, rp, ci = matrix("six tiles and a tail")
    val = pv.values("half", rp, ci)
    A = sm.CsrMatrix(rows, cols, rp, ci, val)
    try:
        A.set_kernel(STREAM, 2048)
        plain = A.plan_info()["plan_bytes"]
        A.set_kernel(PACKED, 0)
        nnz, ntiles = len(val), -(-len(val) // pv.TILE)
        slots = sum(int(((p + 1) // 2 * 2).sum()) for p in pv.escapes_per_wavefront(rp, ci, val) if p is not None)
        assert A.plan_info()["plan_bytes"] - plain == nnz + 8 * pv.HOT + 4 * (4 * ntiles + 1) + 8 * slots
        assert A.describe()[1] == 12.0 * nnz + 4.0 * (rows + 1) + 8.0 * cols + 8.0 * rows      # the algorithmic bytes, as STREAM reports them
    finally:
        A.close()


def test_allocations_return_to_their_start():
    """The counted build of the library (tests/resource_count.cpp) in a process of its own: tests/packed_values_scenarios.py."""
    counted = os.path.join(ROOT, "smvp-toolkit_amd", "lib", "libsmvp_amd_counted.so")
    if not os.path.exists(counted):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "smvp-toolkit_amd"), "lib/libsmvp_amd_counted.so"])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "packed_values_scenarios.py")], env=dict(os.environ, SMVP_LIB_PATH=counted),
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0 and p.stdout.strip().endswith("packed values ok"), "exit status %d\n%s\n%s" % (
        p.returncode, p.stdout[-3000:], p.stderr[-3000:])
