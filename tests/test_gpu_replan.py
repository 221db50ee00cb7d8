"""GPU: a handle walked from plan to plan behaves like one that was given its last plan directly.

What this pins is state left over from one plan when the next is built.  A CSR handle goes through every ordered pair of the
five kernel families (STREAM, STREAM_CARRY, VECTOR, COLSWEEP, BINNED) with changing parameters, two refused calls in between,
and ends on AUTO; a TJDS handle goes through the tile sizes, the value cache and the modes for each index form of its
row-gather stream, and through ref-quirks on and off between the modes (the matrices of ref_quirks_walk.py).  After every step a fresh handle is created and configured the same way: get_kernel(), describe(),
launches() and plan_info() (but for build_ms) are equal and the product into a guarded y has the same bits.  Once per family
the product is also held against the oracle (parity.check_y).  smvp_csr_spmm's plan, which belongs to row_ptr alone, gives the
same bits and reports the same bytes before and after the walk.

The matrices: 2000 rows of 5 entries, 10 empty rows, one row of 3000 and 500 rows of 40 -- several tiles at every tile size,
rows that straddle tiles, a row longer than a 2048-entry tile with more far entries than the binned plan's per-row cap (1024:
the row stays near) -- over 50 000 columns (A: every tile's columns span < 65536, so the 16-bit column offsets engage at
1024- / 2048-entry tiles) and over 200 000 columns (B: they cannot).
"""
import contextlib

import numpy as np
import pytest

import oracle_binding as ob
import ref_quirks_walk
import smvp_toolkit_amd as sm
from parity import check_guards, check_y, guarded_y
from test_gpu_parity import csr_from_lengths, row_scale
from test_gpu_spmm import spmm
from transposed import assert_bits

pytestmark = pytest.mark.gpu

LENS = [5] * 2000 + [0] * 10 + [3000] + [40] * 500
COLS = {"A": 50_000, "B": 200_000}

S, C, V, W, B = (sm.CSR_KERNEL_STREAM, sm.CSR_KERNEL_STREAM_CARRY, sm.CSR_KERNEL_VECTOR, sm.CSR_KERNEL_COLSWEEP,
                 sm.CSR_KERNEL_BINNED)
WALK = [S, C, V, W, B, S, V, B, C, W, S, W, C, B, V, S, B, W, V, C, S]
# (param, plan options) of a family's visits, in turn
VISITS = {S: [(0, {}), (1024, {}), (2048, {}), (256, {})],
          C: [(0, {}), (2048, {}), (1024, {})],
          V: [(0, {}), (8, {}), (64, {})],
          W: [(0, {}), (256, {}), (sm.sweep_parts(256, 2), {})],
          B: [(0, {}), (64, {}), (0, {"binned_near": 1})]}          # binned_near 1: the near part behind a nested handle
REFUSED = {3: (S, 512), 7: (W, 255)}                                 # after step 3 (on COLSWEEP) and step 7 (on BINNED)


def test_the_walk_takes_every_ordered_pair_of_families_once():
    pairs = list(zip(WALK, WALK[1:]))
    assert len(pairs) == len(set(pairs)) == 20 and all(a != b for a, b in pairs)
    assert all(len(VISITS[f]) <= WALK.count(f) for f in VISITS)     # every parameter of VISITS is used


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def matrices():
    """name -> (rows, cols, row_ptr, col_ind, val, x, the oracle's y, sum|a x| per row), computed once and left unchanged."""
    out = {}
    for name, cols in COLS.items():
        rng = np.random.default_rng(2511 + cols)
        rp, ci, v = csr_from_lengths(rng, LENS, cols)
        x = rng.random(cols)
        arrays = (rp, ci, v, x, ob.csr_spmv(rp, ci, v, x), row_scale(rp, ci, v, x))
        for a in arrays:
            a.setflags(write=False)
        out[name] = (len(LENS), cols) + arrays
    assert out["A"][2][-1] == 33_000 and out["A"][0] == 2511
    return out


@contextlib.contextmanager
def options(opts):
    with contextlib.ExitStack() as stack:
        for option, value in opts.items():
            stack.enter_context(sm.option(option, value))
        yield


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()                      # (a copy: the fixture's arrays are read-only)


def product(torch, A, dx):
    buf, dy = guarded_y(torch, A.rows)
    A.spmv(dx, dy)
    torch.cuda.synchronize()
    check_guards(buf, A.rows)
    return dy.cpu().numpy()


def csr_state(A):
    info = A.plan_info()
    return A.get_kernel(), A.describe(), A.launches(), info["matrix_bytes"], info["plan_bytes"]


# ------------------------------------------------------------------------------------------------------------- CSR walk
@pytest.mark.parametrize("name", sorted(COLS))
def test_csr_walk_through_every_pair_of_families(torch, matrices, name):
    rows, cols, rp, ci, v, x, ref, scale = matrices[name]
    terms = np.diff(rp)
    dx = dev(torch, x)
    X = np.random.default_rng(3).random((cols, 3))
    A = sm.CsrMatrix(rows, cols, rp, ci, v)
    Y_before = spmm(torch, A, X, 3, 3, 3)
    spmm_bytes = A.spmm_describe(3)[2]["plan_bytes"]
    assert spmm_bytes > 0

    def against_fresh(kernel, param, opts, what):
        fresh = sm.CsrMatrix(rows, cols, rp, ci, v)
        with options(opts):
            fresh.set_kernel(kernel, param)
        assert csr_state(A) == csr_state(fresh), what
        y = product(torch, A, dx)
        assert_bits(y, product(torch, fresh, dx), what + " (%s), walked against fresh" % A.describe()[0])
        fresh.close()
        return y

    seen, col16 = {}, set()
    for step, family in enumerate(WALK):
        param, opts = VISITS[family][seen.get(family, 0) % len(VISITS[family])]
        what = "%s, step %d: kernel %d param %d %r" % (name, step, family, param, opts)
        with options(opts):
            A.set_kernel(family, param)
        assert A.get_kernel()[0] == family, what
        y = against_fresh(family, param, opts, what)
        if family not in seen:
            check_y(y, ref, scale, terms)
        seen[family] = seen.get(family, 0) + 1
        if family == S:
            col16.add((A.get_kernel()[1], A.describe()[0]))
        if step in REFUSED:
            before = A.get_kernel(), A.describe()
            with pytest.raises(sm.SmvpError) as e:
                A.set_kernel(*REFUSED[step])
            assert e.value.code == sm.ERR_INVALID, what
            assert (A.get_kernel(), A.describe()) == before, what + ", after the refused %r" % (REFUSED[step],)
            assert_bits(product(torch, A, dx), y, what + ", after the refused %r" % (REFUSED[step],))
    # the 16-bit column offsets (flavour 5 in the kernel's name, plain CSR is 0) engaged on A at 1024 / 2048 entries per tile only
    flavour = {tile: int(kernel_name.split(",")[1]) for tile, kernel_name in col16}
    assert flavour == {256: 0, 1024: 5 * (name == "A"), 2048: 5 * (name == "A")}, col16

    A.set_kernel(sm.CSR_KERNEL_AUTO, 0)
    check_y(against_fresh(sm.CSR_KERNEL_AUTO, 0, {}, name + ", AUTO at the end"), ref, scale, terms)
    assert_bits(spmm(torch, A, X, 3, 3, 3), Y_before, name + ", spmm after the walk")
    assert A.spmm_describe(3)[2]["plan_bytes"] == spmm_bytes
    A.close()


# ------------------------------------------------------------------------------------------------------------ TJDS walk
def tjds_product(torch, T, dx):
    buf, dy = guarded_y(torch, T.rows)
    T.set_x(dx)
    T.zero_y(dy)
    T.spmv(dy)
    torch.cuda.synchronize()
    check_guards(buf, T.rows)
    return dy.cpu().numpy()


@pytest.mark.parametrize("index", [0, 1, 2])
def test_tjds_walk_through_tiles_value_cache_and_modes(torch, matrices, index):
    rows, cols, rp, ci, v, x, ref, scale = matrices["A"]
    terms = np.diff(rp)
    dx = dev(torch, x)
    t = sm.tjds_from_coo(sm.make_coo(np.repeat(np.arange(rows), terms), ci, v), rows, cols)
    steps = [("tile", 256), ("tile", 1024), ("tile", 2048)]
    if index < 2:                                                    # (the row-order stream, index 2, has no value cache)
        steps += [("cache", 0), ("cache", 16), ("cache", 2)]
    steps += [("mode", sm.TJDS_MODE_TWO_PHASE), ("mode", sm.TJDS_MODE_ATOMIC), ("mode", sm.TJDS_MODE_ROW_GATHER), ("tile", 1024)]
    with sm.option("tjds_index", index):
        T = sm.TjdsMatrix(t)
    setters = {"tile": "set_tile", "cache": "set_value_cache", "mode": "set_mode"}
    now = {}                                                         # what the walked handle is configured to: setter -> value
    for step, (kind, value) in enumerate(steps):
        what = "tjds_index %d, step %d: %s %d" % (index, step, setters[kind], value)
        getattr(T, setters[kind])(value)
        now[kind] = value
        with sm.option("tjds_index", index):
            fresh = sm.TjdsMatrix(t)
        for k in ("tile", "cache", "mode"):                          # (the tile and the cache belong to the row-gather plan,
            if k in now:                                             #  which every mode keeps: set before the mode)
                getattr(fresh, setters[k])(now[k])
        assert T.describe() == fresh.describe() and T.get_value_cache() == fresh.get_value_cache(), what
        if "mode" not in now:                                        # (afterwards the walked handle keeps the other modes' plans)
            assert T.plan_info()["plan_bytes"] == fresh.plan_info()["plan_bytes"], what
        y = tjds_product(torch, T, dx)
        if now.get("mode") == sm.TJDS_MODE_ATOMIC:
            check_y(y, ref, scale, terms)
            check_y(tjds_product(torch, fresh, dx), ref, scale, terms)
        else:
            assert_bits(y, tjds_product(torch, fresh, dx), what + " (%s), walked against fresh" % T.describe()[0])
            if step == 0:
                check_y(y, ref, scale, terms)
        fresh.close()
    T.close()


# the work items carry both the ref-quirks flag and the copy of start_pos that TWO_PHASE's first phase reads: each is changed
# with the other in every state
QUIRKS_WALK = [("quirks", True), ("mode", sm.TJDS_MODE_TWO_PHASE), ("quirks", False), ("mode", sm.TJDS_MODE_ATOMIC), ("quirks", True),
               ("mode", sm.TJDS_MODE_ROW_GATHER), ("quirks", False), ("tile", 256), ("quirks", True), ("quirks", False)]


@pytest.mark.parametrize("index", [0, 2])
@pytest.mark.parametrize("name", sorted(ref_quirks_walk.LONGEST_COLUMNS))
def test_tjds_walk_through_ref_quirks_and_modes(torch, name, index):
    """Exact operands: every product equals the oracle's -- ob.tjds_spmv with refquirks as the handle is set -- and the fresh
    handle's bit for bit, the atomic kernel's included.  A second handle takes the walk's mode steps only: the plan bytes of the
    two are equal before the first step and after the last, so toggling ref-quirks leaves no bytes behind and loses none."""
    m = ref_quirks_walk.matrix(name)
    t = sm.tjds_from_coo(m.coo, m.rows, m.cols)
    assert t.last_diag_single == m.oracle.last_diag_single
    dx = dev(torch, m.x)
    setters = {"tile": "set_tile", "mode": "set_mode", "quirks": "set_ref_quirks"}
    with sm.option("tjds_index", index):
        T, modes_only = sm.TjdsMatrix(t), sm.TjdsMatrix(t)
    assert T.plan_info()["plan_bytes"] == modes_only.plan_info()["plan_bytes"]
    now = {}
    for step, (kind, value) in enumerate(QUIRKS_WALK):
        what = "%s, tjds_index %d, step %d: %s %d" % (name, index, step, setters[kind], value)
        getattr(T, setters[kind])(value)
        now[kind] = value
        if kind == "mode":
            modes_only.set_mode(value)
        with sm.option("tjds_index", index):
            fresh = sm.TjdsMatrix(t)
        for k in ("tile", "mode", "quirks"):
            if k in now:
                getattr(fresh, setters[k])(now[k])
        assert T.describe() == fresh.describe() and T.get_value_cache() == fresh.get_value_cache(), what
        y = tjds_product(torch, T, dx)                               # (checks the guards)
        assert_bits(y, tjds_product(torch, fresh, dx), what + " (%s), walked against fresh" % T.describe()[0])
        assert np.array_equal(y, m.y[now["quirks"]]), what + " (%s), against the oracle" % T.describe()[0]
        fresh.close()
    assert T.plan_info()["plan_bytes"] == modes_only.plan_info()["plan_bytes"]
    modes_only.close()
    T.close()
