"""GPU: the forward products y = A x on non-finite, signed-zero, subnormal and overflowing operands (tests/special_values.py
has the scenarios A ... G, their structures and conditions, and the assertions; test_special_values_host.py shows on the host
that those assertions reject the wrong kernels they are for).

Every scenario runs on every path: the CSR_VARIANTS of test_gpu_parity.py and AUTO, COLSWEEP with 2 | 4 | 8 column parts,
STREAM with the plan options csr_col16 / csr_rowrel on and off, BINNED with binned_near 0 and 1, the TJDS_MODES, the
TJDS_GATHER_VARIANTS with the value cache off and -- where the stream form has one ("half", "sorted") -- on.  y always lies
in a guarded buffer; scenarios A and B also run with x and y shifted by one double.  The reference is the oracle's serial loop.
Exemptions: scenario A compares bits with the same handle's product of the clean x except on TJDS ATOMIC (not reproducible
from run to run: parity.check_y against the oracle there); structures of fewer than 64 columns take no part in A; G runs on
the paths that promise the serial loop's bits.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import smvp_toolkit_amd as sm
import special_values as sv
from parity import G as GUARD_DOUBLES, GUARD, check_guards, check_y
from test_gpu_parity import CSR_VARIANTS, TJDS_GATHER_VARIANTS, TJDS_MODES, tjds_gather_matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# ------------------------------------------------------------------------------------------------------------------ paths
def serial_rows(name, row_ptr, ascending):
    """The rows a CSR kernel (by its describe() name) sums left to right by one lane, i.e. with the serial loop's bits: every
    row of the column sweep without column parts (columns ascending), rows of up to 32 entries of the owner form of the tile
    kernel, and of the carry form where they lie inside one tile."""
    lens = np.diff(row_ptr)
    if name.startswith("csr_colsweep<") and "parts" not in name:
        return np.full(len(lens), bool(ascending))
    if name.startswith("csr_stream_owner<"):
        return lens <= 32
    if name.startswith("csr_stream_tiles<"):
        tile = 256 * int(name[len("csr_stream_tiles<"):].split(">")[0])
        return (lens <= 32) & (row_ptr[:-1] // tile == (np.maximum(row_ptr[1:], 1) - 1) // tile)
    return np.zeros(len(lens), dtype=bool)


def csr_paths(rows, cols, row_ptr, col_ind, val, only_serial=False, first_row=0):
    """(label, run, serial-rows mask or None for "not reproducible", kernel name) of every CSR path, one after the other; run(dx,
    dy, stream=None) enqueues one product on `stream`.  first_row: the handles are row blocks (smvp_csr_create_block)."""
    ascending = bool(np.all((np.diff(col_ind.astype(np.int64)) > 0) | (np.diff(sv.row_of_entries(row_ptr)) > 0))) if len(col_ind) > 1 else True

    def path(A, label):
        name = A.describe()[0]
        return label, (lambda dx, dy, stream=None: A.spmv(dx, dy, stream=stream)), serial_rows(name, row_ptr, ascending), name

    A = sm.CsrMatrix(rows, cols, row_ptr, col_ind, val, first_row=first_row)
    try:
        settings = [("AUTO", sm.CSR_KERNEL_AUTO, 0)] + [("kernel %d param %d" % kp, kp[0], kp[1]) for kp in CSR_VARIANTS] + \
                   [("COLSWEEP 1024 rows, %d parts" % p, sm.CSR_KERNEL_COLSWEEP, sm.sweep_parts(1024, p)) for p in (2, 4, 8)]
        for label, kernel, param in settings:
            if only_serial and kernel not in (sm.CSR_KERNEL_AUTO, sm.CSR_KERNEL_STREAM, sm.CSR_KERNEL_STREAM_CARRY, sm.CSR_KERNEL_COLSWEEP):
                continue
            A.set_kernel(kernel, param)
            assert kernel == sm.CSR_KERNEL_AUTO or A.get_kernel()[0] == kernel, label
            yield path(A, label)
    finally:
        A.close()
    for col16 in (1, 0):
        for rowrel in (None, 0):
            with sm.option("csr_col16", col16), sm.option("csr_rowrel", rowrel):
                A = sm.CsrMatrix(rows, cols, row_ptr, col_ind, val, first_row=first_row)
                try:
                    A.set_kernel(sm.CSR_KERNEL_STREAM, 1024)
                    yield path(A, "STREAM 1024, csr_col16 %r, csr_rowrel %r" % (col16, rowrel))
                finally:
                    A.close()
    if only_serial:
        return
    for near in (0, 1):
        with sm.option("binned_near", near):
            A = sm.CsrMatrix(rows, cols, row_ptr, col_ind, val, first_row=first_row)
            try:
                A.set_kernel(sm.CSR_KERNEL_BINNED, 0)
                yield path(A, "BINNED band 0, binned_near %d" % near)
            finally:
                A.close()


def tjds_paths(rows, cols, row_ptr, col_ind, val):
    """(label, run, mask, name) of every TJDS path; mask is None on TJDS ATOMIC (hardware atomics: the order of a row's sum
    changes from run to run), all-False elsewhere (reproducible, but no promise of the serial loop's bits)."""
    coo = sm.make_coo(sv.row_of_entries(row_ptr), col_ind[:row_ptr[-1]], val[:row_ptr[-1]])
    t = sm.tjds_from_coo(coo, rows, cols)
    none = np.zeros(rows, dtype=bool)

    def run_of(T):
        def run(dx, dy, stream=None):
            T.set_x(dx, stream=stream)
            T.zero_y(dy, stream=stream)
            T.spmv(dy, stream=stream)
        return run

    T = sm.TjdsMatrix(t)
    try:
        for mode in TJDS_MODES:
            T.set_mode(mode)
            yield "TJDS mode %d" % mode, run_of(T), (None if mode == sm.TJDS_MODE_ATOMIC else none), T.describe()[0]
    finally:
        T.close()
    for index, tile in TJDS_GATHER_VARIANTS:
        T = tjds_gather_matrix(t, index, tile)
        try:
            for cache in ((0, 1) if index in ("half", "sorted") else (0,)):       # (the row-order stream "k32" has no value cache)
                T.set_value_cache(cache)
                assert T.get_value_cache()[0] == cache and (T.get_value_cache()[1] > 0) == (cache == 1 and len(coo) > 0)
                yield "TJDS %s tile %d, value cache %d" % (index, tile, cache), run_of(T), none, T.describe()[0]
        finally:
            T.close()


def all_paths(rows, cols, row_ptr, col_ind, val):
    yield from csr_paths(rows, cols, row_ptr, col_ind, val)
    yield from tjds_paths(rows, cols, row_ptr, col_ind, val)


class Operands:
    """x and a guarded y on the device, 16-byte aligned (shift 0) or one double off (shift 1)."""

    def __init__(self, torch, rows, cols):
        self.torch, self.rows, self.cols = torch, rows, cols
        self.bx = torch.zeros(cols + 1, dtype=torch.float64, device="cuda")
        self.by = torch.empty(rows + 2 * GUARD_DOUBLES + 1, dtype=torch.float64, device="cuda")

    def product(self, run, x, shift=0):
        torch, rows, g = self.torch, self.rows, GUARD_DOUBLES
        dx = self.bx[shift:shift + self.cols]
        dx.copy_(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)))
        self.by.view(torch.int64).fill_(int(GUARD))
        dy = self.by[g + shift:g + shift + rows]
        dy.fill_(float("nan"))
        run(dx, dy)
        torch.cuda.synchronize()
        check_guards(self.by[shift:shift + rows + 2 * g], rows)
        return dy.cpu().numpy()


def scale_of(row_ptr, col_ind, val, x):
    with np.errstate(invalid="ignore"):
        return ob.csr_spmv(row_ptr, col_ind, np.abs(val), np.abs(x))


# -------------------------------------------------------------------------------------------------------------- scenarios
@pytest.mark.parametrize("name", sv.STRUCTURES)
def test_scenarios_a_to_d_on_every_path(torch, name):
    """A (poison nobody references), B (poison in referenced columns), C (stored zeros under Inf), D (signed zeros)."""
    rows, cols, rp, ci, u = sv.structure(name)
    o = sv.ordinary(rows, cols, rp, ci, u)
    val, terms = o["val"], np.diff(rp)
    with_a = cols >= sv.MIN_COLS_A
    sv.assert_regime(name, "A", rows, cols, rp, ci, val, o["x_a"], u)
    want = {}
    for key, scenario in (("x", None), ("x_a", "A"), ("x_b", "B"), ("x_c", "C")):
        if scenario in ("B", "C"):
            sv.assert_regime(name, scenario, rows, cols, rp, ci, val, o[key])
        want[key] = (ob.csr_spmv(rp, ci, val, o[key]), scale_of(rp, ci, val, o[key]), sv.row_classes(rp, ci, val, o[key]))
    zeros = (np.zeros(cols), -np.zeros(cols))
    for z in zeros:
        sv.assert_regime(name, "D", rows, cols, rp, ci, val, z)
    ops = Operands(torch, rows, cols)
    checks = 0
    for label, run, serial, kernel in all_paths(rows, cols, rp, ci, val):
        what = "%s, %s (%s)" % (name, label, kernel)
        if with_a:
            if serial is None:                                       # TJDS ATOMIC
                for shift in (0, 1):
                    sv.assert_against_oracle(ops.product(run, o["x_a"], shift), *want["x_a"][:2], terms, want["x_a"][2], what + ", A")
                    assert (want["x_a"][2] == sv.FINITE).all()
            else:
                clean = ops.product(run, o["x"])
                check_y(clean, want["x"][0], want["x"][1], terms)
                for shift in (0, 1):
                    sv.assert_unreferenced(ops.product(run, o["x_a"], shift), clean, what + ", A, shift %d" % shift)
            checks += 1
        for shift in (0, 1):
            sv.assert_against_oracle(ops.product(run, o["x_b"], shift), *want["x_b"][:2], terms, want["x_b"][2],
                                     what + ", B, shift %d" % shift, serial)
        sv.assert_against_oracle(ops.product(run, o["x_c"]), *want["x_c"][:2], terms, want["x_c"][2], what + ", C", serial)
        for z in zeros:
            sv.assert_exact(ops.product(run, z), np.zeros(rows), what + ", D, x = %r everywhere" % z[:1].tolist())
        checks += 3
    print("special values: %s: %d (path, scenario) checks of A ... D" % (name, checks))


@pytest.mark.parametrize("name", sv.STRUCTURES)
def test_scenarios_e_and_f_on_every_path(torch, name):
    """E (subnormals are kept) and F (sums of +-2^1020 that overflow in every order or in none): the oracle's bits."""
    rows, cols, rp, ci, u = sv.structure(name)
    ops = Operands(torch, rows, cols)
    checks = 0
    for scenario, (val, x) in (("E", sv.subnormal(rows, cols, rp, ci)), ("F", sv.overflowing(rows, cols, rp, ci))):
        ref = ob.csr_spmv(rp, ci, val, x)
        if scenario == "E" and int(rp[-1]) >= 100:
            assert np.count_nonzero(ref) > 0 and np.abs(ref).max() < 2.0 ** -1022
        for label, run, serial, kernel in all_paths(rows, cols, rp, ci, val):
            sv.assert_exact(ops.product(run, x), ref, "%s, %s (%s), %s" % (name, label, kernel, scenario))
            checks += 1
    print("special values: %s: %d (path, scenario) checks of E and F" % (name, checks))


@pytest.mark.parametrize("name", sv.STRUCTURES)
def test_scenario_g_on_the_paths_that_promise_the_serial_bits(torch, name):
    """G: products that round.  A kernel built with contraction on (fma) differs from the serial loop in most rows."""
    rows, cols, rp, ci, u = sv.structure(name)
    val, x = sv.rounded(rows, cols, rp, ci)
    sv.assert_regime(name, "G", rows, cols, rp, ci, val, x)
    ref, scale, terms = ob.csr_spmv(rp, ci, val, x), scale_of(rp, ci, val, x), np.diff(rp)
    ops = Operands(torch, rows, cols)
    checks = promised = 0
    for label, run, serial, kernel in csr_paths(rows, cols, rp, ci, val, only_serial=True):
        if not serial.any():
            continue                                                  # (AUTO on another family, column parts)
        sv.assert_against_oracle(ops.product(run, x), ref, scale, terms, np.zeros(rows, int), "%s, %s (%s), G" % (name, label, kernel), serial)
        checks += 1
        promised = max(promised, int(serial.sum()))
    assert checks >= (8 if (terms <= 32).any() else 3), (checks, promised)     # (the sweep's three strip heights promise every row)
    print("special values: %s: %d (path, scenario) checks of G, up to %d rows each" % (name, checks, promised))


# ------------------------------------------------------------------------------------------------------ other entry points
ENTRY_STRUCTURES = ("memplus", "fuzz:1")


def shuffled_coo(rp, ci, val, seed=4):
    coo = sm.make_coo(sv.row_of_entries(rp), ci[:rp[-1]], val[:rp[-1]])
    return coo[np.random.default_rng(seed).permutation(len(coo))]


@pytest.mark.parametrize("name", ENTRY_STRUCTURES)
def test_reference_shaped_entry_points_and_the_repeating_kernel(torch, name):
    """smvp_csr_compute / smvp_tjds_compute with an operand of their own: one product, three, 1500 (two launches of the
    repeating kernel), and 1500 through the fall-back onto one graph launch per product (repeat_patience_us = -1): the bits of
    the one-shot handle, on scenario A's and B's operands."""
    rows, cols, rp, ci, u = sv.structure(name)
    o = sv.ordinary(rows, cols, rp, ci, u)
    coo = sm.make_coo(sv.row_of_entries(rp), ci, o["val"])
    ops = Operands(torch, rows, cols)
    A = sm.CsrMatrix(rows, cols, rp, ci, o["val"])
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, rows, cols))

    def tjds_run(dx, dy):
        T.set_x(dx)
        T.spmv(dy)

    for key in ("x_a", "x_b"):
        ref, scale, cls = ob.csr_spmv(rp, ci, o["val"], o[key]), scale_of(rp, ci, o["val"], o[key]), sv.row_classes(rp, ci, o["val"], o[key])
        for fn, run in ((sm.csr_compute, lambda dx, dy: A.spmv(dx, dy)), (sm.tjds_compute, tjds_run)):
            one_shot = ops.product(run, o[key])
            sv.assert_against_oracle(one_shot, ref, scale, np.diff(rp), cls, "%s, %s, handle" % (name, fn.__name__))
            if key == "x_a":
                sv.assert_unreferenced(one_shot, ops.product(run, o["x"]), "%s, %s, handle" % (name, fn.__name__))
            for iters, patience in ((1, 0), (3, 0), (1500, 0), (1500, -1)):
                y, ms, _ = fn(coo, rows, cols, iters=iters, x=o[key], repeat_patience_us=patience)
                info = sm.last_run_info()
                assert len(ms) == iters
                if iters == 1500 and name == "memplus":                  # (the run of test_repeating_kernel_gives_up_quickly_...)
                    assert (info.repeat_launches, info.repeat_gave_up, info.graph_replays > 0) == ((2, 0, False) if patience == 0 else (0, 1, True))
                sv.check_bits(y, one_shot, "%s, %s, %s, %d products, patience %d" % (name, fn.__name__, key, iters, patience))
    A.close()
    T.close()


def test_a_captured_product_replayed_with_the_operand_poisoned_again(torch):
    """The products recorded into a caller's graph (the pattern of test_products_can_be_captured_in_a_callers_graph), replayed
    with clean x, scenario A's, scenario B's and clean x again: what x holds at the replay is what counts."""
    rows, cols, rp, ci, u = sv.structure("memplus")
    o = sv.ordinary(rows, cols, rp, ci, u)
    val = o["val"]
    A = sm.CsrMatrix(rows, cols, rp, ci, val)
    T = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo(sv.row_of_entries(rp), ci, val), rows, cols))
    dx = torch.zeros(cols, dtype=torch.float64, device="cuda")
    dy = torch.zeros(rows, dtype=torch.float64, device="cuda")
    forms = [("stream", lambda: A.set_kernel(sm.CSR_KERNEL_STREAM, 0), lambda st: A.spmv(dx, dy, stream=st)),
             ("colsweep", lambda: A.set_kernel(sm.CSR_KERNEL_COLSWEEP, 0), lambda st: A.spmv(dx, dy, stream=st)),
             ("binned", lambda: A.set_kernel(sm.CSR_KERNEL_BINNED, 0), lambda st: A.spmv(dx, dy, stream=st)),
             ("vector", lambda: A.set_kernel(sm.CSR_KERNEL_VECTOR, 8), lambda st: A.spmv(dx, dy, stream=st)),
             ("tjds", lambda: None, lambda st: (T.set_x(dx, stream=st), T.spmv(dy, stream=st)))]
    want = {k: (ob.csr_spmv(rp, ci, val, o[k]), scale_of(rp, ci, val, o[k]), sv.row_classes(rp, ci, val, o[k])) for k in ("x", "x_a", "x_b")}
    for form, setup, run in forms:
        setup()
        dx.copy_(torch.from_numpy(o["x"]))
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            run(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                run(s)
        got = {}
        for key in ("x", "x_a", "x_b", "x"):
            dx.copy_(torch.from_numpy(o[key]))
            dy.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            y = dy.cpu().numpy()
            sv.assert_against_oracle(y, *want[key][:2], np.diff(rp), want[key][2], "captured %s, %s" % (form, key))
            sv.check_bits(y, got.setdefault(key, y), "captured %s: clean x after the poisoned ones" % form)
        sv.assert_unreferenced(got["x_a"], got["x"], "captured %s" % form)
        del g
    A.close()
    T.close()


@pytest.mark.parametrize("push", ["copies", "direct"])
@pytest.mark.parametrize("ranks", [2, 8])
def test_sharded_products_carry_non_finite_chunks(torch, ranks, push):
    """ShardedMatrix with virtual ranks on one GPU, both push exchanges, 1 and 3 chunks: a NaN / Inf in a chunk of y arrives
    as such on every rank, scenario A's poison reaches nobody, and the iterate fed back from a poisoned y is the oracle's
    second product by class."""
    exchange = sm.EXCHANGE_COPIES if push == "copies" else sm.EXCHANGE_DIRECT
    for name in ENTRY_STRUCTURES:
        rows, cols, rp, ci, u = sv.structure(name)
        assert rows == cols or name != "memplus"                    # (the iterate needs a square matrix: memplus)
        o = sv.ordinary(rows, cols, rp, ci, u)
        val, terms = o["val"], np.diff(rp)
        coo = sm.make_coo(sv.row_of_entries(rp), ci, val)
        for fmt in ("csr", "tjds"):
            for chunks in (1, 3):
                S = sm.ShardedMatrix(fmt, ranks, rows, cols, coo=coo, csr=(rp, ci, val), devices=[0] * ranks, chunks=chunks, exchange=exchange)
                got = {}
                for key in ("x", "x_a", "x_b"):
                    ref, scale, cls = ob.csr_spmv(rp, ci, val, o[key]), scale_of(rp, ci, val, o[key]), sv.row_classes(rp, ci, val, o[key])
                    S.set_x(o[key])
                    S.spmv(allgather=sm.GATHER_OVERLAPPED)
                    S.synchronize()
                    what = "%s, %s, %d ranks, %s, %d chunks, %s" % (name, fmt, ranks, push, chunks, key)
                    for slot in range(ranks):
                        y = S.get_y(slot, gathered=True)
                        sv.assert_against_oracle(y, ref, scale, terms, cls, what + ", rank %d" % slot)
                        sv.check_bits(y, got.setdefault(key, y), what + ": every rank holds the same vector")
                sv.assert_unreferenced(got["x_a"], got["x"], "%s, %s, %d ranks, %s, %d chunks" % (name, fmt, ranks, push, chunks))
                if rows == cols:                                    # the poisoned y (scenario B's) as the next operand
                    x2 = ob.csr_spmv(rp, ci, val, o["x_b"])
                    S.feed_back(normalize=False)
                    S.spmv(allgather=sm.GATHER_OVERLAPPED)
                    S.synchronize()
                    sv.check_classes(S.get_y(ranks - 1, gathered=True), sv.classes_of(ob.csr_spmv(rp, ci, val, x2)),
                                     "%s, %s, %d ranks, %s, %d chunks: the iterate of a poisoned y" % (name, fmt, ranks, push, chunks))
                    assert (sv.classes_of(x2) != sv.FINITE).sum() >= 10
                S.close()


def test_cli_report_on_a_matrix_with_infinities(torch, tmp_path):
    """The command line on a Matrix Market file whose values include inf, -inf, nan and 0: with its operand of ones the rows
    that hold inf alone, -inf alone, both, or nan print what the oracle's y prints ("%g"; the sign of a NaN is not part of it)."""
    rng = np.random.default_rng(8)
    rows = cols = 60
    entries = []
    for r in range(rows):
        cs = np.sort(rng.choice(cols, int(rng.integers(1, 9)), replace=False))
        vs = ["%.17g" % (k / 64.0) for k in rng.choice([-1, 1], len(cs)) * rng.integers(1, 65, len(cs))]   # (sums exact in any order)
        kind = r % 6
        if kind == 1:
            vs[0] = "inf"
        elif kind == 2:
            vs[-1] = "-inf"
        elif kind == 3 and len(cs) > 1:
            vs[0], vs[-1] = "inf", "-Infinity"
        elif kind == 4:
            vs[0] = "0"
        elif kind == 5 and r % 12 == 5:
            vs[0] = "nan"
        entries += [(r + 1, int(c) + 1, v) for c, v in zip(cs, vs)]
    path = tmp_path / "infinities.mtx"
    path.write_text("%%MatrixMarket matrix coordinate real general\n" + "%d %d %d\n" % (rows, cols, len(entries)) +
                    "".join("%d %d %s\n" % e for e in entries))
    tc, m, n, coo = sm.mm_read_coo(str(path))
    sv.check_bits(coo["val"], np.array([float(v) for _, _, v in entries]), "the reader")
    rp, ci, val = sm.csr_from_coo(coo, m)
    ref = ob.csr_spmv(rp, ci, val, np.ones(n))
    cls = sv.classes_of(ref)
    assert all((cls == c).sum() >= 5 for c in (sv.NAN, sv.PINF, sv.NINF, sv.FINITE))
    want = [t.replace("-nan", "nan") for t in ob.fmt_g(ref)]
    out = tmp_path / "reports"
    os.mkdir(out)
    p = subprocess.run([sm.CLI_PATH, "-c", "-t", "-n", "3", "-d", str(out), str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    files = sorted(os.listdir(out))
    assert len(files) == 2
    for f in files:
        got = [t.replace("-nan", "nan") for t in ob.report_y_lines(open(out / f).read())]
        assert got == want, (f, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5])
