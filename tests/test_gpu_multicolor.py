"""GPU: the multicolour reordering (smvp_csr_color, smvp_perm_from_classes, smvp_csr_create_permuted, smvp_vector_gather; kernel
K23) against tests/coloring_method.py, which test_coloring_host.py pins on the CPU.

No tolerance anywhere.  A colour is the smallest integer no neighbour of larger key holds: one right answer whatever the timing of
the rounds, so d_color equals the restatement's element for element and only `rounds` may vary, inside 1 .. depth.  The permutation
is a stable sort, B's arrays are the host converter's of the mapped entries, a gathered vector is a copy: bits.  The solvers did
not change, so on B they give the bits of their own restatements run on B's arrays."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import bicgstab_method as bi
import cg_method as cg
import coloring_method as cm
import gmres_method as gm
import ilu0_method as ilu
import pbicgstab_method as pb
import pcg_tri_method as tri
import smvp_toolkit_amd as sm
import test_gpu_gmres as k19
import test_gpu_pbicgstab as k18
import test_gpu_pcg_tri as k16
import trsv_method as trsv
from conftest import ROOT
from parity import check_guards, guarded_y
from test_gpu_transposed import arrays_of, assert_arrays, inner_csr_handle
from transposed import assert_bits

pytestmark = pytest.mark.gpu

PKG = os.path.join(ROOT, "smvp-toolkit_amd")
COUNTED = os.path.join(PKG, "lib", "libsmvp_amd_counted.so")
LIMIT_S = 240
TOL = 1e-8


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def ints(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def handles(P, at):
    A = sm.CsrMatrix(P.n, P.n, *P.csr)
    return A, (A.transposed() if at else None)


def colored(torch, A, At, n, seed, stream=None, max_rounds=4096):
    """(colours, info) of one call into a guarded buffer of sentinels."""
    buf = torch.full((n + 64,), -77, dtype=torch.int32, device="cuda")
    out = buf[32:32 + n]
    info = A.color(out, At, seed, max_rounds, stream)
    got = buf.cpu().numpy()
    assert (got[:32] == -77).all() and (got[32 + n:] == -77).all(), "smvp_csr_color wrote outside d_color"
    return got[32:32 + n].copy(), info


def held(P, at, seed, col, info, what):
    want, colors, depth = P.reference(at, seed)
    bad = np.flatnonzero(col != want)
    assert not len(bad), "%s: %d of %d colours differ; first at vertex %d: %d against %d" % (what, len(bad), P.n, bad[0], col[bad[0]], want[bad[0]])
    assert info["colors"] == colors and 1 <= info["rounds"] <= depth, "%s: %r; the restatement has %d colours, depth %d" % (what, info, colors, depth)
    sizes = np.bincount(want, minlength=colors)
    assert (info["largest_class"], info["smallest_class"]) == (int(sizes.max()), int(sizes.min())), what
    assert info["entries"] == P.nnz * (2 if at else 1) and info["lanes_per_row"] in (2, 4, 8, 16, 32, 64) and info["build_ms"] >= 0.0, what


# ============================================================================================================== 1. the colouring
@pytest.mark.parametrize("seed", cm.SEEDS)
def test_the_colours_are_the_restatements_on_the_constructed_cases(torch, seed):
    for P, _ in cm.small_cases():
        for at in (False, True):
            A, At = handles(P, at)
            col, info = colored(torch, A, At, P.n, seed)
            held(P, at, seed, col, info, "%s, at %s, seed %#x" % (P.name, at, seed))
            for H in (At, A):
                if H is not None:
                    H.close()


@pytest.mark.parametrize("name", cm.SAMPLES)
def test_the_colours_are_the_restatements_on_the_samples(torch, name):
    P = cm.sample(name)
    lanes = set()
    for at in (False, True):
        A, At = handles(P, at)
        for seed in cm.SEEDS:
            col, info = colored(torch, A, At, P.n, seed)
            held(P, at, seed, col, info, "%s, at %s, seed %#x" % (name, at, seed))
            lanes.add(info["lanes_per_row"])
            print("%-8s at %-5s seed %#10x: %3d colours in %3d rounds (depth %3d), %d lanes per row, classes of %d .. %d rows, %.2f ms" % (
                name, at, seed, info["colors"], info["rounds"], P.reference(at, seed)[2], info["lanes_per_row"], info["smallest_class"],
                info["largest_class"], info["build_ms"]))
        for H in (At, A):
            if H is not None:
                H.close()
    if name == "memplus":
        assert max(lanes) >= 8, "memplus's 574-entry row should get more than a few lanes"    # several strides AND several windows


def test_a_callers_stream_twice_on_one_handle_and_the_handles_product_stays(torch):
    P = cm.sample("memplus")
    A, At = handles(P, True)
    x = dev(torch, cg.rhs(P.n))
    y0, y1 = (torch.empty(P.n, dtype=torch.float64, device="cuda") for _ in range(2))
    z0, z1 = (torch.empty(P.n, dtype=torch.float64, device="cuda") for _ in range(2))
    A.spmv(x, y0)
    At.spmv(x, z0)
    torch.cuda.synchronize()
    kernels = A.describe()[0], At.describe()[0]
    s = torch.cuda.Stream()
    for seed in (1, 1, 0):
        col, info = colored(torch, A, At, P.n, seed, stream=s)
        held(P, True, seed, col, info, "memplus on a stream of the caller's, seed %d" % seed)
    assert (A.describe()[0], At.describe()[0]) == kernels
    A.spmv(x, y1)
    At.spmv(x, z1)
    torch.cuda.synchronize()
    assert_bits(y1.cpu().numpy(), y0.cpu().numpy(), "A x after the colourings")
    assert_bits(z1.cpu().numpy(), z0.cpu().numpy(), "A^T x after the colourings")
    At.close()
    A.close()


def test_past_the_round_kernels_first_grid_trip(torch):
    """The grid is capped (plan option color_max_blocks, default 2048 workgroups of 256 threads): with the cap at 3 a banded matrix of
    5000 rows takes many trips; with the default cap a size past 2048 * 256 / lanes_per_row takes a second one.  Checked against
    smvp_csr_color_host, which test_coloring_host.py holds to the restatement."""
    P = cm.banded(5000, 3)
    A, _ = handles(P, False)
    with sm.option("color_max_blocks", 3):
        col, info = colored(torch, A, None, P.n, 1)
    want, colors, depth = sm.color_host(P.n, P.csr[0], P.csr[1], seed=1)
    assert (col == want).all() and info["colors"] == colors and 1 <= info["rounds"] <= depth
    assert 3 * 256 // info["lanes_per_row"] < P.n
    A.close()
    lanes = info["lanes_per_row"]
    n = 2048 * 256 // lanes + 1000
    P = cm.banded(n, 3)
    A, _ = handles(P, False)
    col, info = colored(torch, A, None, P.n, 0)
    assert info["lanes_per_row"] == lanes and 2048 * 256 // lanes < n
    want, colors, depth = sm.color_host(P.n, P.csr[0], P.csr[1], seed=0)
    assert (col == want).all() and info["colors"] == colors and 1 <= info["rounds"] <= depth
    assert (col[-2000:] >= 0).all()
    A.close()


def color_status(torch, h, ht, n, opts="default", color="own", info="own", stream=None):
    """The status of one raw call; a refused call must leave d_color and *info as they were."""
    d = torch.full((max(n, 1),), -77, dtype=torch.int32, device="cuda") if color == "own" else color
    i = sm.ColorInfo()
    C.memset(C.byref(i), 0x5a, C.sizeof(i))
    i.struct_size = C.sizeof(sm.ColorInfo) if info == "own" else info
    before = bytes(i)
    if opts == "default":
        opts = sm.ColorOpts()
        sm.lib().smvp_color_opts_default(C.byref(opts))
    rc = sm.lib().smvp_csr_color(h, ht, C.byref(opts) if opts is not None else None, sm._dev_ptr(d), C.byref(i), sm._stream_ptr(stream))
    if rc != sm.OK and stream is None:
        torch.cuda.synchronize()
        assert bytes(i) == before, "a refused call wrote *info"
        if d is not None and not (rc == sm.ERR_UNSUPPORTED and b"max_rounds" in sm.lib().smvp_last_error()):
            assert (d.cpu().numpy() == -77).all(), "a refused call wrote d_color"
    return rc


def test_max_rounds_and_every_refusal(torch):
    P = cm.path(301)
    A, At = handles(P, True)
    n = P.n
    err = sm.lib().smvp_last_error
    o = sm.ColorOpts()
    sm.lib().smvp_color_opts_default(C.byref(o))
    o.max_rounds = 1
    assert P.reference(False, 0)[2] > 1
    assert color_status(torch, A._h, None, n, o) == sm.ERR_UNSUPPORTED and b"max_rounds" in err()
    assert color_status(torch, A._h, None, n, None) == sm.OK                     # NULL opts: the defaults
    assert color_status(torch, None, None, n) == sm.ERR_INVALID and b"handle" in err()
    assert color_status(torch, A._h, None, n, color=None) == sm.ERR_INVALID and b"d_color" in err()
    o.max_rounds = 0
    assert color_status(torch, A._h, None, n, o) == sm.ERR_INVALID and b"max_rounds" in err()
    o.max_rounds, o.struct_size = 5, 8
    assert color_status(torch, A._h, None, n, o) == sm.ERR_INVALID and b"struct_size" in err()
    assert color_status(torch, A._h, None, n, info=16) == sm.ERR_INVALID and b"struct_size" in err()
    Q = cm.path(300)
    Bq, _ = handles(Q, False)
    assert color_status(torch, A._h, Bq._h, n) == sm.ERR_INVALID and b"ht" in err()
    rect = sm.CsrMatrix(2, 3, np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.ones(2))
    assert color_status(torch, rect._h, None, 2) == sm.ERR_INVALID and b"square" in err()
    block = sm.CsrMatrix(P.n, P.n, *P.csr, first_row=5)
    assert color_status(torch, block._h, None, n) == sm.ERR_UNSUPPORTED and b"row block" in err()
    assert color_status(torch, A._h, block._h, n) == sm.ERR_UNSUPPORTED and b"row block" in err()
    M = tri.lap2d(8)
    T = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
    inner = inner_csr_handle(T, M.n, M.n, M.nnz)
    L8, _ = handles(cm.lap2d(8), False)
    assert color_status(torch, inner, None, M.n) == sm.ERR_UNSUPPORTED and b"plain CSR" in err()
    assert color_status(torch, L8._h, inner, M.n) == sm.ERR_UNSUPPORTED and b"plain CSR" in err()
    E = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    info = E.color(torch.empty(0, dtype=torch.int32, device="cuda"))
    assert (info["colors"], info["rounds"], info["largest_class"], info["smallest_class"], info["entries"]) == (0, 0, 0, 0, 0)
    for H in (E, L8, T, block, rect, Bq, At, A):
        H.close()


def test_a_capturing_stream_is_refused_by_the_three_calls_that_wait_and_the_capture_stays_valid(torch):
    P = cm.lap2d(8)
    A, _ = handles(P, False)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    d = torch.full((P.n,), -77, dtype=torch.int32, device="cuda")
    ident = ints(torch, np.arange(P.n))
    o1, o2 = (torch.full((P.n,), -77, dtype=torch.int32, device="cuda") for _ in range(2))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    got, msgs, out = [], [], C.c_void_p(0x1234)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)
            got.append(color_status(torch, A._h, None, P.n, color=d, stream=s))
            msgs.append(sm.lib().smvp_last_error().decode())
            got.append(sm.lib().smvp_perm_from_classes(0, P.n, 4, sm._dev_ptr(ident), sm._dev_ptr(o1), sm._dev_ptr(o2), None, s.cuda_stream))
            msgs.append(sm.lib().smvp_last_error().decode())
            got.append(sm.lib().smvp_csr_create_permuted(C.byref(out), A._h, sm._dev_ptr(ident), s.cuda_stream))
            msgs.append(sm.lib().smvp_last_error().decode())
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] * 3 and all("captur" in m for m in msgs) and not out.value
    g.replay()
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16
    for t in (d, o1, o2):
        assert (t.cpu().numpy() == -77).all()
    del g
    col, info = colored(torch, A, None, P.n, 0, stream=s)
    held(P, False, 0, col, info, "outside a capture the same stream is fine")
    A.close()


# ================================================================================================= 2. the permutation and the handle
def test_perm_from_classes_is_a_stable_argsort_with_empty_classes_too(torch):
    rng = np.random.default_rng(20232)
    s = torch.cuda.Stream()
    for n, k, used in ((1, 1, [0]), (5000, 7, [0, 2, 3, 6]), (70001, 300, list(range(0, 300, 2))), (2049, 1, [0]), (4097, 70000, [69999, 3])):
        classes = rng.choice(np.array(used), n).astype(np.int32)
        for stream in (None, s):
            got = sm.perm_from_classes(ints(torch, classes), k, stream)
            want = cm.perm_from_classes(classes, k)
            for g, w, name in zip(got, want, ("old_of_new", "new_of_old", "class_ptr")):
                g = g.cpu().numpy() if name != "class_ptr" else g
                assert g.dtype == np.int32 and (g == w).all(), "n = %d, %d classes: %s differs" % (n, k, name)
    o, p, ptr = sm.perm_from_classes(torch.empty(0, dtype=torch.int32, device="cuda"), 3)
    assert o.numel() == p.numel() == 0 and ptr.tolist() == [0, 0, 0, 0]
    # refused: a class out of range (found before anything indexes with it, nothing written), no class at all, bad sizes
    o1, o2 = (torch.full((100,), -77, dtype=torch.int32, device="cuda") for _ in range(2))
    ptr = np.full(5, -77, np.int32)
    for bad in (4, -1, 2 ** 31 - 1):
        classes = np.arange(100, dtype=np.int32) % 4
        classes[37] = bad
        rc = sm.lib().smvp_perm_from_classes(0, 100, 4, sm._dev_ptr(ints(torch, classes)), sm._dev_ptr(o1), sm._dev_ptr(o2), sm._p(ptr), None)
        assert rc == sm.ERR_INVALID and b"d_class[37]" in sm.lib().smvp_last_error()
        assert (o1.cpu().numpy() == -77).all() and (o2.cpu().numpy() == -77).all() and (ptr == -77).all()
    d = ints(torch, np.zeros(100))
    L = sm.lib().smvp_perm_from_classes
    assert L(0, 100, 0, sm._dev_ptr(d), sm._dev_ptr(o1), sm._dev_ptr(o2), None, None) == sm.ERR_INVALID
    assert L(0, -1, 4, sm._dev_ptr(d), sm._dev_ptr(o1), sm._dev_ptr(o2), None, None) == sm.ERR_INVALID
    assert L(0, 100, -1, sm._dev_ptr(d), sm._dev_ptr(o1), sm._dev_ptr(o2), None, None) == sm.ERR_INVALID
    assert L(0, 100, 4, None, sm._dev_ptr(o1), sm._dev_ptr(o2), None, None) == sm.ERR_INVALID
    assert L(0, 100, 4, sm._dev_ptr(d), None, sm._dev_ptr(o2), None, None) == sm.ERR_INVALID
    assert L(0, 100, 4, sm._dev_ptr(d), sm._dev_ptr(o1), None, None, None) == sm.ERR_INVALID
    assert (o1.cpu().numpy() == -77).all() and (o2.cpu().numpy() == -77).all()


def test_the_permuted_handle_is_the_host_converter_on_the_mapped_entries(torch):
    rng = np.random.default_rng(20233)
    s = torch.cuda.Stream()
    for P in (cm.messy(), cm.lap2d(32), cm.sample("ibm32"), cm.sample("memplus")):
        A, _ = handles(P, False)
        for kind, stream in (("random", None), ("identity", s)):
            p = rng.permutation(P.n).astype(np.int32) if kind == "random" else np.arange(P.n, dtype=np.int32)
            B = A.permuted(ints(torch, p), stream)
            want = cm.permuted_csr(P.n, *P.csr, p)
            assert_arrays(arrays_of(torch, B), want, "%s, %s permutation" % (P.name, kind))
            assert (B.rows, B.cols, B.nnz) == (P.n, P.n, P.nnz) and B.get_kernel()[0] != sm.CSR_KERNEL_AUTO
            if kind == "identity" and P.name.startswith("lap2d"):
                assert_arrays(arrays_of(torch, B), P.csr, "the identity gives A's arrays where A's columns ascend")
            # B is a handle of its own: its product is the serial loop over its arrays, and it outlives A
            x = cg.rhs(P.n, 3)
            buf, y = guarded_y(torch, P.n)
            B.spmv(dev(torch, x), y)
            torch.cuda.synchronize()
            check_guards(buf, P.n)
            import oracle_binding as ob
            ref, scale = ob.csr_spmv(*want, x), ob.csr_spmv(want[0], want[1], np.abs(want[2]), np.abs(x))
            assert (np.abs(y.cpu().numpy() - ref) <= 1e-13 * scale).all()
            B.close()
        A.close()
    E = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    B = E.permuted(torch.empty(0, dtype=torch.int32, device="cuda"))
    assert (B.rows, B.nnz) == (0, 0)
    B.close()
    E.close()


def test_a_wrong_permutation_or_handle_is_refused_and_nothing_is_built(torch):
    P = cm.lap2d(32)
    A, _ = handles(P, False)
    err = sm.lib().smvp_last_error

    def status(h, p):
        out = C.c_void_p(0x1234)
        rc = sm.lib().smvp_csr_create_permuted(C.byref(out), h, sm._dev_ptr(p), None)
        assert rc == sm.OK or not out.value, "*out is not NULL after a failure"
        if rc == sm.OK:
            sm.lib().smvp_csr_destroy(out)
        return rc

    good = np.random.default_rng(1).permutation(P.n).astype(np.int32)
    assert status(A._h, ints(torch, good)) == sm.OK
    for at, value in ((5, int(good[6])), (0, -1), (P.n - 1, P.n), (17, 2 ** 31 - 1), (900, -2 ** 31)):
        bad = good.copy()
        bad[at] = value
        assert status(A._h, ints(torch, bad)) == sm.ERR_INVALID and b"no permutation" in err(), (at, value)
    assert status(A._h, ints(torch, np.zeros(P.n))) == sm.ERR_INVALID
    assert status(None, ints(torch, good)) == sm.ERR_INVALID and status(A._h, None) == sm.ERR_INVALID
    assert sm.lib().smvp_csr_create_permuted(None, A._h, sm._dev_ptr(ints(torch, good)), None) == sm.ERR_INVALID
    M = tri.lap2d(32)
    T = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
    assert status(inner_csr_handle(T, M.n, M.n, M.nnz), ints(torch, good)) == sm.ERR_UNSUPPORTED and b"plain CSR" in err()
    block = sm.CsrMatrix(P.n, P.n, *P.csr, first_row=3)
    assert status(block._h, ints(torch, good)) == sm.ERR_UNSUPPORTED and b"row block" in err()
    rect = sm.CsrMatrix(2, 3, np.array([0, 1, 2], np.int32), np.array([0, 2], np.int32), np.ones(2))
    assert status(rect._h, ints(torch, [0, 1])) == sm.ERR_INVALID and b"square" in err()
    for H in (rect, block, T, A):
        H.close()


def test_vector_gather_there_and_back_every_bit(torch):
    n = 70001
    rng = np.random.default_rng(20234)
    x = rng.standard_normal(n)
    x[:8] = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1.0, -1.0]
    x.view(np.uint64)[8:12] = [0x7ff8000000000001, 0xfff8000000000abc, 0x7ff0000000000001, 0xfff4000000000000]   # NaN payloads, quiet and signalling
    p = rng.permutation(n).astype(np.int32)
    inv = np.empty(n, np.int32)
    inv[p] = np.arange(n, dtype=np.int32)
    dx, dp, dinv = dev(torch, x), ints(torch, p), ints(torch, inv)
    buf, y = guarded_y(torch, n)
    s = torch.cuda.Stream()
    sm.vector_gather(dp, dx, y, s)
    s.synchronize()
    check_guards(buf, n)
    assert y.cpu().numpy().view(np.uint64).tolist() == x[p].view(np.uint64).tolist()
    z = torch.empty(n, dtype=torch.float64, device="cuda")
    sm.vector_gather(dinv, y, z)
    torch.cuda.synchronize()
    assert z.cpu().numpy().tobytes() == x.tobytes()
    # an index out of range is not followed: a quiet NaN there, everything else as before, no fault
    bad = p.copy()
    bad[[0, 100, n - 1]] = [-1, n, 2 ** 31 - 1]
    sm.vector_gather(ints(torch, bad), dx, y)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert got.view(np.uint64)[[0, 100, n - 1]].tolist() == [0x7ff8000000000000] * 3
    keep = np.ones(n, bool)
    keep[[0, 100, n - 1]] = False
    assert got[keep].tobytes() == x[p][keep].tobytes()
    # refused: overlap, null arrays, n < 0
    L, P_ = sm.lib().smvp_vector_gather, sm._dev_ptr
    assert L(0, n, P_(dp), P_(dx), P_(dx), None) == sm.ERR_INVALID and b"overlap" in sm.lib().smvp_last_error()
    assert L(0, n - 1, P_(dp), P_(dx), C.c_void_p(dx.data_ptr() + 8), None) == sm.ERR_INVALID
    assert L(0, n, None, P_(dx), P_(y), None) == sm.ERR_INVALID and L(0, n, P_(dp), None, P_(y), None) == sm.ERR_INVALID
    assert L(0, n, P_(dp), P_(dx), None, None) == sm.ERR_INVALID and L(0, -1, P_(dp), P_(dx), P_(y), None) == sm.ERR_INVALID
    assert L(0, 0, None, None, None, None) == sm.OK
    torch.cuda.synchronize()
    assert dx.cpu().numpy().tobytes() == x.tobytes()


# ================================================================================================================ 3. end to end
class OnB:
    """What test_gpu_pcg_tri / _pbicgstab / _gmres.solve ask of their plans: first, second, m and the restatement's triples."""

    def __init__(self, first, m, second, triples):
        self.first, self.m, self.second, self.triples = first, m, second, triples

    def close(self):
        self.first.close()
        self.second.close()


def product_of(torch, H, n):
    seen = {}

    def product(x):
        key = np.ascontiguousarray(x, dtype=np.float64).tobytes()
        if key not in seen:
            buf, dy = guarded_y(torch, n)
            H.spmv(dev(torch, x), dy)
            torch.cuda.synchronize()
            check_guards(buf, n)
            seen[key] = dy.cpu().numpy()
        return seen[key].copy()
    return product


def natural_steps(torch, A, n, b, solver):
    """Steps to tol of the library's solver on A in its natural order with ILU(0) and SGS: printed beside the multicolour ones."""
    out = {}
    f = A.ilu0()
    for kind in ("ilu0", "sgs"):
        if kind == "ilu0":
            first, second, m = *f.plans(), None
        else:
            first, second = A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER)
            m = A.diagonal(torch.empty(n, dtype=torch.float64, device="cuda"))
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        r = getattr(A, solver)(dev(torch, b), x, first, second, m, max_steps=400, tol=TOL)[0]
        out[kind] = (r.steps, first.info()["levels"], second.info()["levels"])
        first.close()
        second.close()
    f.close()
    return out


@pytest.mark.parametrize("name", ["lap2d(32)", "convdiff(32, 0.5)"])
def test_plans_factor_and_solvers_on_the_reordered_matrix(torch, name):
    M = tri.lap2d(32) if name.startswith("lap2d") else pb.convdiff(32, 0.5)
    n = M.n
    A = sm.CsrMatrix(n, n, *M.csr)
    R = A.multicolored()
    P = cm.of_matrix(name, M)
    want_col, colors, _ = P.reference(False, 0)
    assert R.colors == colors == R.info["colors"] and len(R.color_ptr) == colors + 1
    want_perm = cm.perm_from_classes(want_col, colors)
    for got, want in zip((R.old_of_new.cpu().numpy(), R.new_of_old.cpu().numpy(), R.color_ptr), want_perm):
        assert (got == want).all()
    Bcsr = cm.permuted_csr(n, *M.csr, want_perm[1])
    assert_arrays(arrays_of(torch, R.matrix), Bcsr, name + ": B's arrays")
    Cs = trsv.Case.of_csr("B of " + name, n, *Bcsr)
    # vectors there and back
    b = bi.rhs(n)
    db, dbn, dback = dev(torch, b), torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    R.to_new(db, dbn)
    R.to_old(dbn, dback)
    torch.cuda.synchronize()
    bn = dbn.cpu().numpy()
    assert bn.tobytes() == b[want_perm[0]].tobytes() and dback.cpu().numpy().tobytes() == b.tobytes()
    # the factor and the plans: at most `colors` levels each
    f = R.matrix.ilu0()
    assert_bits(arrays_of(torch, f.matrix)[2], sm.ilu0_host(n, *Bcsr), name + ": the ILU(0) of B")
    assert_bits(arrays_of(torch, f.matrix)[2], ilu.factor(Cs).csr[2], name + ": the ILU(0) of B against the restatement")
    assert f.info()["levels"] <= colors
    L, U = f.plans()
    sl, su = R.matrix.trsv_plan(sm.TRSV_LOWER), R.matrix.trsv_plan(sm.TRSV_UPPER)
    for T in (L, U, sl, su):
        assert T.info()["levels"] <= colors, "%s: %d levels with %d colours" % (name, T.info()["levels"], colors)
    sgs = tri.sgs(Cs)
    m_dev = R.matrix.diagonal(torch.empty(n, dtype=torch.float64, device="cuda")).cpu().numpy()
    assert_bits(m_dev, sgs[1], "diagonal() of B")
    plans = {"ilu0": OnB(L, None, U, ilu.plans(ilu.factor(Cs))), "sgs": OnB(sl, sgs[1], su, sgs)}
    product = product_of(torch, R.matrix, n)
    steps = {}
    for kind, Pl in plans.items():
        if name.startswith("lap2d"):
            got = k16.solve(torch, R.matrix, n, bn, Pl, None, 200, TOL)
            k16.same(got, tri.run(product, bn, None, *Pl.triples, 200, TOL), "%s, pcg_tri with %s on B" % (name, kind), bn)
            steps[("pcg_tri", kind)] = got[0]
            assert got[2] == cg.CONVERGED
        got = k18.solve(torch, R.matrix, n, bn, Pl, None, 200, TOL)
        k18.same(got, pb.run(product, bn, None, *Pl.triples, 200, TOL), "%s, pbicgstab with %s on B" % (name, kind), bn)
        steps[("pbicgstab", kind)] = got[0]
        assert got[3] == pb.CONVERGED
        got = k19.solve(torch, R.matrix, n, bn, Pl, None, 30, 300, TOL)
        k19.same(got, gm.run_rr(product, bn, None, *Pl.triples, 30, 300, TOL), "%s, gmres with %s on B" % (name, kind), bn)
        steps[("gmres", kind)] = got[0]
        assert got[3] == gm.CONVERGED
        # x in A's numbering is numpy's fancy indexing of x', and it solves A x = b
        xo = torch.empty(n, dtype=torch.float64, device="cuda")
        R.to_old(dev(torch, got[6]), xo)
        torch.cuda.synchronize()
        x = xo.cpu().numpy()
        assert x.tobytes() == got[6][want_perm[1]].tobytes()
        assert np.linalg.norm(M.spmv(x) - b) <= 10 * TOL * np.linalg.norm(b)
    for solver in ("pcg_tri", "pbicgstab", "gmres"):
        if solver == "pcg_tri" and not name.startswith("lap2d"):
            continue
        nat = natural_steps(torch, A, n, b, solver)
        for kind in ("ilu0", "sgs"):
            print("%-18s %-9s %-4s steps to %g: natural %3d (levels %d / %d), multicolour %3d (%d colours)" % (
                name, solver, kind, TOL, nat[kind][0], nat[kind][1], nat[kind][2], steps[(solver, kind)], colors))
    for Pl in plans.values():
        Pl.close()
    f.close()
    R.close()
    A.close()


def test_a_capture_of_to_new_solve_to_old_replays(torch):
    M = tri.lap2d(32)
    n = M.n
    A = sm.CsrMatrix(n, n, *M.csr)
    R = A.multicolored()
    T = R.matrix.trsv_plan(sm.TRSV_LOWER)
    b = dev(torch, bi.rhs(n))
    bn, xn, x = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(3))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            R.to_new(b, bn, s)
            T.solve(bn, xn, s)
            R.to_old(xn, x, s)
    wants = []
    for seed in (15, 16):
        rhs = trsv.rhs(n, seed)
        b.copy_(torch.from_numpy(rhs))
        x.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        Cs = trsv.Case.of_csr("B", n, *arrays_of(torch, R.matrix))
        p, q = R.old_of_new.cpu().numpy(), R.new_of_old.cpu().numpy()
        want = trsv.solve(Cs, trsv.LOWER, trsv.STORED, rhs[p])[q]
        assert_bits(x.cpu().numpy(), want, "the replayed capture, right-hand side %d" % seed)
        wants.append(want)
    assert wants[0].tobytes() != wants[1].tobytes()
    del g
    T.close()
    R.close()
    A.close()


# ================================================================================ 4. resources and fresh memory, in a child process
SCRIPT = os.path.join(ROOT, "tests", "multicolor_scenarios.py")
_crashed = []


@pytest.mark.parametrize("group", ["resources", "fresh"])
def test_the_calls_give_back_what_they_took_and_read_no_fresh_memory(group):
    """tests/multicolor_scenarios.py against lib/libsmvp_amd_counted.so, one child per group under one time limit, nothing retried:
    every new call balances exactly, every device allocation refused in turn gives an error and holds nothing, and under
    test_gpu_fresh_memory.py's fill patterns the colours, B and the gathered vectors are the same."""
    assert not _crashed, "not started: the group %r ended in a crash or at its time limit" % _crashed[0]
    if not os.path.exists(COUNTED):
        subprocess.check_call(["make", "-C", PKG, "lib/libsmvp_amd_counted.so"])
    env = dict(os.environ, SMVP_LIB_PATH=COUNTED)
    try:
        p = subprocess.run([sys.executable, SCRIPT, group], env=env, capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _crashed.append(group)
        seen = e.stdout or ""
        seen = seen.decode(errors="replace") if isinstance(seen, bytes) else seen
        raise AssertionError("group %s did not finish in %d s\n%s" % (group, LIMIT_S, seen[-3000:]))
    if p.returncode not in (0, 1, 2):
        _crashed.append(group)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and ("group %s ok" % group) in p.stdout, \
        "group %s: exit status %d\n%s\n%s" % (group, p.returncode, p.stdout[-6000:], p.stderr[-3000:])
