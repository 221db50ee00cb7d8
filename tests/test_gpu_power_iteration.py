"""GPU: power iteration (iterate / normalize, smvp_sharded_feed_back) step by step on every path, ranks included
(tests/power_iteration.py has the normalisation, the host chain, the matrices and the start vectors;
test_power_iteration_host.py pins them to the oracle and shows that every regime occurs).

Three checks, none with a tolerance of its own:
 1. the loop adds nothing to the products: k iterated steps through an entry point are bit for bit the host chain -- a handle
    made the way the entry point makes it, one product, normalise() in numpy, the result uploaded as the next operand, k times
    -- on every path whose product is reproducible from run to run (every CSR family, TJDS ROW_GATHER and TWO_PHASE, every
    sharded form);
 2. every product of the chain is right: parity.check_y against the oracle on the operand it was actually given;
 3. the normalisation is a pure function: a maximum is exact in any order, an IEEE division correctly rounded, so the device
    has numpy's bits -- at a peak in every position of the absmax grid (its second trip included), on a negative, NaN,
    infinite, zero and subnormal maximum.
TJDS ATOMIC, whose order of summation varies, runs on integers for which every order is exact.  Comparisons are
transposed.assert_bits (any NaN equals any NaN); products the test runs itself write into a guarded y."""
import ctypes as C
import functools

import numpy as np
import pytest

import power_iteration as pi
import smvp_toolkit_amd as sm
from parity import check_guards, check_y, guarded_y
from test_gpu_parity import CSR_VARIANTS, TJDS_MODES
from transposed import assert_bits

pytestmark = pytest.mark.gpu

AUTO = (sm.CSR_KERNEL_AUTO, 0)
CSR_PATHS = [AUTO] + CSR_VARIANTS
REPRODUCIBLE_TJDS = [m for m in TJDS_MODES if m != sm.TJDS_MODE_ATOMIC]
ORDINARY = ("short", "long", "shuffled")
PEAKS = [(n, p, s) for n, ps in (pi.PEAK_SMALL, pi.PEAK_LARGE) for p in ps for s in (1, -1)]
EXCHANGES = {"copies": sm.EXCHANGE_COPIES, "direct": sm.EXCHANGE_DIRECT}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def matrix(name, *args):
    """The matrices of power_iteration.py, built once and left unchanged."""
    return getattr(pi, name)(*args)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


# ------------------------------------------------------------------------------------------- one handle's product, numpy to numpy
def csr_product(torch, M, kernel=sm.CSR_KERNEL_AUTO, param=0):
    """(handle, product) of a CsrMatrix set up as smvp_csr_compute sets its own up: the host converter's arrays, set_kernel only
    where a kernel or a parameter is named."""
    A = sm.CsrMatrix(M.n, M.n, *M.csr)
    if (kernel, param) != AUTO:
        A.set_kernel(kernel, param)

    def product(x):
        dx = dev(torch, x)
        buf, dy = guarded_y(torch, M.n)
        A.spmv(dx, dy)
        torch.cuda.synchronize()
        check_guards(buf, M.n)
        return dy.cpu().numpy()

    return A, product


def tjds_product(torch, M, mode=sm.TJDS_MODE_AUTO):
    """(handle, product) of a TjdsMatrix set up as smvp_tjds_compute sets its own up; every product takes its operand by set_x."""
    T = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
    if mode != sm.TJDS_MODE_AUTO:
        T.set_mode(mode)

    def product(x):
        dx = dev(torch, x)
        buf, dy = guarded_y(torch, M.n)
        T.set_x(dx)
        T.zero_y(dy)
        T.spmv(dy)
        torch.cuda.synchronize()
        check_guards(buf, M.n)
        return dy.cpu().numpy()

    return T, product


def checked_chain(M, product, x0, steps, normalize, what):
    """The host chain over `product`, every raw product of it within check_y of the oracle's on the operand it was given."""
    raw, its = pi.host_chain(product, x0, steps, normalize)
    for k, (x, y) in enumerate(zip(pi.operands(x0, its), raw)):
        try:
            check_y(y, M.spmv(x), M.scale(x), M.terms)
        except AssertionError as e:
            raise AssertionError("%s, product %d of the chain: %s" % (what, k + 1, e)) from None
    return raw, its


def compute(fmt, M, steps, normalize, x=None, **kw):
    """smvp_csr_compute / smvp_tjds_compute with iterate -> the last iterate; one time per step, every one of them measured."""
    fn = sm.csr_compute if fmt == "csr" else sm.tjds_compute
    y, ms, st = fn(M.coo, M.n, M.n, iters=steps, x=x, iterate=True, normalize=normalize, **kw)
    assert len(ms) == steps and (ms > 0).all(), "one time per step: %d for %d steps, %d of them not positive" % (len(ms), steps, (ms <= 0).sum())
    return y


def start_vectors(M):
    """(label, the vector, what the entry point is given for it)."""
    x = pi.random_x(M)
    return (("ones", pi.ones(M), None), ("random x", x, x))


def assert_owner_plan(A, M):
    """AUTO chose the owner form of the tile kernel and no row has more than 32 entries: the serial loop's bits are promised."""
    name = A.describe()[0]
    assert name.startswith("csr_stream_owner<") and M.terms.max() <= 32, (name, M.terms.max())


# ================================================================================== 1. one GPU: entry points against the chain
@pytest.mark.parametrize("kernel,param", CSR_PATHS)
@pytest.mark.parametrize("name", ORDINARY)
def test_csr_iteration_is_the_chain_of_the_handles_products(torch, name, kernel, param):
    M = matrix(name)
    A, product = csr_product(torch, M, kernel, param)
    for label, x0, x_arg in start_vectors(M):
        for normalize in (False, True):
            what = "%s, kernel %d param %d, %s, normalize %s" % (name, kernel, param, label, normalize)
            raw, its = checked_chain(M, product, x0, max(pi.STEPS), normalize, what)
            for steps in pi.STEPS:
                y = compute("csr", M, steps, normalize, x_arg, kernel=kernel, param=param)
                assert_bits(y, its[steps - 1], "%s, %d steps" % (what, steps))
                if name == "short" and (kernel, param) == AUTO:          # ... and the oracle's own iteration
                    assert_owner_plan(A, M)
                    assert_bits(y, M.iterate(x0, steps, normalize), "%s, %d steps, the oracle's iteration" % (what, steps))
            if (kernel, param) == AUTO and normalize and x_arg is not None:  # the arrays built on the device: the same bits
                y = compute("csr", M, 3, True, x_arg, device_convert=True)
                assert_bits(y, its[2], "%s, converted on the device" % what)
    A.close()


@pytest.mark.parametrize("mode", REPRODUCIBLE_TJDS)
@pytest.mark.parametrize("name", ORDINARY)
def test_tjds_iteration_is_the_chain_of_the_handles_products(torch, name, mode):
    M = matrix(name)
    T, product = tjds_product(torch, M, mode)
    for label, x0, x_arg in start_vectors(M):
        for normalize in (False, True):
            what = "%s, TJDS mode %d, %s, normalize %s" % (name, mode, label, normalize)
            raw, its = checked_chain(M, product, x0, max(pi.STEPS), normalize, what)
            for steps in pi.STEPS:
                assert_bits(compute("tjds", M, steps, normalize, x_arg, mode=mode), its[steps - 1], "%s, %d steps" % (what, steps))
            if mode == sm.TJDS_MODE_ROW_GATHER and normalize and x_arg is not None:
                y = compute("tjds", M, 3, True, x_arg, mode=mode, device_convert=True)
                assert_bits(y, its[2], "%s, converted on the device" % what)
    T.close()


# =================================================================================================== 2. TJDS ATOMIC on integers
def test_tjds_atomic_iterates_exactly_on_small_integers(torch):
    """The atomic adds come in any order; on integers below 2^53 every order is exact.  Steps 1 ... 5 without normalisation (the
    buffer that is cleared alternates), and one normalised step: the raw product is exact, so the quotients are normalise()'s."""
    M = matrix("small_integers")
    assert pi.partial_sum_bound(M, pi.ones(M), 5) < 2.0 ** 53
    for steps in range(1, 6):
        y = compute("tjds", M, steps, False, mode=sm.TJDS_MODE_ATOMIC)
        assert_bits(y, M.iterate(pi.ones(M), steps), "ATOMIC, %d steps" % steps)
    y = compute("tjds", M, 1, True, mode=sm.TJDS_MODE_ATOMIC)
    assert_bits(y, pi.normalise(M.spmv(pi.ones(M))), "ATOMIC, one normalised step")


# ================================================================================================ 3. the normalisation by itself
def both_formats(torch, M):
    """(format, handle, product, entry-point options) of CSR AUTO and TJDS ROW_GATHER."""
    A, pa = csr_product(torch, M)
    T, pt = tjds_product(torch, M, sm.TJDS_MODE_ROW_GATHER)
    return (("csr", A, pa, {}), ("tjds", T, pt, {"mode": sm.TJDS_MODE_ROW_GATHER}))


@pytest.mark.parametrize("n,p,sign", PEAKS)
def test_normalisation_finds_the_largest_magnitude_wherever_it_lies(torch, n, p, sign):
    """The largest magnitude of every iterate is at index p alone, 3 against 1.5 at most elsewhere: a device maximum that skipped
    element p (the last of the absmax grid's first trip, the only one of its second) or dropped its sign changes every element."""
    M = matrix("peak", n, p, sign)
    for fmt, H, product, kw in both_formats(torch, M):
        what = "peak of %d at %d, sign %d, %s" % (n, p, sign, fmt)
        raw, its = checked_chain(M, product, pi.ones(M), 2, True, what)
        assert np.abs(raw[1]).argmax() == p and its[1][p] == 1.0
        y = compute(fmt, M, 2, True, **kw)
        assert_bits(y, its[1], what)
        if fmt == "csr":
            assert_owner_plan(H, M)
            assert_bits(y, M.iterate(pi.ones(M), 2, True), what + ", the oracle's iteration")
        H.close()


def test_a_zero_iterate_is_left_alone(torch):
    """A^2 = 0: the second iterate's maximum is 0 -- no division, no NaN from 0 / 0, +0.0 in every element -- and the third's."""
    M = matrix("square_zero")
    for fmt, H, product, kw in both_formats(torch, M):
        raw, its = checked_chain(M, product, pi.ones(M), 3, True, "square_zero, " + fmt)
        for steps in (1, 2, 3):
            y = compute(fmt, M, steps, True, **kw)
            assert_bits(y, its[steps - 1], "square_zero, %s, %d steps" % (fmt, steps))
            if steps >= 2:
                assert (y.view(np.int64) == 0).all(), "square_zero, %s, %d steps: not +0.0 everywhere" % (fmt, steps)
        assert np.abs(its[0]).max() == 1.0
        H.close()


@pytest.mark.parametrize("case", ["nan", "overflow", "subnormal"])
def test_normalisation_on_nan_infinite_and_subnormal_maxima(torch, case):
    """NaN entries take no part in the maximum and stay NaN; an infinite maximum turns finite elements into zeros of their sign
    and itself into NaN; a subnormal maximum divides like any other."""
    M, x = getattr(pi, case + "_case")()[:2]
    for fmt, H, product, kw in both_formats(torch, M):
        what = "%s start vector, %s" % (case, fmt)
        raw, its = checked_chain(M, product, x, 2, True, what)
        if case == "nan":
            assert 0 < np.isnan(raw[0]).sum() < M.n and np.nanmax(np.abs(its[0])) == 1.0
        elif case == "overflow":
            assert np.isposinf(raw[0]).sum() == 1 and np.isfinite(raw[0]).sum() == M.n - 1
        else:
            assert 0.0 < np.abs(raw[0]).max() < pi.TINY and np.abs(its[0]).max() == 1.0
        for steps in (1, 2):
            assert_bits(compute(fmt, M, steps, True, x, **kw), its[steps - 1], "%s, %d steps" % (what, steps))
        H.close()


# ========================================================================================================= 4. across the event ring
@pytest.mark.parametrize("fmt", ["csr", "tjds"])
def test_iteration_across_the_event_ring(torch, fmt):
    """1026 normalised steps: the ring of 1024 event pairs is drained in mid-run and two more steps follow."""
    M = matrix("short")
    steps = 1026
    H, product = csr_product(torch, M) if fmt == "csr" else tjds_product(torch, M)
    raw, its = checked_chain(M, product, pi.ones(M), steps, True, "short, %s, %d steps" % (fmt, steps))
    assert_bits(compute(fmt, M, steps, True), its[-1], "short, %s, %d steps" % (fmt, steps))
    assert_bits(compute(fmt, M, 1024, True), its[1023], "short, %s, 1024 steps" % fmt)
    H.close()


# =================================================================================================================== 5. several ranks
def sharded(fmt, M, ranks, exchange, chunks=0, devices="one GPU"):
    return sm.ShardedMatrix(fmt, ranks, M.n, M.n, coo=M.coo, csr=M.csr, devices=[0] * ranks if devices == "one GPU" else devices,
                            chunks=chunks, exchange=exchange)


def every_rank(S, ranks, what):
    """The gathered vector, the same bits on every rank."""
    v = S.get_y(0, gathered=True)
    for r in range(1, ranks):
        assert_bits(S.get_y(r, gathered=True), v, "%s: rank %d against rank 0" % (what, r))
    return v


def sharded_product(S, gather=sm.GATHER_OVERLAPPED):
    """A sharded handle's product for the host chain: the operand by set_x, the gathered y of rank 0."""
    def product(x):
        S.set_x(x)
        S.spmv(allgather=gather)
        S.synchronize()
        return S.get_y(0, gathered=True)

    return product


def synchronised_walk(W, Cn, M, ranks, x0, steps, gather, normalize, what):
    """spmv, synchronize, read, feed_back, synchronize, read -- every raw product the same on every rank, within check_y of the
    oracle's on that step's operand and bit for bit what the chain handle Cn (the same settings; it only ever gets set_x) gives for
    it; every vector after a feed_back is normalise() of the raw one; the local slices stay raw.  Returns the iterates."""
    chain = sharded_product(Cn, gather)
    W.synchronize()
    W.set_x(x0)
    x, its = np.asarray(x0, dtype=np.float64), []
    for k in range(steps):
        W.spmv(allgather=gather)
        W.synchronize()
        raw = every_rank(W, ranks, "%s, raw product %d" % (what, k + 1))
        check_y(raw, M.spmv(x), M.scale(x), M.terms)
        assert_bits(raw, chain(x), "%s, product %d against the chain handle's" % (what, k + 1))
        W.feed_back(normalize=normalize)
        W.synchronize()
        x = every_rank(W, ranks, "%s, iterate %d" % (what, k + 1))
        assert_bits(x, pi.normalise(raw) if normalize else raw, "%s, iterate %d" % (what, k + 1))
        assert_bits(W.get_y(0, gathered=False), raw, "%s, the local slices after feed_back %d stay raw" % (what, k + 1))
        its.append(x)
    return its


def unsynchronised_walk(W, ranks, x0, steps, gather, normalize, what):
    """The same steps with nothing but stream and event order between spmv and feed_back; one synchronize at the end."""
    W.synchronize()
    W.set_x(x0)
    for _ in range(steps):
        W.spmv(allgather=gather)
        W.feed_back(normalize=normalize)
    W.synchronize()
    return every_rank(W, ranks, what)


@pytest.mark.parametrize("push", sorted(EXCHANGES))
@pytest.mark.parametrize("ranks", [2, 8])
def test_sharded_feed_back_step_by_step(torch, ranks, push):
    """Virtual ranks on one GPU, 1003 rows (rows % ranks != 0), CSR and TJDS chunks, 1 and 3 chunks, both gather modes, four steps
    from a random vector: the synchronised walk, then the walk without a synchronize -- where only ev_placed keeps the next
    product's pushes out of a vector that is still being divided and copied -- with the synchronised walk's bits on every rank;
    both gather modes and the other push form give those bits too."""
    M = matrix("short")
    x0 = pi.random_x(M)
    PUSH = EXCHANGES[push]
    OTHER = [e for e in EXCHANGES.values() if e != PUSH][0]
    for fmt in ("csr", "tjds"):
        for chunks in (1, 3):
            final = {}
            for gather in (sm.GATHER_OVERLAPPED, sm.GATHER_AFTER):
                what = "%d ranks, %s, %s, %d chunks, gather %d" % (ranks, push, fmt, chunks, gather)
                W, Cn = sharded(fmt, M, ranks, PUSH, chunks), sharded(fmt, M, ranks, PUSH, chunks)
                assert W.layout()[0] == chunks and W.info()[0] == ranks
                for normalize in (True, False):
                    w = "%s, normalize %s" % (what, normalize)
                    its = synchronised_walk(W, Cn, M, ranks, x0, 4, gather, normalize, w)
                    got = unsynchronised_walk(W, ranks, x0, 4, gather, normalize, w + ", not synchronised")
                    assert_bits(got, its[-1], w + ", not synchronised")
                    final[gather, normalize] = its[-1]
                W.set_exchange(OTHER)                                   # the other push form on the same handle
                got = unsynchronised_walk(W, ranks, x0, 4, gather, True, what + ", the other push form")
                assert_bits(got, final[gather, True], what + ", the other push form")
                W.close()
                Cn.close()
            for normalize in (True, False):
                assert_bits(final[sm.GATHER_AFTER, normalize], final[sm.GATHER_OVERLAPPED, normalize],
                            "%d ranks, %s, %s, %d chunks: the two gather modes" % (ranks, push, fmt, chunks))


@pytest.mark.parametrize("push", sorted(EXCHANGES))
def test_sharded_feed_back_with_more_ranks_than_rows(torch, push):
    """5 rows on 8 ranks of 2 chunks each, three normalised steps.  The first product of small integers is exact: the oracle's
    bits, and normalise() of them; the later products against the oracle and against a one-rank handle's, within check_y."""
    M = matrix("tiny_integers")
    for fmt in ("csr", "tjds"):
        what = "5 rows on 8 ranks, %s, %s" % (push, fmt)
        W, one = sharded(fmt, M, 8, EXCHANGES[push], 2), sharded(fmt, M, 1, EXCHANGES[push], 2)
        single = sharded_product(one)
        W.set_x(None)
        x = pi.ones(M)
        for k in range(3):
            W.spmv()
            W.synchronize()
            raw = every_rank(W, 8, "%s, raw product %d" % (what, k + 1))
            if k == 0:
                assert_bits(raw, M.spmv(x), what + ", the first product is exact")
            check_y(raw, M.spmv(x), M.scale(x), M.terms)
            check_y(raw, single(x), M.scale(x), M.terms)
            W.feed_back(normalize=True)
            W.synchronize()
            x = every_rank(W, 8, "%s, iterate %d" % (what, k + 1))
            assert_bits(x, pi.normalise(raw), "%s, iterate %d" % (what, k + 1))
        assert_bits(unsynchronised_walk(W, 8, pi.ones(M), 3, sm.GATHER_OVERLAPPED, True, what), x, what + ", not synchronised")
        W.close()
        one.close()


@pytest.mark.parametrize("push", sorted(EXCHANGES))
@pytest.mark.parametrize("ranks", [2, 8])
def test_sharded_iteration_through_the_entry_points(torch, ranks, push):
    """opts.iterate with opts.ngpus > 1: the walk sharded_compute does over a handle of its own making -- the default shard
    options and devices, GATHER_OVERLAPPED, feed_back after every step but an un-normalised last one, rank 0's gathered vector."""
    M = matrix("short")
    x0 = pi.random_x(M)
    PUSH = EXCHANGES[push]
    for fmt in ("csr", "tjds"):
        S = sharded(fmt, M, ranks, PUSH, devices=None)
        for normalize in (False, True):
            for steps in (1, 4):
                what = "%d ranks, %s, %s, normalize %s, %d steps" % (ranks, push, fmt, normalize, steps)
                S.synchronize()
                S.set_x(x0)
                for k in range(steps):
                    S.spmv(allgather=sm.GATHER_OVERLAPPED)
                    S.synchronize()
                    if k + 1 < steps or normalize:
                        S.feed_back(normalize=normalize)
                S.synchronize()
                want = S.get_y(0, gathered=True)
                raw, its = pi.host_chain(sharded_product(S), x0, steps, normalize)
                assert_bits(want, its[-1], what + ", the handle's walk against its own chain")
                y = compute(fmt, M, steps, normalize, x0, ngpus=ranks, exchange=PUSH)
                assert_bits(y, want, what)
        S.close()


def test_a_synchronize_before_any_timed_product_leaves_no_error_behind(torch):
    """smvp_sharded_synchronize asked for a time before any timed product has run has no event pair to read; the HIP error of that
    question must not be what the launch check of a later call -- the normalisation of feed_back -- finds and reports."""
    M = matrix("tiny_integers")
    S = sharded("csr", M, 2, sm.EXCHANGE_COPIES, 1)
    assert S.synchronize() == 0.0
    S.set_x(None)
    S.spmv(timed=False)
    assert S.synchronize() == 0.0
    S.feed_back(normalize=True)
    S.synchronize()
    assert_bits(every_rank(S, 2, "tiny"), pi.normalise(M.spmv(pi.ones(M))), "a normalised feed_back after an untimed product")
    S.close()


# ================================================================================================================= 6. refusals
def refused(fn, coo, rows, cols, iters, **opts):
    """The status of smvp_csr_compute / smvp_tjds_compute called with a y of the caller's; y must come back untouched."""
    coo = np.ascontiguousarray(coo, dtype=sm.COO_DTYPE)
    y = np.full(max(rows, cols) + 2, 12345.678)
    ms = np.zeros(iters)
    o, keep = sm._run_opts(0, opts.pop("kernel", sm.CSR_KERNEL_AUTO), 0, opts.pop("ref_quirks", False), None, **opts)
    rc = getattr(sm.lib(), fn)(coo.ctypes.data_as(C.c_void_p), rows, cols, len(coo), iters, C.byref(o), y.ctypes.data_as(C.c_void_p),
                               ms.ctypes.data_as(C.c_void_p), None)
    assert (y == 12345.678).all() and (ms == 0).all(), "%s wrote its outputs although it refused" % fn
    return rc


def test_refusals_stay_refusals(torch):
    wide = sm.make_coo([0, 1, 2], [1, 3, 0], [1.5, -2.5, 3.5])                       # 3 x 4
    for fn in ("smvp_csr_compute", "smvp_tjds_compute"):
        assert refused(fn, wide, 3, 4, 2, iterate=True) == sm.ERR_INVALID
        assert refused(fn, wide, 3, 4, 2, iterate=True, normalize=True, ngpus=2, exchange=sm.EXCHANGE_COPIES) == sm.ERR_INVALID
    M = matrix("tiny_integers")
    assert refused("smvp_tjds_compute", M.coo, M.n, M.n, 2, iterate=True, ref_quirks=True) == sm.ERR_UNSUPPORTED
    assert refused("smvp_tjds_compute", M.coo, M.n, M.n, 2, iterate=True, ref_quirks=True, ngpus=2,
                   exchange=sm.EXCHANGE_COPIES) == sm.ERR_UNSUPPORTED
    row_ptr, col_ind, val = sm.csr_from_coo(wide, 3)
    x = np.array([1.0, -2.0, 3.0, 0.5])
    for fmt in ("csr", "tjds"):
        S = sm.ShardedMatrix(fmt, 2, 3, 4, coo=wide, csr=(row_ptr, col_ind, val), devices=[0, 0], exchange=sm.EXCHANGE_COPIES)
        S.set_x(x)
        S.spmv()
        S.synchronize()
        before = S.get_y(1, gathered=True)
        assert_bits(before, [-3.0, -1.25, 3.5], "3 x 4, " + fmt)
        for normalize in (False, True):
            with pytest.raises(sm.SmvpError) as e:
                S.feed_back(normalize=normalize)
            assert e.value.code == sm.ERR_INVALID
        S.synchronize()
        assert_bits(S.get_y(1, gathered=True), before, "the gathered vector after a refused feed_back")
        S.spmv()                                                                 # ... and the operand: the same product again
        S.synchronize()
        assert_bits(S.get_y(0, gathered=True), before, "the product after a refused feed_back")
        S.close()
