"""What tests/test_gpu_stream_order.py puts a stream-taking call into: operands that are still being written, and outputs that are
still being poisoned, on the stream the call is given.

Plain functions (no fixtures).  The pattern: on a non-blocking stream `side` a delay kernel runs first, then the copies that give
every operand its true content, then the fills that poison every output, then an event.  While the event is pending the operands
hold STALE content: NaN in doubles, and in integer structure arrays a valid structure of the same sizes that is not the true one
(stale_like: every index 0, every COO entry (0, 0, 1.0)), so that work which runs too early -- on the null stream, on a stream
of the library's own that was not joined, in a blocking copy that did not wait for `side` -- computes wrong numbers and can never
index out of range.  Work enqueued on `side` itself comes behind the copies and the fills and sees the true content.

The delay is an input, not a pass criterion: the guard is the event.  It must still be pending immediately before the library call
and, for the asynchronous entry points, immediately after it returns (every enqueue happened while the operands were pending, and
the call synchronised nothing).  An event found complete is a failure of the test -- "delay too short" -- never a skip or a pass."""
import numpy as np

from parity import check_guards
from transposed import assert_bits

TARGET_MS = 50.0        # how long the operands stay pending; a case whose host side needs longer passes its own ms to in_flight
_RATE = {}              # {"cycles_per_ms": ...}: torch.cuda._sleep measured once per process, printed once


def sleep_rate(torch, side):
    """Cycles of torch.cuda._sleep per millisecond on this device, measured once with an event pair on `side` (the probe grows
    until it takes 5 ms or more, so that the launch overhead does not count)."""
    if "cycles_per_ms" not in _RATE:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(1000)                                  # (the first launch loads the kernel)
        side.synchronize()
        cycles, ms = 1_000_000, 0.0
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                a.record(side)
                torch.cuda._sleep(cycles)
                b.record(side)
            side.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0 or cycles >= 1 << 40:
                break
            cycles *= 8
        assert ms > 0.0, "torch.cuda._sleep(%d) took no time" % cycles
        _RATE["cycles_per_ms"] = cycles / ms
        print("stream order: torch.cuda._sleep runs %.0f cycles per ms (%d cycles in %.2f ms); target delay %.0f ms"
              % (_RATE["cycles_per_ms"], cycles, ms, TARGET_MS))
    return _RATE["cycles_per_ms"]


def runs_beside_the_null_stream(torch, s):
    """Whether work on the null stream finishes while a delay on `s` is still running.  Streams are non-blocking, but the runtime
    maps them onto a few hardware queues (four by default), and two streams that share a queue run one after the other: wrong-stream
    work would then wait for the operands by accident and nothing here could see it."""
    cycles = int(sleep_rate(torch, s) * 20.0)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        torch.cuda._sleep(cycles)
        ev = torch.cuda.Event()
        ev.record(s)
    probe = torch.zeros(64, dtype=torch.float64, device="cuda").add_(1.0)      # the null stream
    done = torch.cuda.Event()
    done.record()
    done.synchronize()
    beside = not ev.query()
    torch.cuda.synchronize()
    assert probe.sum().item() == 64.0
    return beside


def side_stream(torch, tries=16):
    """The caller's stream of the tests: one of torch's pool streams (non-blocking: nothing orders them against the null stream)
    whose work was seen to run beside the null stream's.  None of `tries` streams doing so is a failure: every test would be
    vacuous."""
    shared = []
    for _ in range(tries):
        s = torch.cuda.Stream()
        if runs_beside_the_null_stream(torch, s):
            print("stream order: stream %#x runs beside the null stream (%d before it shared its hardware queue)" % (s.cuda_stream, len(shared)))
            return s
        shared.append(s)
    raise AssertionError("none of %d pool streams runs beside the null stream: work on the wrong stream is invisible on this machine" % tries)


def stale_like(torch, t, kind="zeros"):
    """Stale content for an integer structure array: a valid structure of the same size that is not the true one.  "zeros": every
    index 0 (a column index, a row index, a permutation entry read as a position); "coo": every smvp_coo_t (0, 0, 1.0) in a uint8
    tensor of 16-byte entries."""
    if kind == "zeros":
        return torch.zeros_like(t)
    assert kind == "coo" and str(t.dtype) == "torch.uint8" and t.numel() % 16 == 0, (kind, t.dtype, t.numel())
    one = np.zeros(1, dtype=np.dtype([("row", "<i4"), ("col", "<i4"), ("val", "<f8")], align=True))
    one["val"] = 1.0
    return torch.from_numpy(np.tile(one.view(np.uint8), t.numel() // 16)).to(t.device)


def stage(torch, t, stale=None):
    """(t, a separate device tensor with t's true content): a pair for in_flight.  t itself is left holding stale content: NaN
    for doubles, `stale` (a tensor of t's shape, see stale_like) for anything else.  Call it with the device idle."""
    true = t.clone()
    if t.dtype.is_floating_point:
        assert stale is None
        t.fill_(float("nan"))
    else:
        assert stale is not None and stale.shape == t.shape and not torch.equal(stale, true), "the stale structure must differ from the true one"
        t.copy_(stale)
    return t, true


def in_flight(torch, side, pairs, outputs, ms=None):
    """On entry every destination in `pairs` holds stale content, every staged true value sits in a separate device tensor, and
    the device has been synchronised.  Enqueues on `side`, in this order: the delay, dst.copy_(src) for every pair, a NaN fill of
    every output (views into parity.guarded_y buffers: the guards stay), then an event.  Returns the event."""
    cycles = int(sleep_rate(torch, side) * (TARGET_MS if ms is None else ms))
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        for dst, src in pairs:
            dst.copy_(src, non_blocking=True)
        for out in outputs:
            out.fill_(float("nan"))
        ev = torch.cuda.Event()
        ev.record(side)
    return ev


def pending(ev, when):
    """The guard: the event of in_flight has not completed."""
    assert not ev.query(), "delay too short: the operands' event had completed %s" % when


def read_on(torch, side, outputs):
    """The results of asynchronous calls on `side`, seen from `side` alone: a clone of every output is enqueued there, then
    side.synchronize() -- and nothing else -- and the clones come back as numpy arrays (with the device tensors, for settled)."""
    with torch.cuda.stream(side):
        clones = [o.clone() for o in outputs]
    side.synchronize()
    return [c.cpu().numpy() for c in clones], clones


def settled(torch, outputs, clones, guarded=(), what=""):
    """After read_on: the whole device is synchronised, the guards of every (buffer, rows) in `guarded` are intact, and every
    output still has its clone's bits -- a straggler on another stream, finishing after `side` did, would have changed it."""
    torch.cuda.synchronize()
    for buf, rows in guarded:
        check_guards(buf, rows)
    for i, (o, c) in enumerate(zip(outputs, clones)):
        assert_bits(o.cpu().numpy().ravel(), c.cpu().numpy().ravel(), "%s: output %d after the device has settled against what `side` saw" % (what, i))


def solver_hook(torch, side, seen=None, ms=None):
    """The hook the solve() helpers of the solver tests take in place of their leading torch.cuda.synchronize(): every input vector
    (b, x0, m -- whatever the helper passes that is not None) goes in flight behind the delay, d_x is poisoned in flight, and the
    guard is checked right before the library call.  seen: a list that receives (event, pairs) -- to check afterwards that the call
    returned after the event, and to keep the staged tensors alive until then."""
    seen = [] if seen is None else seen

    def before(x, **inputs):
        torch.cuda.synchronize()
        pairs = [stage(torch, t) for t in inputs.values() if t is not None]
        torch.cuda.synchronize()
        ev = in_flight(torch, side, pairs, [x], ms)
        seen.append((ev, pairs))
        pending(ev, "before the call")
    return before

