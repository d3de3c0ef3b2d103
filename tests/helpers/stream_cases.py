"""The stream contract of include/literate_hip.h, entry point by entry point (tests/test_hip_stream_contract.py runs every
case in a child process of its own, under a time limit):

    python tests/helpers/stream_cases.py CASE [ARG ...]

The header promises that "`stream` is a hipStream_t passed as void* (NULL = default stream); every call is asynchronous on
it and returns after enqueueing" and that "what a call needs cleared it clears itself, on `stream`".  Every other test
passes torch's default stream and ends in a synchronise, which hides a launch, a copy or a memset on another stream and a
missing join alike.  ordered() runs a case on a side stream that is non-blocking against the null stream and BUSY:

  1. plain passes on the default stream, each ended by a synchronise: the decoy B in the buffers the call reads -> want_b,
     then input set A -> want_a (the decoy first: what happens once per process, kernels loaded at their first launch, is
     then not in the host times taken with A).  want_a == want_b: the case could not see a stale read ('blind').  B is
     valid data of the same shapes: a misordered kernel reads in-range counts, indices and times - the case can fail,
     never fault.
  2. side pass: B is left in the buffers.  On the side stream: a delay (a spinning kernel), then the copies of A into
     the buffers, then call(), then - with no host synchronisation - a clone of every output.  The workspaces and outputs
     the call allocates come from Guarded(0xFF), whose fills are enqueued on the side stream too: a clear issued on any
     other stream is overwritten by the fill.  After side.synchronize() the outputs and the clones must have want_a's
     bits.  Work that ran on another stream without waiting for the caller's read B or was overwritten ('order'); work that
     waited but was not joined back is missing from the clone ('join').  A rehearsal of the same pass without the delay
     comes first and is judged for the join alone: it takes the host time of what happens once per stream (the
     allocator's first blocks), and with nothing held back the streams a call forks onto start as they are enqueued, the
     last one last, which is when a missing join shows most surely (behind a delay they start, and may end, together).
  3. the hook: for the side pass every function of the library whose last parameter is the stream is wrapped.  The
     wrapper notes whether the delay enqueued last is still running (an event behind it; if not, the case or a wrapper of
     literate_amd drained the stream: 'inconclusive' - nothing was tested), enqueues a delay of its own on the stream it was
     given so that successive calls are separated too, calls, and notes whether that delay is still running when the call
     returns: if it is not, the call waited for it ('blocked'), unless the header says that it blocks (BLOCKING, by the
     sentence; the call behind such a one is excused from finding the stream busy).  A delay still running at the return
     proves that it was long enough: its length is no criterion.  It is the larger of 20 ms and ten times the longest host
     time of a single call in the plain pass (the first replay instantiates a hipGraph), at most 500 ms.
  4. the side stream: torch's pool streams are non-blocking against the null stream, but a process has GPU_MAX_HW_QUEUES
     hardware queues (4 by default), the runtime maps the streams that have work onto them, and two streams on one queue
     run in order - beside such a side stream work on the null stream looks ordered.  The child process asks for 16
     queues, and TorchRuntime.side_stream() takes the first stream beside which work on the null stream demonstrably runs
     (by values: _runs_beside), from torch's pool and then from hipStreamCreateWithFlags(hipStreamNonBlocking).

ordered() takes its runtime as a parameter: TorchRuntime on the device, DeferredRuntime - streams as queues of closures
that a delay holds back until somebody synchronises - in tests/test_stream_contract_host.py, which replays the fakes of
FAULTS on it and checks COVERS and BLOCKING against the headers."""
import contextlib
import ctypes as C
import glob
import os
import re
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import abi_cases as A  # noqa: E402
from helpers.abi_cases import (Guarded, T0, _bits, _engine_state, _make_engine, _tensors, abi, dev, lineages, rates,  # noqa: E402,F401
                               say)

MIN_DELAY_MS, MAX_DELAY_MS, DELAY_FACTOR = 20.0, 500.0, 10.0


class StreamViolation(AssertionError):
    """kind: 'order' (the call's work did not run behind the caller's earlier work on `stream`), 'join' (it did, but the
    caller's later work on `stream` did not wait for it), 'blocked' (the call waited for the stream although the header
    does not say so), 'inconclusive' (the stream was idle when an entry point was called, or no delay is long enough: the
    case tests nothing), 'blind' (the decoy gives the same answer)."""

    def __init__(self, kind, msg):
        super().__init__("%s: %s" % (kind, msg))
        self.kind = kind


# entry point -> the header sentence by which it may wait for `stream` (verbatim, as `partial` in abi_cases)
BLOCKING = {
    "lr_mcmc_time_scan": "Blocks until the launches finish; re-scores the pending proposal, so chain state is unchanged.",
    "lr_mcmc_time_steps": "lr_mcmc_steps(n_iters) bracketed by HIP events on `stream`; blocks; *total_ms = elapsed device time.",
    "lr_mcmc_status": "Blocks until `stream` is idle and copies the engine status word to *status (host)",
    "lr_mcmc_warnings": "Blocks until `stream` is idle and copies the engine's warning word to *warnings (host)",
    "lr_mcmc_init": "lr_mcmc_init and lr_mcmc_restore block until `stream` is idle on the persistent engines and on the packed scan",
    "lr_mcmc_restore": "lr_mcmc_init and lr_mcmc_restore block until `stream` is idle on the persistent engines and on the packed scan",
}


def stream_entry_points(root=ROOT):
    """every function the headers declare whose last parameter is `void* stream` -> the header it stands in"""
    out = {}
    for h in sorted(glob.glob(os.path.join(root, "include", "*.h"))):
        with open(h) as f:
            text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
        for m in re.finditer(r"\b(?:int|int64_t)\s+(lr_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
            args = [" ".join(a.split()) for a in m.group(2).split(",")]
            if args[-1] == "void* stream":
                out[m.group(1)] = os.path.basename(h)
    return out


# ------------------------------------------------------------------------------------------------
# the runtimes
# ------------------------------------------------------------------------------------------------
class TorchRuntime:
    """HIP streams through torch.  library: (object whose attributes are the entry points, their names); None: the loaded
    libliterate_hip.so and every function of the headers that takes the stream."""

    def __init__(self, library=None):
        import torch
        assert torch.cuda.is_available(), "the cases need an MI355X"
        from literate_amd import ops
        self.torch, self.ops, self._library = torch, ops, library

    _per_ms = None          # spin cycles per millisecond: calibrated once per process

    def entry_points(self):
        if self._library is None:
            from literate_amd import _hip
            self._library = (_hip.load(), sorted(stream_entry_points()))
        return self._library

    # streams
    def _runs_beside(self, busy, other):
        """Does work on `other` run while `busy` is held up - the situation of every case, rehearsed on a buffer of its
        own?  No rule orders two non-blocking streams, but a process has only GPU_MAX_HW_QUEUES hardware queues, the
        runtime maps the streams that have work onto them, and two streams on one queue run in order: beside such a side
        stream work issued on the wrong stream would look right.  Decided by values, not by times."""
        torch = self.torch
        src, dst = self._probe
        src.fill_(1.0)
        torch.cuda.synchronize()
        with torch.cuda.stream(busy):
            self.sleep(5.0)
            src.fill_(2.0)
        with torch.cuda.stream(other):
            torch.mul(src, 3.0, out=dst)
        torch.cuda.synchronize()
        return bool((dst == 3.0).all())

    def _raw_stream(self):
        """a stream of hipStreamCreateWithFlags(hipStreamNonBlocking), never destroyed (the child process is short)"""
        hip = C.CDLL("libamdhip64.so")
        h = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(h), C.c_uint(1)) == 0 and h.value          # hipStreamNonBlocking = 0x01
        return self.torch.cuda.ExternalStream(h.value)

    _streams = None          # (side, other): chosen once per process - every further stream competes for the hardware queues

    def side_stream(self):
        """A stream beside which the null stream runs and, for the fakes, a second one beside which the first runs and
        that runs beside the first: from torch's pool (non-blocking streams), then from hipStreamCreateWithFlags."""
        torch = self.torch
        if TorchRuntime._streams is None:
            self.calibrate()
            self._probe = torch.zeros(256, dtype=torch.float64, device="cuda"), torch.zeros(256, dtype=torch.float64, device="cuda")
            null, found, tried = torch.cuda.default_stream(), [], 0
            for attempt in range(12):
                s = torch.cuda.Stream() if attempt < 8 else self._raw_stream()
                if any(s.cuda_stream == f.cuda_stream for f in found):
                    continue
                tried += 1
                if not found and self._runs_beside(s, null):
                    found.append(s)
                elif found and self._runs_beside(found[0], s) and self._runs_beside(s, found[0]) and self._runs_beside(found[0], null):
                    found.append(s)
                    break
            assert len(found) == 2, ("of %d streams no two run beside the null stream and each other (GPU_MAX_HW_QUEUES=%s): work on a "
                                     "wrong stream could not be told from work on the right one" % (tried, os.environ.get("GPU_MAX_HW_QUEUES")))
            say("streams: side %#x, another %#x, after %d tried" % (found[0].cuda_stream, found[1].cuda_stream, tried))
            TorchRuntime._streams = tuple(found)
        self._other = TorchRuntime._streams[1]
        return TorchRuntime._streams[0]

    def pool_stream(self):
        return getattr(self, "_other", None) or self.torch.cuda.Stream()

    def null_stream(self):
        return self.torch.cuda.default_stream()

    def stream(self, s):
        return self.torch.cuda.stream(s)

    def stream_of(self, arg):
        v = getattr(arg, "value", arg)
        return self.null_stream() if not v else self.torch.cuda.ExternalStream(int(v))

    def current_stream_arg(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def synchronize(self):
        self.torch.cuda.synchronize()

    def record(self, s):
        ev = self.torch.cuda.Event()
        ev.record(s)
        return ev

    def record_here(self):
        ev = self.torch.cuda.Event()
        ev.record()
        return ev

    def wait(self, s, ev):
        s.wait_event(ev)

    def calibrate(self):
        """spin cycles per millisecond of torch.cuda._sleep, measured once per process with events"""
        torch = self.torch
        if TorchRuntime._per_ms is None:
            cycles = 1000000
            for _ in range(8):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                torch.cuda._sleep(cycles)
                e1.record()
                e1.synchronize()
                took = e0.elapsed_time(e1)
                if took >= 5.0:
                    break
                cycles *= 4
            assert took >= 5.0, "torch.cuda._sleep(%d) took %.3f ms: no delay can be built from it" % (cycles, took)
            TorchRuntime._per_ms = cycles / took
            say("delay: %.0f spin cycles per ms" % TorchRuntime._per_ms)

    def sleep(self, ms):
        """a kernel that spins for about `ms` on the current stream"""
        self.calibrate()
        self.torch.cuda._sleep(int(ms * TorchRuntime._per_ms))

    # tensors
    def copy(self, dst, src):
        dst.copy_(src)

    def clone(self, t):
        return t.clone()

    def bits(self, t):
        return _bits(self.torch, t)

    def tensors(self, out):
        return _tensors(self.torch, out)[0]

    @contextlib.contextmanager
    def seam(self, fill):
        ops = self.ops
        saved = ops.alloc_workspace, ops.alloc_output
        g = Guarded(self.torch, fill)
        ops.alloc_workspace, ops.alloc_output = g.workspace, g.output
        try:
            yield g
        finally:
            ops.alloc_workspace, ops.alloc_output = saved

    # what the fakes of FAULTS need beyond that
    def alloc_output(self, n):
        return self.ops.alloc_output(int(n), self.torch.float64, "cuda")

    def kernel(self, dst, src):
        self.torch.mul(src, 3.0, out=dst)

    def fill(self, dst, value):
        dst.fill_(value)

    def upload(self, x):
        return self.torch.as_tensor(x).cuda()          # from pageable memory: the copy waits for the current stream

    def host_tensor(self, x):
        return dev(self.torch, x)


class _Queue:
    """A stream of DeferredRuntime: closures run at once while nothing holds the queue back; a delay, or a wait for an event
    that has not happened, holds back everything behind it until somebody synchronises."""

    def __init__(self, rt, name):
        self.rt, self.name, self.todo, self.done = rt, name, [], 0

    def enqueue(self, fn, holds=False):
        self.todo.append((fn, holds))
        if not holds:
            self._run(len(self.todo), eager=True)

    def _run(self, upto, eager=False):
        while self.done < upto:
            fn, holds = self.todo[self.done]
            if eager and (holds or (getattr(fn, "event", None) is not None and not fn.event.happened())):
                return
            self.done += 1
            fn()

    def synchronize(self):
        self._run(len(self.todo))

    def query(self):
        return self.done == len(self.todo)


class _Event:
    def __init__(self, q):
        self.q, self.at = q, len(q.todo)

    def happened(self):
        return self.q.done >= self.at

    query = happened

    def reach(self):
        self.q._run(self.at)


class DeferredRuntime:
    """ordered()'s runtime without a device: numpy arrays, streams as queues (_Queue).  The null stream and the pool streams
    do not wait for each other, as HIP's non-blocking streams."""

    def __init__(self, library):
        self._library = library
        self._null = _Queue(self, "null")
        self._current, self._streams, self._fill = self._null, [self._null], None

    def entry_points(self):
        return self._library

    def side_stream(self):
        q = _Queue(self, "pool %d" % len(self._streams))
        self._streams.append(q)
        return q

    pool_stream = side_stream

    def null_stream(self):
        return self._null

    @contextlib.contextmanager
    def stream(self, s):
        saved, self._current = self._current, s
        try:
            yield
        finally:
            self._current = saved

    def stream_of(self, arg):
        return arg

    def current_stream_arg(self):
        return self._current

    def synchronize(self):
        for q in self._streams:
            q.synchronize()

    def record(self, s):
        return _Event(s)

    def record_here(self):
        return _Event(self._current)

    def wait(self, s, ev):
        fn = ev.reach
        wrapped = lambda: fn()
        wrapped.event = ev
        s.enqueue(wrapped)

    def sleep(self, ms):
        self._current.enqueue(lambda: None, holds=True)

    def copy(self, dst, src):
        self._current.enqueue(lambda: np.copyto(dst, src))

    def clone(self, t):
        out = np.empty_like(t)
        self._current.enqueue(lambda: np.copyto(out, t))
        return out

    def bits(self, t):
        return np.ascontiguousarray(t).tobytes()

    def tensors(self, out):
        return {"0": out} if isinstance(out, np.ndarray) else {str(k): v for k, v in (out.items() if isinstance(out, dict) else enumerate(out))}

    @contextlib.contextmanager
    def seam(self, fill):
        self._fill = fill
        try:
            yield None
        finally:
            self._fill = None

    def alloc_output(self, n):
        out = np.zeros(int(n))
        if self._fill is not None:
            fill = self._fill
            self._current.enqueue(lambda: out.view(np.uint8).fill(fill))
        return out

    def kernel(self, dst, src):
        self._current.enqueue(lambda: np.multiply(src, 3.0, out=dst))

    def fill(self, dst, value):
        self._current.enqueue(lambda: dst.fill(value))

    def upload(self, x):
        self._current.synchronize()
        return np.array(x)

    def host_tensor(self, x):
        return np.array(x, dtype=float)


# ------------------------------------------------------------------------------------------------
# the harness
# ------------------------------------------------------------------------------------------------
class _Hook:
    """The entry points of rt.entry_points() wrapped.  mode 'time': the host time of every call; mode 'check': busy before,
    a delay, the call, busy after."""

    def __init__(self, rt, blocking):
        self.rt, self.blocking = rt, set(blocking)
        self.calls, self.mode, self.delay_ms, self.delay_at, self.last_delay = [], None, 0.0, 0.0, None

    @contextlib.contextmanager
    def installed(self, mode, delay_ms=0.0):
        obj, names = self.rt.entry_points()
        saved = {n: getattr(obj, n) for n in names}
        self.mode, self.delay_ms, self._drained = mode, delay_ms, False
        for n in names:
            setattr(obj, n, self._wrap(n, saved[n]))
        try:
            yield self
        finally:
            for n, fn in saved.items():
                setattr(obj, n, fn)

    def _wrap(self, name, fn):
        rt = self.rt

        def wrapper(*args):
            if self.mode == "time":
                t = time.perf_counter()
                rc = fn(*args)
                self.calls.append(dict(name=name, mode="time", ms=(time.perf_counter() - t) * 1e3))
                return rc
            # busy: the delay enqueued last has not run out (an event behind it; a stream that merely has the case's own
            # fills in flight behind an upload that drained it is not busy in this sense)
            s = rt.stream_of(args[-1])
            busy_before = self.last_delay is not None and not self.last_delay.query() and not s.query()
            since = (time.perf_counter() - self.delay_at) * 1e3
            with rt.stream(s):
                rt.sleep(self.delay_ms)
                mine = rt.record_here()
            t = time.perf_counter()
            rc = fn(*args)
            ms = (time.perf_counter() - t) * 1e3
            busy_after = not mine.query()
            self.last_delay = mine
            # the call behind one that may block finds the stream as that one left it: possibly idle (lr_mcmc_init waits in
            # its middle and enqueues a few short kernels behind that)
            self.calls.append(dict(name=name, mode="check", ms=ms, busy_before=busy_before or self._drained, busy_after=busy_after, since=since))
            self._drained = name in self.blocking
            return rc
        wrapper.__name__ = name
        return wrapper

    def longest(self):
        return max([c for c in self.calls if c["mode"] == "time"], key=lambda c: c["ms"], default=None)

    def table(self):
        """per entry point: calls, the longest host time of one in the plain pass and in the side pass (ms), the delay"""
        rows = {}
        for c in self.calls:
            r = rows.setdefault(c["name"], dict(calls=0, time=0.0, check=0.0))
            r[c["mode"]] = max(r[c["mode"]], c["ms"])
            r["calls"] += c["mode"] == "time"
        return rows


def _pass(rt, hook, mode, delay_ms, call, prepare, buffers, first, then, finish):
    """prepare, `first` into the buffers (and a synchronise), [the delay, `then` into the buffers], call(), clones"""
    ctx = prepare() if prepare else None
    bufs = buffers(ctx) if callable(buffers) else buffers
    assert len(bufs) == len(first), "one input per buffer"
    for b, x in zip(bufs, first):
        rt.copy(b, x)
    rt.synchronize()
    if then is not None:
        hook.last_delay = None
        if delay_ms:
            rt.sleep(delay_ms)
            hook.last_delay = rt.record_here()
        for b, x in zip(bufs, then):
            rt.copy(b, x)
        hook.delay_at = time.perf_counter()
    with (hook.installed(mode, delay_ms) if mode else contextlib.nullcontext()):
        out = call(ctx) if prepare else call()
    ts = rt.tensors(out)
    snap = {k: rt.clone(v) for k, v in ts.items()} if then is not None else None
    return ctx, ts, snap


def _differs(got, want):
    for k in want:
        if got[k] != want[k]:
            a, b = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
            return "output %s (%d bytes, first difference at byte %d)" % (k, b.size, int(np.nonzero(a != b)[0][0]) if a.size == b.size else -1)
    return None


def ordered(rt, call, inputs_a, inputs_b, buffers, label, blocking=(), prepare=None, finish=None):
    """Hold call() to the stream contract (the module docstring).  buffers: the device tensors the call reads - or a
    function of prepare()'s result that returns them; inputs_a / inputs_b: what they hold, A and the decoy.  An entry point
    without a device input has no decoy: buffers = (), and only the fills, the join and the return are checked.
    prepare(): run before the inputs are copied, on the stream and through the seam of the pass; it may synchronise (an
    engine's constructor does).  call(ctx) then.  finish(ctx, outputs): after the pass's synchronise -> further bits to
    compare (host reads allowed), and the place to release what prepare() made.  Returns (want_a, hook table)."""
    hook = _Hook(rt, blocking)
    getattr(rt, "calibrate", lambda: None)()
    no_inputs = not callable(buffers) and len(buffers) == 0

    def bits(ts, ctx):
        got = {k: rt.bits(v) for k, v in ts.items()}
        if finish:
            got.update({"finish " + k: v for k, v in finish(ctx, ts).items()})
        return got

    # 1. the plain passes: the decoy first, so that what happens once per process (kernels loaded at their first launch) is
    # not in the host times taken with A
    if not no_inputs:
        ctx, ts, _ = _pass(rt, hook, None, 0.0, call, prepare, buffers, inputs_b, None, finish)
        rt.synchronize()
        want_b = bits(ts, ctx)
    ctx, ts, _ = _pass(rt, hook, "time", 0.0, call, prepare, buffers, inputs_a, None, finish)
    rt.synchronize()
    want_a = bits(ts, ctx)
    if not no_inputs and want_a == want_b:
        raise StreamViolation("blind", "%s: the decoy gives the same bits as the inputs: a stale read would not show" % label)
    slow = hook.longest()
    assert slow is not None, "%s: the call reaches no entry point that takes the stream" % label
    delay_ms = max(MIN_DELAY_MS, DELAY_FACTOR * slow["ms"])
    if delay_ms > MAX_DELAY_MS:
        raise StreamViolation("inconclusive", "%s: %s took %.1f ms of host time: it needs a delay of %.0f ms, above the cap of %.0f"
                              % (label, slow["name"], slow["ms"], delay_ms, MAX_DELAY_MS))
    # 2. the side passes
    side = rt.side_stream()
    first = inputs_b if not no_inputs else ()

    def side_pass(mode, delay):
        with rt.seam(0xFF) as guarded, rt.stream(side):
            ctx, ts, snap = _pass(rt, hook, mode, delay, call, prepare, buffers, first, inputs_a, finish)
        side.synchronize()
        got_snap = {k: rt.bits(v) for k, v in snap.items()}
        got_side = {k: rt.bits(v) for k, v in ts.items()}
        rt.synchronize()
        got_dev = bits(ts, ctx)
        if guarded is not None:
            guarded.check_guards(label + " side stream")
        want_out = {k: want_a[k] for k in got_side}
        return _differs(got_dev, want_a), _differs(got_snap, want_out) or _differs(got_side, want_out)
    join = ("%s: %s is right once the device is idle but not for work enqueued on `stream` behind the call: part of the call is not "
            "joined back%s")
    # a rehearsal without the delay.  What happens once per stream or process (the allocator's first blocks for that stream,
    # kernels loaded at their first launch) takes host time that is not the call's; and with nothing held back the work a
    # call forks starts as it is enqueued, the last of it last: the regime in which a missing join shows most surely (behind
    # a delay the forked streams start together and may finish together).  Only that is judged here - order needs the delay
    wrong, stale = side_pass(None, 0.0)
    if stale and not wrong:
        raise StreamViolation("join", join % (label, stale, " (the pass without a delay)"))
    wrong, stale = side_pass("check", delay_ms)
    checks = [c for c in hook.calls if c["mode"] == "check"]
    for c in checks:
        if not c["busy_before"]:
            raise StreamViolation("inconclusive", "%s: the delay had run out when %s was called, %.1f ms of host time behind a delay of %.0f "
                                  "ms: the case synchronised, uploaded or read back between the delay and the call"
                                  % (label, c["name"], c["since"], delay_ms))
    if wrong:
        raise StreamViolation("order", "%s: on a busy side stream %s differs from the default stream's: part of the call did not run "
                              "behind the work enqueued on `stream` before it" % (label, wrong))
    if stale:
        raise StreamViolation("join", join % (label, stale, ""))
    for c in checks:
        if not c["busy_after"] and c["name"] not in blocking:
            raise StreamViolation("blocked", "%s: %s returned only when `stream` was idle (%.1f ms, behind a delay of %.0f ms): it waits "
                                  "for the stream, and the header does not say so" % (label, c["name"], c["ms"], delay_ms))
    table = hook.table()
    for name, r in sorted(table.items()):
        say("  %-24s calls %d  host %8.3f ms  behind the delay %8.3f ms  delay %5.0f ms" % (name, r["calls"], r["time"], r["check"], delay_ms))
    return want_a, table


# ------------------------------------------------------------------------------------------------
# the harness on fakes (the device self-test and tests/test_stream_contract_host.py)
# ------------------------------------------------------------------------------------------------
# fault -> the violation ordered() must raise (None: it passes)
FAULTS = {None: None, "works on another pool stream": "order", "works on the null stream": "order", "joins nothing back": "join",
          "synchronises": "blocked", "uploads a host array first": "inconclusive", "ignores its input": "blind"}


def fake_library():
    return types.SimpleNamespace(), ["fake_entry"]


def run_fake(rt, fault):
    """One entry point, out = 3 * in, on the library object of rt (fake_library), and the ways it can break the contract."""
    lib, _ = rt.entry_points()
    n = 4096

    def fake_entry(src, dst, stream):
        s = rt.stream_of(stream)
        if fault == "works on another pool stream":
            with rt.stream(rt.pool_stream()):
                rt.kernel(dst, src)
        elif fault == "works on the null stream":
            with rt.stream(rt.null_stream()):
                rt.kernel(dst, src)
        elif fault == "joins nothing back":
            other = rt.pool_stream()
            rt.wait(other, rt.record(s))
            with rt.stream(other):
                rt.sleep(5.0)
                rt.kernel(dst, src)
        else:
            with rt.stream(s):
                if fault == "ignores its input":
                    rt.fill(dst, 1.0)
                else:
                    rt.kernel(dst, src)
            if fault == "synchronises":
                s.synchronize()
        return 0
    lib.fake_entry = fake_entry
    a, b = rt.host_tensor(np.arange(n, dtype=float)), rt.host_tensor(np.arange(n, dtype=float) + 0.5)
    src = rt.host_tensor(np.zeros(n))
    rt.synchronize()

    def call():
        if fault == "uploads a host array first":
            rt.upload(np.ones(1 << 18))
        dst = rt.alloc_output(n)
        assert lib.fake_entry(src, dst, rt.current_stream_arg()) == 0          # (looked up at call time, as _hip.launch's callers do)
        return dst
    return ordered(rt, call, [a], [b], [src], "fake that " + str(fault))


def self_test(rt_factory):
    for fault, kind in FAULTS.items():
        rt = rt_factory(fake_library())
        try:
            run_fake(rt, fault)
            got = why = None
        except StreamViolation as e:
            got, why = e.kind, e
        assert got == kind, "a fake that %s: expected %s, got %s (%s)" % (fault, kind, got, why)
        say("fake that %s: %s" % (fault, got))


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
COVERS = {}            # case name -> the entry points it runs that must not block
RUNS_BLOCKING = {}     # case name -> the entry points of BLOCKING it runs


def case(*entry_points):
    def deco(fn):
        COVERS[fn.__name__[5:]] = tuple(e for e in entry_points if e not in BLOCKING)
        RUNS_BLOCKING[fn.__name__[5:]] = tuple(e for e in entry_points if e in BLOCKING)
        return fn
    return deco


def _gpu():
    rt = TorchRuntime()
    from literate_amd import _hip
    return rt, rt.torch, rt.ops, _hip, _hip.load()


def _sets(torch, make):
    """(inputs A, decoy B, buffers) from make(seed) -> host arrays"""
    a, b = [dev(torch, x) for x in make(0)], [dev(torch, x) for x in make(1)]
    assert all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(a, b))
    return a, b, [torch.empty_like(x) for x in a]


def _hold(rt, label, call, sets, **kw):
    a, b, bufs = sets
    out = ordered(rt, lambda: call(*bufs), a, b, bufs, label, **kw)
    say(label, "ok")
    return out


@case("lr_bin_events")
def case_bin_events():
    rt, torch, ops, _hip, lib = _gpu()
    n, w = 4099, 65

    def make(seed):
        ts, te = lineages(n, 40, seed)
        rng = np.random.default_rng(w + seed)
        lo = T0 - 2.0 + rng.random(w) * 40.0
        return ts, te, lo, lo + 0.25 + rng.random(w) * 7.0
    _hold(rt, "bin_events n %d windows %d" % (n, w), lambda ts, te, lo, hi: ops.bin_events(ts, te, lo, hi), _sets(torch, make))


@case("lr_bin_unit_events")
def case_bin_unit():
    """73 bins: the first class that raises the kernel's LDS attribute"""
    rt, torch, ops, _hip, lib = _gpu()
    n, nb = 4099, 73
    assert A.ub_plan(nb)[1] > 64 * 1024 >= A.ub_plan(nb - 1)[1]
    _hold(rt, "bin_unit n %d bins %d" % (n, nb), lambda ts, te: ops.bin_unit_events(ts, te, T0, nb),
          _sets(torch, lambda seed: lineages(n, nb, seed)))


CHAINS, BINS = 5, 7


@case("lr_expand_rates", "lr_rj_propose_score", "lr_log_priors")
def case_chain_maps():
    rt, torch, ops, _hip, lib = _gpu()
    kmax = 4

    def seg(seed):
        r, t, K = A._segments(CHAINS, kmax, BINS, np.random.default_rng(50 + seed))
        return r, t, K
    _hold(rt, "expand_rates", lambda r, t, K: ops.expand_rates(r, t, K, BINS, 0), _sets(torch, seg))

    def pri(seed):
        rng = np.random.default_rng(60 + seed)
        r, t, K = seg(seed)
        return r, K, 0.5 + rng.random(CHAINS), 0.5 + rng.random(CHAINS)
    _hold(rt, "log_priors", lambda r, K, g, p: ops.log_priors(r, K, 2.0, g, p), _sets(torch, pri))

    def rj(seed):
        # a multiplier move on every chain, K = 2 (the construction of abi_cases.case_chain_maps)
        rng = np.random.default_rng(70 + seed)
        k = 2
        tt = np.zeros((CHAINS, kmax + 1))
        tt[:, :k + 1] = np.linspace(0.0, 100.0, k + 1)
        u = rng.uniform(0.05, 0.95, (CHAINS, 2 * kmax))
        u[:, :kmax] = (u[:, :kmax] < 0.5)
        return (0.05 + rng.random((CHAINS, kmax)), tt, np.full(CHAINS, k, dtype=np.int32), np.zeros(CHAINS, dtype=np.int32),
                np.zeros(CHAINS, dtype=np.int32), u)
    _hold(rt, "rj_propose_score", lambda *a: ops.rj_propose_score(*a), _sets(torch, rj))


@case("lr_dd_rates", "lr_ddv2_rates", "lr_trend_rates", "lr_binned_keiding")
def case_rate_maps():
    rt, torch, ops, _hip, lib = _gpu()
    Cn = CHAINS

    def par(seed):
        rng = np.random.default_rng(80 + seed)
        dd = np.column_stack([rng.uniform(.1, .5, Cn), rng.uniform(.05, .3, Cn), rng.uniform(2, 60, Cn), rng.uniform(5, 50, Cn),
                              rng.uniform(10, 200, Cn), rng.uniform(.05, .4, Cn), rng.uniform(.5, 2, Cn), rng.uniform(.5, 2, Cn)])
        v2 = np.column_stack([rng.uniform(.01, .1, Cn), dd])
        tr = np.column_stack([rng.uniform(.05, .3, Cn), rng.uniform(.05, .3, Cn)] + [rng.uniform(-1, 1, Cn) for _ in range(4)])
        return dd, v2, tr, rng.uniform(1.0, 300.0, BINS), np.maximum(rng.random(BINS), 1e-15)
    _hold(rt, "dd_rates", lambda dd, DT: ops.dd_rates(dd, DT, 2, 2), _sets(torch, lambda s: (par(s)[0], par(s)[3])))
    _hold(rt, "ddv2_rates", lambda v2, DT: ops.ddv2_rates(v2, DT, 2, 2), _sets(torch, lambda s: (par(s)[1], par(s)[3])))
    _hold(rt, "trend_rates", lambda tr, x: ops.trend_rates(tr, x, False, False), _sets(torch, lambda s: (par(s)[2], par(s)[4])))

    def keiding(seed):
        rng = np.random.default_rng(90 + seed)
        return (0.05 + rng.random((Cn, BINS)), 0.05 + rng.random((Cn, BINS)), rng.integers(0, 40, BINS), rng.integers(0, 40, BINS),
                rng.uniform(1.0, 300.0, BINS))
    _hold(rt, "binned_keiding", lambda b, d, ns, ne, DT: ops.binned_keiding(b, d, ns, ne, DT), _sets(torch, keiding))


LOGLIK_SHAPES = {"small": (1025, 2, 7), "tiled": (1027, 17, 129)}


@case("lr_bd_loglik_batch")
def case_loglik(which):
    rt, torch, ops, _hip, lib = _gpu()
    n, Cn, nb = LOGLIK_SHAPES[which]
    plan = (C.c_int32 * 4)()
    _hip.check(lib.lr_bd_loglik_plan(n, nb, Cn, 0, plan), "lr_bd_loglik_plan")
    say("loglik %s: cb %d tiles %d H %d" % (which, plan[0], plan[1], plan[2]))
    end = float(T0 + nb // 2 + 0.5)
    _hold(rt, "loglik n %d C %d bins %d" % (n, Cn, nb), lambda ts, te, lam, mu, br: ops.bd_loglik_batch(ts, te, T0, lam, mu, 0, br, end),
          _sets(torch, lambda s: lineages(n, nb, s) + rates(Cn, nb, s)))


WALK_N, WALK_BINS, WALK_DRAWS = 513, 5, ("6", "25")


@case("lr_waic_pointwise")
def case_waic(draws):
    rt, torch, ops, _hip, lib = _gpu()
    S, end = int(draws), float(T0 + WALK_BINS // 2 + 0.5)
    _hold(rt, "waic draws %d" % S, lambda ts, te, lam, mu: ops.waic_pointwise(ts, te, T0, lam, mu, 2, None, end)[:2],
          _sets(torch, lambda s: lineages(WALK_N, WALK_BINS, s) + rates(S, WALK_BINS, s)[:2]))


@case("lr_loo_pointwise")
def case_loo(draws):
    rt, torch, ops, _hip, lib = _gpu()
    S, end = int(draws), float(T0 + WALK_BINS // 2 + 0.5)
    _hold(rt, "loo draws %d" % S, lambda ts, te, lam, mu: ops.loo_pointwise(ts, te, T0, lam, mu, 2, None, end)[:2],
          _sets(torch, lambda s: lineages(WALK_N, WALK_BINS, s) + rates(S, WALK_BINS, s)[:2]))


@case("lr_psis_rows")
def case_psis():
    rt, torch, ops, _hip, lib = _gpu()
    _hold(rt, "psis_rows 7 x 25", lambda L: ops.psis_loo_rows(L), _sets(torch, lambda s: (-3.0 + np.random.default_rng(4 + s).normal(size=(7, 25)) * 1.5,)))


@case("lr_simulate_bd")
def case_simulate_bd():
    rt, torch, ops, _hip, lib = _gpu()
    n_steps, cap = 12, 4096

    def call(lam, mu):
        ts, te = ops.alloc_output(cap, torch.float64, "cuda"), ops.alloc_output(cap, torch.float64, "cuda")
        cnt, trace = ops.alloc_output(4, torch.int64, "cuda"), ops.alloc_output(n_steps, torch.int64, "cuda")
        ws = ops.alloc_workspace(64, "cuda")
        abi("lr_simulate_bd", _hip.ptr(lam), _hip.ptr(mu), n_steps, 0, .4, .1, 50., 1., 3, cap, 5, _hip.ptr(ts), _hip.ptr(te), _hip.ptr(cnt),
            _hip.ptr(trace), _hip.ptr(ws), ws.numel())
        made = torch.arange(cap, device="cuda") < cnt[0]          # ts / te beyond counters[0] are not defined (no read-back)
        zero = torch.zeros((), dtype=torch.float64, device="cuda")
        return dict(ts=torch.where(made, ts, zero), te=torch.where(made, te, zero), counters=cnt[:3], trace=trace)
    _hold(rt, "simulate_bd", call, _sets(torch, lambda s: (np.full(n_steps, .3 - .05 * s), np.full(n_steps, .1 + .02 * s))))


SIM_SHAPE = (3, 4, 3, 1000)          # (n_reps, n_bins, steps_per_bin, capacity)


@case("lr_simulate_bd_batch")
def case_sim_batch():
    rt, torch, ops, _hip, lib = _gpu()
    R, nb, spb, cap = SIM_SHAPE
    _hold(rt, "simulate_bd_batch", lambda lam, mu: ops.simulate_bd_batch(lam, mu, spb, 5, 77, capacity=cap),
          _sets(torch, lambda s: (np.full((R, nb), (.3 - .05 * s) * spb), np.full((R, nb), .05 * spb))))


@case("lr_simulate_dd_batch")
def case_dd_batch():
    rt, torch, ops, _hip, lib = _gpu()
    R, nb, spb, cap = SIM_SHAPE

    def make(s):
        par = np.column_stack([np.full(R, (.3 - .05 * s) * spb), np.full(R, .1), np.full(R, 2.), np.full(R, 20.), np.full(R, 30.),
                               np.full(R, .05 * spb), np.ones(R), np.ones(R)])
        return par, np.arange(nb, dtype=float)
    _hold(rt, "simulate_dd_batch", lambda par, x: ops.simulate_dd_batch(par, x, spb, 5, 77, 2, 2, capacity=cap), _sets(torch, make))


@case("lr_shift_prior")
def case_shift_prior():
    """accumulate = 0 has no device input: the fills, the join and the return; accumulate = 1 adds to its outputs: they are
    the buffers, the pattern copied behind the delay"""
    rt, torch, ops, _hip, lib = _gpu()
    nb, reps = BINS, 64 * _hip.LR_SHIFT_PRIOR_BLOCKS + 1
    ordered(rt, lambda: tuple(ops.shift_prior(0.0, nb + 0.5, reps, seed=9)), (), (), (), "shift_prior accumulate 0")
    say("shift_prior accumulate 0 ok")
    sizes = (4, nb, _hip.LR_SHIFT_PRIOR_KCAP, _hip.LR_SHIFT_PRIOR_KCAP)
    a = [torch.arange(n, dtype=torch.int64, device="cuda") * 3 + 1000 * j for j, n in enumerate(sizes)]
    b = [torch.arange(n, dtype=torch.int64, device="cuda") * 5 + 7 for n in sizes]
    bufs = [torch.empty_like(x) for x in a]
    _hold(rt, "shift_prior accumulate 1", lambda *o: tuple(ops.shift_prior(0.0, nb + 0.5, reps, seed=9, out=ops.ShiftPrior(*o))), (a, b, bufs))


@case("lr_ppc_age")
def case_ppc_age():
    rt, torch, ops, _hip, lib = _gpu()
    _hold(rt, "ppc_age", lambda ts, te, mu: ops.ppc_age(ts, te, T0, mu, 5)[:3],
          _sets(torch, lambda s: lineages(WALK_N, WALK_BINS, s) + (rates(6, WALK_BINS, s)[1],)))


ADE_BINS = 12


def _classes(torch, ops, seed):
    ts, te = lineages(WALK_N, ADE_BINS, seed)
    dead, cens, _ = ops.ade_classes(dev(torch, ts), dev(torch, te), T0, ADE_BINS)
    torch.cuda.synchronize()
    return dead.cpu().numpy(), cens.cpu().numpy()


@case("lr_ade_classes", "lr_ade_profile")
def case_ade():
    rt, torch, ops, _hip, lib = _gpu()
    _hold(rt, "ade_classes", lambda ts, te: ops.ade_classes(ts, te, T0, ADE_BINS), _sets(torch, lambda s: lineages(WALK_N, ADE_BINS, s)))
    sh = dev(torch, np.array([0.5, 1.0, 1.5, 2.0]))
    _hold(rt, "ade_profile", lambda dead, cens, mu: ops.ade_profile(dead, cens, mu, sh),
          _sets(torch, lambda s: _classes(torch, ops, s) + (rates(6, ADE_BINS, s)[1],)))


@case("lr_adej_prepare", "lr_adej_loglik", "lr_adej_init", "lr_adej_steps")
def case_adej():
    """12 bins, 5 chains, 60 iterations in two launches"""
    rt, torch, ops, _hip, lib = _gpu()
    sh = dev(torch, np.array([0.7, 2.0]))

    def call(dead, cens, mu):
        data = ops.adej_prepare(dead, cens)
        ll, flag = ops.adej_loglik(data, mu, sh)
        state = ops.adej_init(data, 0.0, CHAINS, 9)
        first = ops.adej_steps(data, 0.0, state, 0, 25, 3, 9)
        rest = ops.adej_steps(data, 0.0, state, 25, 35, 3, 9)
        return dict(ll=ll, flag=flag, first=first, rest=rest, state=state)
    _hold(rt, "adej", call, _sets(torch, lambda s: _classes(torch, ops, s) + (rates(2, ADE_BINS, s)[1],)))


@case("lr_mlik_init", "lr_mlik_steps", "lr_mlik_estimate")
def case_mlik():
    """8 bins, three temperatures, two replicates, 60 iterations in two launches"""
    rt, torch, ops, _hip, lib = _gpu()
    nb, T, R = 8, 3, 2
    betas = (np.arange(T) / (T - 1.0)) ** (1.0 / 0.3)
    with np.errstate(divide="ignore"):
        scales = np.minimum(betas ** -0.5, 8.0)

    def make(seed):
        rng = np.random.default_rng(5 + seed)
        DT = np.abs(20.0 + np.cumsum(rng.normal(size=nb) * 3.0)) + 1.0 + rng.random(nb)
        return rng.poisson(0.3 * DT).astype(float), rng.poisson(0.2 * DT).astype(float), DT

    def call(n_spec, n_exti, DT):
        data = ops.MlikData(n_spec, n_exti, DT, -float(nb) - 3.0, -2.0, 2, 2, 0.15)
        state = ops.mlik_init(data, betas, scales, R, 9)
        first = ops.mlik_steps(data, betas, scales, state, 0, 25, 3, 9)
        rest = ops.mlik_steps(data, betas, scales, state, 25, 35, 3, 9)
        est = ops.mlik_estimate(rest, betas, row0=2)
        return dict(state=state, first=first, rest=rest, **est._asdict())
    _hold(rt, "mlik", call, _sets(torch, make))


SUMMARY_SAMPLES, SUMMARY_CHAINS = 40, 3


def _trace(torch, seed):
    """trace rows [40, 3, LR_TRACE_W] of a short run of the launch-based engine (abi_cases._engine_trace with a seed)"""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    ts, te, _ = synth.make_lineages(300, n_bins=30, n_shifts=3, seed=1)
    eng = ChainEngine(ts, te, SUMMARY_CHAINS, model=0, seed=3 + seed, s_freq=10, n_trace_slots=SUMMARY_SAMPLES, engine="launch")
    eng.init()
    eng.steps(10 * SUMMARY_SAMPLES)
    eng.check_status()
    tr = eng.trace[:SUMMARY_SAMPLES].clone()
    a, b = eng.cfg.start_time, eng.cfg.end_time
    eng.close()
    return tr, a, b


@case("lr_rtt_summary", "lr_col_summary", "lr_curve_summary", "lr_ess_summary")
def case_summaries():
    """40 samples by 3 chains, per chain; workspaces at the one-bin / one-column floor: the sort sits between the call's own
    launches once per pass"""
    rt, torch, ops, _hip, lib = _gpu()
    S, Cn, burn, pooled = SUMMARY_SAMPLES, SUMMARY_CHAINS, 0.2, False
    (tr_a, a, b), (tr_b, _, _) = _trace(torch, 0), _trace(torch, 1)
    nb = int(np.ceil(b - a)) - 1
    up = lambda x: (x + 255) // 256 * 256
    one = lib.lr_rtt_summary_workspace_bytes(S, Cn, a, a + 1.5, burn, int(pooled))          # (the floor: abi_cases.case_summaries)
    floor = one - up(8 * Cn * 2 * 2) + up(8 * Cn * 2 * (nb + 1))
    assert 0 < floor < lib.lr_rtt_summary_workspace_bytes(S, Cn, a, b, burn, int(pooled)) and nb >= 2
    _hold(rt, "rtt_summary, %d passes" % nb, lambda tr: tuple(ops.rtt_summary(tr, S, a, b, burn, pooled, floor)[1:4]),
          ([tr_a], [tr_b], [torch.empty_like(tr_a)]))

    def rows(seed):
        rng = np.random.default_rng(8 + seed)
        n = S * Cn
        par = np.column_stack([rng.uniform(.1, .5, n), rng.uniform(.05, .3, n), rng.uniform(2, 6, n), rng.uniform(5, 50, n),
                               rng.uniform(10, 200, n), rng.uniform(.05, .4, n), rng.uniform(.5, 2, n), rng.uniform(.5, 2, n)])
        r = np.cumsum(rng.normal(size=(S, Cn, 12)), axis=0) * 0.1 + rng.normal(size=(S, Cn, 12))
        r[:, :, 4:12] = par.reshape(S, Cn, 8)
        return (r,)
    cols = np.array([0, 11, 3], dtype=np.int32)
    cp = cols.ctypes.data_as(_hip.c_vp)
    floor_c = lib.lr_col_summary_workspace_bytes(S, Cn, 12, cp, 3, burn, int(pooled), 1)
    assert 0 < floor_c < lib.lr_col_summary_workspace_bytes(S, Cn, 12, cp, 3, burn, int(pooled), 0)
    _hold(rt, "col_summary, 3 passes", lambda r: tuple(ops.col_summary(r, S, cols, burn, pooled, floor_c)[:3]), _sets(torch, rows))
    aux = dev(torch, np.random.default_rng(9).uniform(10.0, 100.0, 5))
    floor_v = lib.lr_curve_summary_workspace_bytes(S, Cn, 12, 4, 1, 5, burn, int(pooled), 1)
    assert 0 < floor_v < lib.lr_curve_summary_workspace_bytes(S, Cn, 12, 4, 1, 5, burn, int(pooled), 0)
    _hold(rt, "curve_summary, a pass per bin", lambda r: ops.curve_summary(r, S, 1, aux, 2, 2, 4, burn, pooled, floor_v)[1], _sets(torch, rows))
    _hold(rt, "ess_summary", lambda r: tuple(ops.ess_summary(r, S, [0, 3, 11], 0.1, 16))[:8], _sets(torch, rows))


# ---- the engine --------------------------------------------------------------------------------
# "partitioned": 64 chains on the launch-based engine are two partitions, each pipelined: lr_mcmc_steps forks onto streams of
# its own, replays their hipGraphs there and joins them back through events
ENGINES = dict(A.ENGINES, partitioned=(dict(engine="launch"), 64, dict(persistent=0, pipelined=1, n_parts=2)))
ENGINE_RUNS = [(e, "unit", "rj") for e in ENGINES] + [("persistent4", "unit", "dd"), ("spec1", "unit", "trend")]
STEPS = (70, 1, 129)
assert sum(STEPS) == A.N_IT


def _decoy_lineages(ts, te):
    """the engine's own (sorted) lineages with most lifespans halved: as many lineages, the same first birth and last death,
    the same in-bin fractions, every time in range, in the engine's order (by birth bin, then death)"""
    ts, te = np.asarray(ts), np.asarray(te)
    frac = te - (np.ceil(te) - 1.0)
    assert np.all(frac == frac[0]), "the decoy is built for unit times"
    half = np.floor(ts + (te - ts) / 2.0) + frac[0]
    half = np.where(half <= ts, te, half)
    te2 = np.where(te >= te.max(), te, half)
    o1 = np.argsort(te2, kind="stable")
    o2 = np.argsort(np.floor(ts[o1]), kind="stable")
    order = o1[o2]
    ts2, te2 = ts[order], te2[order]
    assert ts2.min() == ts.min() and te2.max() == te.max() and np.all(te2 > ts2) and not np.array_equal(te2, te)
    return ts2, te2


def _outputs(eng, sampler, _hip):
    """the defined state that needs no read-back to delimit: every trace slot (all written after N_IT iterations) and
    the scalar rows; _engine_state (the lanes below K) is compared after the pass's synchronise"""
    S, I = eng.state_f64, eng.state_i32
    sc = S[:, _hip.ROW_SCALARS, :16] if sampler == "rj" else S[:, _hip.ROW_SCALARS][:, list(A.PARAM_SCALARS)]
    return dict(trace=eng.trace, scalars=sc, iscalars=I[:, _hip.IROW_SCALARS, :_hip.I_SLOT + 1])


@case("lr_mcmc_steps", "lr_mcmc_init", "lr_mcmc_restore", "lr_mcmc_status", "lr_mcmc_warnings", "lr_mcmc_time_scan", "lr_mcmc_time_steps")
def case_engine(name, times, sampler):
    """One engine, 200 iterations as steps(70); steps(1); steps(129), three ways: (i) lr_mcmc_init from a state given in
    device arrays, the arrays copied behind the delay; (ii) lr_mcmc_init(NULL) on a workspace of 0xFF and the lineages, both
    copied behind the delay; (iii) a checkpoint of another iteration in the workspace, this run's copied behind the delay,
    lr_mcmc_restore and the remaining steps - bit-identical to the uninterrupted run (ii).  The launch engine then runs the
    measurement hooks, the status and the warning word behind a restore on the busy stream."""
    rt, torch, ops, _hip, lib = _gpu()
    assert times == "unit" and os.environ.get("LR_SHARED_DEVICE", "0") != "1"
    label = "engine %s %s" % (name, sampler)
    P = _hip.ptr

    def make():
        eng = _make_engine(name, times, sampler, table=ENGINES)
        assert eng.workspace.numel() == eng.layout.total_bytes
        return eng

    def steps(eng, plan=STEPS):
        for n in plan:
            eng.steps(n)
        return _outputs(eng, sampler, _hip)

    def finish(eng, out):
        st = _engine_state(torch, eng, sampler)
        eng.close()
        return {k: _bits(torch, v) for k, v in st.items()}

    # what the cases are made from: the engine's sorted lineages, its time span, an initial state, two checkpoints
    eng = make()
    Cn = eng.n_chains
    ts_a, te_a = eng.ts.cpu().numpy(), eng.te.cpu().numpy()
    eng.init()
    eng.check_status()
    S0 = eng.state_f64.cpu().numpy()
    eng.steps(STEPS[0])
    eng.check_status()
    image_b = eng.workspace.clone()
    eng.steps(STEPS[1])
    eng.check_status()
    image_a = eng.workspace.clone()
    eng.steps(STEPS[2])
    whole = {k: _bits(torch, v) for k, v in _engine_state(torch, eng, sampler).items()}
    eng.close()

    # (i) a given state
    kmax = _hip.LR_KMAX
    if sampler == "rj":
        lo, hi = float(S0[0, _hip.ROW_TL, 0]), float(S0[0, _hip.ROW_TL, 1])
        assert lo != hi and np.all(S0[:, _hip.ROW_TL, :2] == [lo, hi])

        def given(s):
            L, M = np.zeros((Cn, kmax)), np.zeros((Cn, kmax))
            tL, tM = np.zeros((Cn, kmax + 1)), np.zeros((Cn, kmax + 1))
            L[:, :2], M[:, :1] = [.3 + .05 * s, .2], [.1 + .02 * s]
            tL[:, :3], tM[:, :2] = [lo, lo + (hi - lo) * (.4 + .1 * s), hi], [lo, hi]
            return L, M, tL, tM, np.full(Cn, 2, dtype=np.int32), np.full(Cn, 1, dtype=np.int32)
    else:
        npar = 8 if sampler == "dd" else 6

        def given(s):
            L = np.zeros((Cn, kmax))
            L[:, :npar] = S0[:, _hip.ROW_L, :npar]
            L[:, 0] *= 1.0 + 0.1 * s
            return (L,)
    a, b, bufs = _sets(torch, given)

    def init_given(eng):
        args = [P(x) for x in bufs] + [None] * (6 - len(bufs))
        _hip.check(eng._launch(lib.lr_mcmc_init, eng.handle, *args, kmax), "lr_mcmc_init")
        return steps(eng)
    ordered(rt, init_given, a, b, bufs, label + " (i) given state", blocking=BLOCKING, prepare=make, finish=finish)
    say(label, "(i) ok")

    # (ii) the CLI's initial state on a workspace of 0xFF
    ts_b, te_b = _decoy_lineages(ts_a, te_a)
    ff = torch.full_like(image_a, 0xFF)
    a, b = [dev(torch, ts_a), dev(torch, te_a), ff], [dev(torch, ts_b), dev(torch, te_b), ff]

    def init_cli(eng):
        _hip.check(eng._launch(lib.lr_mcmc_init, eng.handle, None, None, None, None, None, None, 0), "lr_mcmc_init")
        return steps(eng)
    want, _ = ordered(rt, init_cli, a, b, lambda eng: [eng.ts, eng.te, eng.workspace], label + " (ii) CLI state", blocking=BLOCKING,
                      prepare=make, finish=finish)
    got = {k[7:]: v for k, v in want.items() if k.startswith("finish ")}
    assert got == whole, "the run of (ii) is the uninterrupted run"
    say(label, "(ii) ok")

    # (iii) restore
    def resume(eng):
        _hip.check(eng._launch(lib.lr_mcmc_restore, eng.handle), "lr_mcmc_restore")
        eng.iterations = STEPS[0] + STEPS[1]
        return steps(eng, STEPS[2:])
    want, _ = ordered(rt, resume, [image_a], [image_b], lambda eng: [eng.workspace], label + " (iii) restore", blocking=BLOCKING,
                      prepare=make, finish=finish)
    got = {k[7:]: v for k, v in want.items() if k.startswith("finish ")}
    bad = _differs(got, whole)
    assert bad is None and set(got) == set(whole), "a run restored at iteration %d differs from the uninterrupted one: %s" % (sum(STEPS[:2]), bad)
    say(label, "(iii) ok: identical to the uninterrupted run")

    if name == "launch":
        # the entry points that block by their header sentences: behind a restore on the busy stream, in the order that
        # leaves a stream for the next to find busy - the hook's own delay; their order against the copy still holds
        def hooks(eng):
            _hip.check(eng._launch(lib.lr_mcmc_restore, eng.handle), "lr_mcmc_restore")
            eng.iterations = STEPS[0] + STEPS[1]
            eng.timed_steps(STEPS[2])
            eng.time_scan(2)
            assert eng.warnings() == 0
            eng.check_status()
            return _outputs(eng, sampler, _hip)
        want, _ = ordered(rt, hooks, [image_a], [image_b], lambda eng: [eng.workspace], label + " (iv) blocking hooks", blocking=BLOCKING,
                          prepare=make, finish=finish)
        got = {k[7:]: v for k, v in want.items() if k.startswith("finish ")}
        assert _differs(got, whole) is None, "timed steps are steps, a timed scan changes nothing"
        say(label, "(iv) ok")


@case()
def case_selftest():
    """the harness itself on the device: torch-only fakes, no library"""
    self_test(TorchRuntime)


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    # a hardware queue per stream that has work (the null stream, the side stream, the fakes' second stream, the engine's
    # partition streams): two streams that share one run in order, which would hide what the cases look for.  Read by the
    # HIP runtime when it starts - torch is imported by the case
    os.environ["GPU_MAX_HW_QUEUES"] = "16"
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
