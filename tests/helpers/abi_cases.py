"""The buffer contract of include/literate_hip.h, entry point by entry point (tests/test_hip_abi_contract.py runs every
case in a child process of its own, under a time limit):

    python tests/helpers/abi_cases.py CASE [ARG ...]

The header promises that the caller owns every buffer, that a workspace of exactly *_workspace_bytes bytes is enough, that
it may hold anything on entry, and that an argument error is returned before anything is written.  The value tests never
put the library there: the wrappers hand out a cached workspace of at least 1 MiB, the engine clears its own.  Here every
workspace and every output the wrappers allocate (literate_amd.ops.alloc_workspace / alloc_output, the one seam) is an
interior view of a larger allocation,

    [ 256 KiB of 0xA5 | payload of exactly the queried or documented size, filled with the run's byte | 256 KiB of 0xA5 ]

and a case runs three ways: (a) through plain ops, (b) guarded with fill 0x00, (c) guarded with fill 0xFF (NaN doubles, -1
integers).  contract() asserts, all of it exact:

  1. after the call and a synchronise both guards of every buffer still hold 0xA5 (torch.equal on the device);
  2. the defined extent of every output has the same bits in (a), (b) and (c) - (b) == (c) says that nothing uninitialised
     is read and no defined element is left unwritten.  The defined extent is the whole output unless the case passes
     `partial`, the header sentence the exception rests on;
  3. a second call on the same, now dirty buffers gives the same bits again.

refuses() asserts that an error return (a payload one byte short: LR_ERR_WORKSPACE; one argument error per entry point)
leaves the workspace payload, the outputs and all guards byte for byte what they were.

The harness itself (Guarded, contract, refuses) needs no GPU: tests/test_abi_contract_host.py runs it against fake entry
points on CPU tensors, and checks COVERS against the header and the shape tables against the host-only size queries."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

GUARD = 256 * 1024            # a multiple of 4096: the payload keeps torch's alignment
GUARD_BYTE = 0xA5
FILLS = (0x00, 0xFF)


def say(*a):
    print(*a)
    sys.stdout.flush()


# ------------------------------------------------------------------------------------------------
# the harness
# ------------------------------------------------------------------------------------------------
class ContractViolation(AssertionError):
    """kind: 'guard' (a byte outside a payload changed), 'fill' (the result depends on what the buffers held),
    'plain' (guarded and plain results differ), 'dirty' (a second call on the same buffers differs), 'error-wrote' (an
    error return changed a buffer), 'accepted' (the call did not return the error)."""

    def __init__(self, kind, msg):
        super().__init__("%s: %s" % (kind, msg))
        self.kind = kind


class _Buf:
    def __init__(self, kind, whole, nbytes, tensor):
        self.kind, self.whole, self.nbytes, self.tensor = kind, whole, nbytes, tensor

    @property
    def payload(self):
        return self.whole[GUARD:GUARD + self.nbytes]


class Guarded:
    """The two allocators of literate_amd.ops as guarded buffers.  short: bytes every WORKSPACE payload falls short of the
    size asked for.  replay = 0: hand out the buffers of the first pass again, in order, as they are."""

    def __init__(self, torch, fill, short=0):
        self.torch, self.fill, self.short = torch, int(fill), int(short)
        self.bufs, self.replay, self._guard = [], None, {}

    def _make(self, kind, nbytes, device, dtype, shape):
        torch = self.torch
        if self.replay is not None:
            assert self.replay < len(self.bufs), "the second call allocates more buffers than the first"
            b = self.bufs[self.replay]
            self.replay += 1
            assert (b.kind, b.nbytes, b.tensor.dtype) == (kind, nbytes, dtype), "the second call allocates other buffers"
            return b.tensor
        whole = torch.full((2 * GUARD + nbytes,), GUARD_BYTE, dtype=torch.uint8, device=device)
        whole[GUARD:GUARD + nbytes] = self.fill
        t = whole[GUARD:GUARD + nbytes].view(dtype).reshape(shape)
        assert (nbytes == 0 or t.data_ptr() == whole.data_ptr() + GUARD) and t.is_contiguous()
        self.bufs.append(_Buf(kind, whole, nbytes, t))
        return t

    def workspace(self, nbytes, device, zero=False, cached=False):
        n = max(int(nbytes) - self.short, 0)
        return self._make("ws", n, device, self.torch.uint8, (n,))

    def output(self, shape, dtype, device, zero=False):
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        n = int(np.prod(shape)) * self.torch.empty((), dtype=dtype).element_size()
        return self._make("out", n, device, dtype, shape)

    def _guard_ref(self, device):
        key = str(device)
        if key not in self._guard:
            self._guard[key] = self.torch.full((GUARD,), GUARD_BYTE, dtype=self.torch.uint8, device=device)
        return self._guard[key]

    def check_guards(self, label=""):
        torch = self.torch
        for i, b in enumerate(self.bufs):
            ref = self._guard_ref(b.whole.device)
            for side, g in (("before", b.whole[:GUARD]), ("behind", b.whole[GUARD + b.nbytes:])):
                if not torch.equal(g, ref):
                    at = int(torch.nonzero(g != ref)[0 if side == "behind" else -1])
                    off = at + 1 if side == "behind" else GUARD - at
                    raise ContractViolation("guard", "%s: buffer %d (%s, %d bytes): a byte %d bytes %s the payload changed"
                                            % (label, i, b.kind, b.nbytes, off, side))

    def snapshot(self):
        return [b.whole.clone() for b in self.bufs]

    def check_same(self, snap, label=""):
        assert len(snap) == len(self.bufs)
        for i, (b, s) in enumerate(zip(self.bufs, snap)):
            if not self.torch.equal(b.whole, s):
                at = int(self.torch.nonzero(b.whole != s)[0]) - GUARD
                raise ContractViolation("error-wrote", "%s: buffer %d (%s, %d bytes) changed at payload offset %d although the "
                                        "call returned an error" % (label, i, b.kind, b.nbytes, at))

    def check_untouched(self, label=""):
        """every buffer is still [guard | fill | guard]"""
        torch = self.torch
        pat = []
        for b in self.bufs:
            w = torch.full_like(b.whole, GUARD_BYTE)
            w[GUARD:GUARD + b.nbytes] = self.fill
            pat.append(w)
        self.check_same(pat, label)

    def output_bits(self):
        return [_bits(self.torch, b.tensor) for b in self.bufs if b.kind == "out"]


def _bits(torch, t):
    if t.numel() == 0:
        return b""
    # (through numpy: a one-element slice keeps its parent's stride, which a byte view of the tensor refuses)
    return np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()


def _tensors(torch, out):
    """the tensors of a result (a tensor, or a tuple / namedtuple / dict of them; what is no tensor is compared as it is)"""
    if isinstance(out, torch.Tensor):
        return {"0": out}, {}
    items = out.items() if isinstance(out, dict) else enumerate(out)
    ts, rest = {}, {}
    for k, v in items:
        if isinstance(v, torch.Tensor):
            ts[str(k)] = v
        else:
            rest[str(k)] = repr(np.asarray(v).tolist()) if v is not None else "None"
    return ts, rest


def _sync(torch):
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _compare(kind, label, got, want, what):
    for k in want:
        if got[k] != want[k]:
            a, b = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
            at = int(np.nonzero(a != b)[0][0]) if a.size == b.size else -1
            raise ContractViolation(kind, "%s: output %s: %s (%d bytes, first difference at byte %d)" % (label, k, what, b.size, at))


def contract(ns, torch, call, partial=None, label=""):
    """Run call() (a), (b), (c) and a second time on the dirty buffers of (b) and of (c); see the module docstring.  ns: the
    namespace whose alloc_workspace / alloc_output the call allocates through (literate_amd.ops; a fake's own on the CPU).
    call() returns the DEFINED extent of its outputs.  partial: None - then every output payload as a whole must agree
    too - or the header sentence by which part of an output is not defined.  Returns the plain result."""
    plain = call()
    _sync(torch)
    pt, prest = _tensors(torch, plain)
    want = {k: _bits(torch, v) for k, v in pt.items()}
    saved = ns.alloc_workspace, ns.alloc_output
    seen = {}
    try:
        for fill in FILLS:
            g = Guarded(torch, fill)
            ns.alloc_workspace, ns.alloc_output = g.workspace, g.output
            out = call()
            _sync(torch)
            g.check_guards("%s fill %#04x" % (label, fill))
            t, rest = _tensors(torch, out)
            assert rest == prest, (label, rest, prest)
            got, whole = {k: _bits(torch, v) for k, v in t.items()}, g.output_bits()
            g.replay = 0
            out2 = call()
            _sync(torch)
            assert g.replay == len(g.bufs), "the second call allocates fewer buffers than the first"
            g.check_guards("%s fill %#04x, second call" % (label, fill))
            t2, _ = _tensors(torch, out2)
            _compare("dirty", label, {k: _bits(torch, v) for k, v in t2.items()}, got,
                     "a second call on the same buffers (fill %#04x, not refilled) gives other bits" % fill)
            if partial is None:
                _compare("dirty", label, dict(enumerate(g.output_bits())), dict(enumerate(whole)),
                         "a second call on the same buffers (fill %#04x) leaves another payload" % fill)
            seen[fill] = (got, whole)
    finally:
        ns.alloc_workspace, ns.alloc_output = saved
    _compare("fill", label, seen[0xFF][0], seen[0x00][0], "the bits depend on what the buffers held (fill 0xFF against 0x00)")
    if partial is None:
        assert len(seen[0xFF][1]) == len(seen[0x00][1])
        _compare("fill", label, dict(enumerate(seen[0xFF][1])), dict(enumerate(seen[0x00][1])),
                 "part of the payload is left as it was (fill 0xFF against 0x00)")
    else:
        assert isinstance(partial, str) and len(partial) > 20, "partial is the header sentence the exception rests on"
    _compare("plain", label, seen[0x00][0], want, "guarded buffers give other bits than plain ops")
    return plain


def refuses(ns, torch, call, code, short=0, label="", entry=None):
    """call() must raise ValueError naming `code` (what _hip.check makes of a negative return; `entry`: and the entry point
    that returned it, not its size query), and every buffer it allocated through the seam - workspace payloads `short` bytes
    below what was asked for - must afterwards be [guard | fill | guard] byte for byte, for both fills."""
    saved = ns.alloc_workspace, ns.alloc_output
    try:
        for fill in FILLS:
            g = Guarded(torch, fill, short)
            ns.alloc_workspace, ns.alloc_output = g.workspace, g.output
            try:
                call()
            except ValueError as e:
                if code not in str(e) or (entry and not str(e).startswith(entry + ":")):
                    raise ContractViolation("accepted", "%s: expected %s from %s, got %s" % (label, code, entry or "the call", e))
            else:
                raise ContractViolation("accepted", "%s: the call did not return %s" % (label, code))
            _sync(torch)
            assert g.bufs, "%s: nothing was allocated through the seam" % label
            if short:
                assert any(b.kind == "ws" for b in g.bufs), "%s: no workspace was asked for" % label
            g.check_untouched("%s fill %#04x" % (label, fill))
    finally:
        ns.alloc_workspace, ns.alloc_output = saved


# ------------------------------------------------------------------------------------------------
# the case table: shapes (host data, also read by tests/test_abi_contract_host.py) and what each case covers
# ------------------------------------------------------------------------------------------------
LR_MAX_BINS, LR_KMAX = 4094, 32
COVERS = {}            # case name -> entry points of the header it runs


def case(*entry_points):
    def deco(fn):
        COVERS[fn.__name__[5:]] = entry_points
        return fn
    return deco


def max_bins(query):
    """the largest n_bins a size query still accepts (bisection: the limit is the planner's, not a constant of the header)"""
    lo, hi = 1, LR_MAX_BINS
    assert query(lo) > 0
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if query(mid) > 0:
            lo = mid
        else:
            hi = mid - 1
    return lo


def max_bins_model3(lib, n, C):
    """... of lr_bd_loglik_workspace_bytes for model 3's two table classes"""
    return max_bins(lambda nb: lib.lr_bd_loglik_workspace_bytes(n, nb, C, 3))


# lr_plan_scan's table classes (H = 40 / 72 / 136 / 264 and the generic scan above), both sides of each edge, and the
# bin counts at which the one-launch kernel's table no longer fits its 60 KiB of LDS (2 n_cls (n_bins + 2) 16 bytes)
LOGLIK_BINS = (1, 38, 39, 70, 71, 128, 129, 256, 257)
LOGLIK_SMALL_LDS_EDGE = {1: (1918, 1919), 2: (958, 959)}          # by n_cls


def loglik_shapes(lib, model, tiled):
    """(n, C, n_bins) of lr_bd_loglik_batch.  tiled = False: the process runs with the one-launch kernel allowed (C <= 64
    takes it, C = 65 the tiled path); True: LR_LOGLIK_SMALL=0, every shape takes the tiled path."""
    n_cls = 2 if model == 3 else 1
    out = []
    if not tiled:
        out += [(n, c, 7) for n in (1, 2, 1025) for c in (1, 64)]                  # the one-launch kernel
        out += [(n, 65, 7) for n in (1, 3, 513, 1027)]                             # more than 64 chains: tiled
        out += [(513, 65, nb) for nb in LOGLIK_BINS]                               # (sixteen chains per pass up to 128 bins)
        out += [(257, 2, nb) for nb in LOGLIK_SMALL_LDS_EDGE[n_cls]]               # the one-launch kernel's LDS edge
        top = LR_MAX_BINS if model != 3 else max_bins_model3(lib, 513, 65)
        out += [(513, 65, top), (257, 2, LR_MAX_BINS if model != 3 else max_bins_model3(lib, 257, 2))]
    else:
        out += [(513, c, 7) for c in (1, 2, 3, 4, 8)]                              # cb = 1, 2, 4, 8
        out += [(1027, c, nb) for c in (9, 17) for nb in (7, 128, 129)]            # the sixteen-chain kernel and its edge
        out += [(3, c, nb) for c in (1, 2, 9) for nb in LOGLIK_BINS]
    return out


# lr_ub_plan (csrc/lr_stats.hip): the histograms take (28 W + 16) << rshift bytes of LDS, rshift = 5 lowered until that
# is at most 144 KiB; above 64 KiB the launch raises the kernel's LDS attribute, up to 76 KiB two blocks share a CU.
# Both sides of every edge: 72|73 (64 KiB, 32 copies), 86|87 (76 KiB), 164|165 (16 copies), 173|174 (76 KiB), 328|329 (8),
# 346|347, 657|658 (4), 694|695, 1316|1317 (2), 1389|1390, 2632|2633 (1 copy: the block's 40 W + 32 bytes of column totals are
# then the larger need, above 76 KiB throughout).
BIN_UNIT_BINS = (1, 72, 73, 86, 87, 164, 165, 173, 174, 328, 329, 346, 347, 657, 658, 694, 695, 1316, 1317, 1389, 1390,
                 2632, 2633, LR_MAX_BINS)


def ub_plan(W):
    """(copies, LDS bytes) of lr_ub_plan, restated"""
    r = 5
    while ((28 * W + 16) << r) > 144 * 1024 and r > 0:
        r -= 1
    return 1 << r, max((28 * W + 16) << r, (5 * W + 4) * 8)


def ub_edges():
    out = {1, LR_MAX_BINS}
    for W in range(1, LR_MAX_BINS):
        (c0, l0), (c1, l1) = ub_plan(W), ub_plan(W + 1)
        if c0 != c1 or any((l0 <= k) != (l1 <= k) for k in (64 * 1024, 76 * 1024)):
            out |= {W, W + 1}
    return tuple(sorted(out))


BIN_EVENTS_SHAPES = [(n, w) for n in (1, 513, 4099) for w in (1, 2, 65, LR_MAX_BINS)]
BIN_UNIT_N = (1, 4099)
# (n, n_bins, draws) per model of lr_waic_pointwise: a tile holds 512 lineages; a draw's table takes 32 n_cls (n_bins + 2)
# bytes: up to 32 KiB several draws per LDS chunk, up to 76 KiB one draw and two buffers, above that one buffer
WAIC_BINS = {0: (5, 1022, 1023, 2430, 2431, LR_MAX_BINS), 2: (5, 1022, 1023, 2430, 2431, LR_MAX_BINS),
             3: (5, 510, 511, 1214, 1215, None)}          # None: the most lr_waic_workspace_bytes accepts
WAIC_N, WAIC_DRAWS, WAIC_SLICES = (511, 513), 6, ("1", "3")
LOO_DRAWS = (2, 24, 25, 8192)          # M = 0, 4 (below 5: nothing is smoothed), 5, 272 (a sort padded to 8192 = itself)
LOO_N, LOO_BINS = 7, 5
SIMBATCH_SHAPES = [(1, 4, 3, 1000), (513, 4, 3, 1000), (3, 2, 1, 40000)]      # (n_reps, n_bins, steps_per_bin, capacity)
ESS_ROWS = (4, 16384, 16385)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
T0 = 3.0


def lineages(n, n_bins, seed=0):
    rng = np.random.default_rng(1000003 * seed + 7919 * n + n_bins)
    ts = T0 - 1.0 + rng.random(n) * (n_bins + 1.5)
    te = ts + rng.random(n) * n_bins * 0.6 + 1e-3
    return ts, te


def rates(C, n_bins, seed=0):
    rng = np.random.default_rng(31 * seed + 1009 * C + n_bins)
    return 0.05 + rng.random((C, n_bins)), 0.05 + rng.random((C, n_bins)), 0.5 + 4.0 * rng.random(n_bins)


def _gpu():
    import torch
    assert torch.cuda.is_available(), "the cases need an MI355X"
    from literate_amd import _hip, ops
    return torch, ops, _hip, _hip.load()


def abi(name, *args):
    """an entry point called directly on torch's current stream (an argument error with every pointer valid: the wrappers
    would raise on their own, ask the size query first, or pass the NULL of an empty tensor)"""
    from literate_amd import _hip
    _hip.check(_hip.launch(getattr(_hip.load(), name), "cuda", *args), name)


def dev(torch, x, dtype=None, offset=0):
    """a device tensor of x; offset: elements the data starts behind an aligned allocation (8-byte-offset ts / te)"""
    t = torch.as_tensor(np.ascontiguousarray(x), dtype=dtype)
    if not offset:
        return t.cuda()
    big = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
    big[offset:] = t.cuda()
    out = big[offset:]
    assert out.data_ptr() % 16 == (8 * offset) % 16 and out.is_contiguous()
    return out


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
@case("lr_bd_loglik_batch", "lr_bd_loglik_workspace_bytes")
def case_loglik(model, tiled="0"):
    """lr_bd_loglik_batch under one model: every shape of loglik_shapes, ts / te aligned and 8 bytes off; out_loglik [C]
    and the workspace between guards; one byte short and a fractional t0 refused"""
    model, tiled = int(model), tiled == "1"
    assert (os.environ.get("LR_LOGLIK_SMALL") == "0") == tiled, "the test sets LR_LOGLIK_SMALL for the child"
    torch, ops, _hip, lib = _gpu()
    plan = (C.c_int32 * 4)()
    for n, Cn, nb in loglik_shapes(lib, model, tiled):
        ts, te = lineages(n, nb)
        lam, mu, br = rates(Cn, nb)
        end = float(T0 + nb // 2 + 0.5)
        _hip.check(lib.lr_bd_loglik_plan(n, nb, Cn, model, plan), "lr_bd_loglik_plan")
        lam_d, mu_d, br_d = dev(torch, lam), dev(torch, mu), dev(torch, br)
        for off in (0, 1):
            ts_d, te_d = dev(torch, ts, offset=off), dev(torch, te, offset=off)
            label = "loglik model %d n %d C %d bins %d offset %d (cb %d, tiles %d, H %d)" % (model, n, Cn, nb, 8 * off, plan[0], plan[1], plan[2])

            def call(t0=T0):
                return ops.bd_loglik_batch(ts_d, te_d, t0, lam_d, mu_d, model, br_d, end)
            contract(ops, torch, call, label=label)
        refuses(ops, torch, call, "LR_ERR_WORKSPACE", short=1, label=label, entry="lr_bd_loglik_batch")
        say(label, "ok")
    refuses(ops, torch, lambda: call(T0 + 0.5), "LR_ERR_T0", label="loglik t0", entry="lr_bd_loglik_batch")


@case("lr_bin_events", "lr_bin_events_workspace_bytes")
def case_bin_events():
    """lr_bin_events on windows that are not the unit bins (odd widths, overlapping)"""
    torch, ops, _hip, lib = _gpu()
    for n, w in BIN_EVENTS_SHAPES:
        ts, te = lineages(n, 40)
        rng = np.random.default_rng(w)
        lo = T0 - 2.0 + rng.random(w) * 40.0
        hi = lo + 0.25 + rng.random(w) * 7.0
        ts_d, te_d, lo_d, hi_d = [dev(torch, x) for x in (ts, te, lo, hi)]
        label = "bin_events n %d windows %d" % (n, w)

        def call():
            return ops.bin_events(ts_d, te_d, lo_d, hi_d)
        contract(ops, torch, call, label=label)
        refuses(ops, torch, call, "LR_ERR_WORKSPACE", short=1, label=label, entry="lr_bin_events")
        say(label, "ok")

    def no_window():
        o = [ops.alloc_output(4, torch.int64, "cuda") for _ in range(3)]
        ws = ops.alloc_workspace(4096, "cuda")
        abi("lr_bin_events", P(ts_d), P(te_d), n, P(lo_d), P(hi_d), 0, P(o[0]), P(o[1]), P(o[2]), P(ws), ws.numel())
    P = _hip.ptr
    refuses(ops, torch, no_window, "LR_ERR_SIZE", label="bin_events no window", entry="lr_bin_events")


@case("lr_bin_unit_events", "lr_bin_unit_events_workspace_bytes")
def case_bin_unit():
    """lr_bin_unit_events at every n_bins where lr_ub_plan changes its copies or crosses an LDS threshold"""
    torch, ops, _hip, lib = _gpu()
    assert ub_edges() == BIN_UNIT_BINS, ub_edges()
    for nb in BIN_UNIT_BINS:
        for n in BIN_UNIT_N:
            ts, te = lineages(n, nb)
            ts_d, te_d = dev(torch, ts), dev(torch, te)
            label = "bin_unit n %d bins %d (copies %d, LDS %d)" % ((n, nb) + ub_plan(nb))

            def call(t0=T0):
                return ops.bin_unit_events(ts_d, te_d, t0, nb)
            contract(ops, torch, call, label=label)
        refuses(ops, torch, call, "LR_ERR_WORKSPACE", short=1, label=label, entry="lr_bin_unit_events")
        say(label, "ok")
    refuses(ops, torch, lambda: call(T0 + 0.25), "LR_ERR_T0", label="bin_unit t0", entry="lr_bin_unit_events")


def _segments(C, kmax, n_bins, rng):
    """rates [C, kmax], ascending times [C, kmax + 1] over [0, n_bins], K [C] in 1 .. kmax (1 and kmax among them)"""
    K = rng.integers(1, kmax + 1, C)
    K[0], K[-1] = 1, kmax
    r = 0.05 + rng.random((C, kmax))
    t = np.zeros((C, kmax + 1))
    for c in range(C):
        t[c, 1:K[c]] = np.sort(rng.random(K[c] - 1)) * n_bins
        t[c, K[c]] = float(n_bins)
    return r, t, K.astype(np.int32)


@case("lr_expand_rates", "lr_log_priors", "lr_rj_propose_score")
def case_chain_maps():
    """the per-chain kernels without a workspace: C at the block edges, kmax 1, 16 and LR_KMAX, every move kind of
    lr_rj_propose_score with K at its least and at kmax - 1"""
    torch, ops, _hip, lib = _gpu()
    rng = np.random.default_rng(5)
    for Cn in (1, 2, 65):
        for kmax in (1, 16, LR_KMAX):
            r, t, K = _segments(Cn, kmax, 129, rng)
            r_d, t_d, K_d = dev(torch, r), dev(torch, t), dev(torch, K)
            for nb in (1, 127, 128, 129):
                for mode in (0, 1):
                    contract(ops, torch, lambda: ops.expand_rates(r_d, t_d, K_d, nb, mode),
                             label="expand_rates C %d kmax %d bins %d mode %d" % (Cn, kmax, nb, mode))
            g = dev(torch, 0.5 + rng.random(Cn))
            p = dev(torch, 0.5 + rng.random(Cn))
            for poi in (None, p):
                contract(ops, torch, lambda: ops.log_priors(r_d, K_d, 2.0, g, poi), label="log_priors C %d kmax %d" % (Cn, kmax))
            if kmax < 2:
                continue
            # move 0 multiplier, 1 add a shift (K + 1 <= kmax), 2 remove one (K >= 2)
            for move, Ks in ((0, (1, kmax - 1)), (1, (1, kmax - 1)), (2, (2, kmax - 1))):
                for k in Ks:
                    Kc = np.full(Cn, k, dtype=np.int32)
                    tt = np.zeros((Cn, kmax + 1))
                    tt[:, :k + 1] = np.linspace(0.0, 100.0, k + 1)
                    u = rng.uniform(0.05, 0.95, (Cn, 2 * kmax))
                    if move == 0:
                        u[:, :kmax] = (u[:, :kmax] < 0.5)
                    idx = np.full(Cn, {0: 0, 1: k - 1, 2: k - 1}[move], dtype=np.int32)
                    a = [dev(torch, x) for x in (r, tt, Kc, np.full(Cn, move, dtype=np.int32), idx, u)]
                    contract(ops, torch, lambda: ops.rj_propose_score(*a),
                             label="rj_propose_score C %d kmax %d move %d K %d" % (Cn, kmax, move, k))
        say("chain maps C %d ok" % Cn)
    P = _hip.ptr

    def no_bins():
        out = ops.alloc_output((Cn, 4), torch.float64, "cuda")
        abi("lr_expand_rates", P(r_d), P(t_d), P(K_d), kmax, Cn, 0, 0, P(out))
    refuses(ops, torch, no_bins, "LR_ERR_SIZE", label="expand_rates no bins", entry="lr_expand_rates")
    one = [dev(torch, x) for x in (r[:, :1], t[:, :2], np.ones(Cn, np.int32), np.zeros(Cn, np.int32), np.zeros(Cn, np.int32), u[:, :2])]
    refuses(ops, torch, lambda: ops.rj_propose_score(*one), "LR_ERR_SIZE", label="rj_propose_score kmax 1", entry="lr_rj_propose_score")
    wide = dev(torch, np.full((2, 64), 0.5))
    refuses(ops, torch, lambda: ops.log_priors(wide, K_d[:2], 2.0, g[:2], None), "LR_ERR_SIZE", label="log_priors kmax 64", entry="lr_log_priors")


@case("lr_dd_rates", "lr_ddv2_rates", "lr_trend_rates", "lr_binned_keiding")
def case_rate_maps():
    """the per-bin rate maps and the binned Keiding halves: C in 1, 2, 65, n_bins around the 128-thread block"""
    torch, ops, _hip, lib = _gpu()
    rng = np.random.default_rng(6)
    for Cn in (1, 2, 65):
        dd = np.column_stack([rng.uniform(.1, .5, Cn), rng.uniform(.05, .3, Cn), rng.uniform(2, 60, Cn), rng.uniform(5, 50, Cn),
                              rng.uniform(10, 200, Cn), rng.uniform(.05, .4, Cn), rng.uniform(.5, 2, Cn), rng.uniform(.5, 2, Cn)])
        v2 = np.column_stack([rng.uniform(.01, .1, Cn), dd[:, 0], dd[:, 1], dd[:, 2], dd[:, 3], dd[:, 4], dd[:, 5], dd[:, 6], dd[:, 7]])
        tr = np.column_stack([rng.uniform(.05, .3, Cn), rng.uniform(.05, .3, Cn)] + [rng.uniform(-1, 1, Cn) for _ in range(4)])
        for nb in (1, 127, 128, 129):
            DT = dev(torch, rng.uniform(1.0, 300.0, nb))
            trend = dev(torch, np.maximum(rng.random(nb), 1e-15))
            label = "C %d bins %d" % (Cn, nb)
            for mb, md in ((2, 2), (0, -1), (1, 1)):
                contract(ops, torch, lambda: ops.dd_rates(dd, DT, mb, md), label="dd_rates %s m %d %d" % (label, mb, md))
                contract(ops, torch, lambda: ops.ddv2_rates(v2, DT, mb, md), label="ddv2_rates %s m %d %d" % (label, mb, md))
            for cb, cd in ((False, False), (True, True)):
                contract(ops, torch, lambda: ops.trend_rates(tr, trend, cb, cd), label="trend_rates %s const %d %d" % (label, cb, cd))
            b, d = dev(torch, 0.05 + rng.random((Cn, nb))), dev(torch, 0.05 + rng.random((Cn, nb)))
            ns_, ne_ = dev(torch, rng.integers(0, 40, nb)), dev(torch, rng.integers(0, 40, nb))
            contract(ops, torch, lambda: ops.binned_keiding(b, d, ns_, ne_, DT), label="binned_keiding " + label)
        say("rate maps C %d ok" % Cn)
    refuses(ops, torch, lambda: ops.dd_rates(dd, DT, 5, 2), "LR_ERR_MODEL", label="dd_rates m_birth 5", entry="lr_dd_rates")
    refuses(ops, torch, lambda: ops.ddv2_rates(v2, DT, 2, 3), "LR_ERR_MODEL", label="ddv2_rates m_death 3", entry="lr_ddv2_rates")

    # n_bins = 0 with every pointer valid: the wrappers would pass the NULL of an empty tensor, so these two go to the ABI
    def trend_no_bins():
        o = [ops.alloc_output((Cn, 4), torch.float64, "cuda") for _ in range(2)]
        a = dev(torch, tr)
        _hip.check(_hip.launch(lib.lr_trend_rates, a.device, _hip.ptr(a), _hip.ptr(trend), 0, Cn, 0, 0, _hip.ptr(o[0]), _hip.ptr(o[1])), "lr_trend_rates")

    def keiding_no_bins():
        o = [ops.alloc_output(Cn, torch.float64, "cuda") for _ in range(2)]
        _hip.check(_hip.launch(lib.lr_binned_keiding, b.device, _hip.ptr(b), _hip.ptr(d), _hip.ptr(ns_), _hip.ptr(ne_), _hip.ptr(DT), 0, Cn,
                               _hip.ptr(o[0]), _hip.ptr(o[1])), "lr_binned_keiding")
    refuses(ops, torch, trend_no_bins, "LR_ERR_SIZE", label="trend_rates no bins", entry="lr_trend_rates")
    refuses(ops, torch, keiding_no_bins, "LR_ERR_SIZE", label="binned_keiding no bins", entry="lr_binned_keiding")


@case("lr_shift_prior")
def case_shift_prior():
    """lr_shift_prior: accumulate = 0 starts from the fill byte, accumulate = 1 from a known pattern and must give
    pattern + counts"""
    torch, ops, _hip, lib = _gpu()
    blocks = _hip.LR_SHIFT_PRIOR_BLOCKS
    for nb in (1, 50):
        for reps in (1, 64 * blocks + 1):
            a, b = 0.0, nb + 0.5
            label = "shift_prior bins %d replicates %d" % (nb, reps)
            base = contract(ops, torch, lambda: tuple(ops.shift_prior(a, b, reps, seed=9)), label=label)
            assert int(base[2].sum()) == reps, "every replicate draws a K"
            sizes = (4, nb, _hip.LR_SHIFT_PRIOR_KCAP, _hip.LR_SHIFT_PRIOR_KCAP)

            def add():
                out = ops.ShiftPrior(*[ops.alloc_output(s, torch.int64, "cuda") for s in sizes])
                for j, t in enumerate(out):
                    t.copy_(torch.arange(t.numel(), dtype=torch.int64, device="cuda") * 3 + 1000 * j)
                return tuple(ops.shift_prior(a, b, reps, seed=9, out=out))
            got = contract(ops, torch, add, label=label + " accumulate")
            for j, (g, c) in enumerate(zip(got, base)):
                want = torch.arange(g.numel(), dtype=torch.int64, device="cuda") * 3 + 1000 * j + c
                assert torch.equal(g, want), (label, j)
            say(label, "ok")
    refuses(ops, torch, lambda: ops.shift_prior(0.0, 50.5, 0), "LR_ERR_SIZE", label="shift_prior no replicate", entry="lr_shift_prior")


SIM_PARTIAL = ("Outputs: ts/te [capacity] = birth / death STEP of every lineage (te = n_steps: extant), counters[0] = lineages, "
               "counters[1] = living at the end, counters[2] = 1 if `capacity` was hit: ts / te beyond counters[0] and "
               "counters[3] are not defined")


def _sim_bd(torch, ops, _hip, lib, mode, n_start, capacity, n_steps, with_trace, lam=None, mu=None, ws_bytes=64, seed=5):
    """lr_simulate_bd on buffers from the seam -> the defined extent (ts[:n], te[:n], counters[:3], trace)"""
    ts = ops.alloc_output(capacity, torch.float64, "cuda")
    te = ops.alloc_output(capacity, torch.float64, "cuda")
    cnt = ops.alloc_output(4, torch.int64, "cuda", zero=True)
    trace = ops.alloc_output(n_steps, torch.int64, "cuda", zero=True) if with_trace else None
    ws = ops.alloc_workspace(ws_bytes, "cuda", zero=True)
    rc = _hip.launch(lib.lr_simulate_bd, ts.device, _hip.ptr(lam), _hip.ptr(mu), n_steps, mode, .4, .1, 50., 1., n_start, capacity, seed,
                     _hip.ptr(ts), _hip.ptr(te), _hip.ptr(cnt), _hip.ptr(trace), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_simulate_bd")
    n = int(cnt[0])
    out = dict(ts=ts[:n], te=te[:n], counters=cnt[:3])
    if with_trace:
        out["trace"] = trace
    return out


@case("lr_simulate_bd")
def case_simulate_bd():
    """lr_simulate_bd: modes 0, 1 and 2, no room at all (capacity = n_start), a run that ends exactly at its capacity,
    alive_trace NULL and given, a 64-byte workspace of 0xFF (fill (c)); 63 bytes refused"""
    torch, ops, _hip, lib = _gpu()
    n_steps = 12
    lam, mu = dev(torch, np.full(n_steps, .3)), dev(torch, np.full(n_steps, .1))
    for mode in (0, 1, 2):
        kw = dict(lam=lam, mu=mu) if mode == 0 else {}
        free = _sim_bd(torch, ops, _hip, lib, mode, 3, 4096, n_steps, True, **kw)
        created = int(free["counters"][0])
        assert 3 < created < 4096 and int(free["counters"][2]) == 0, created
        for cap in (3, created, created - 1, 4096):
            for with_trace in (True, False):
                label = "simulate_bd mode %d capacity %d (the free run makes %d) trace %d" % (mode, cap, created, with_trace)
                got = contract(ops, torch, lambda: _sim_bd(torch, ops, _hip, lib, mode, 3, cap, n_steps, with_trace, **kw),
                               partial=SIM_PARTIAL, label=label)
                assert int(got["counters"][0]) == min(cap, created) and int(got["counters"][2]) == (1 if cap < created else 0), label
                if cap >= created:
                    assert torch.equal(got["ts"], free["ts"]) and torch.equal(got["te"], free["te"])
        say("simulate_bd mode %d ok (%d lineages)" % (mode, created))
    refuses(ops, torch, lambda: _sim_bd(torch, ops, _hip, lib, 0, 3, 64, n_steps, True, lam=lam, mu=mu, ws_bytes=64), "LR_ERR_WORKSPACE",
            short=1, label="simulate_bd 63 bytes", entry="lr_simulate_bd")
    refuses(ops, torch, lambda: _sim_bd(torch, ops, _hip, lib, 5, 3, 64, n_steps, True, lam=lam, mu=mu), "LR_ERR_MODEL", label="simulate_bd mode 5",
            entry="lr_simulate_bd")
    # the wrapper itself (its zeros are its own choice, not the library's need)
    contract(ops, torch, lambda: ops.simulate_bd(3, n_steps, 5, lam, mu, capacity=4096), partial=SIM_PARTIAL, label="ops.simulate_bd")


BATCH_PARTIAL = ("A replicate that would exceed it sets its overflow flag; its counts are then unspecified and no other replicate "
                 "is affected: of an overflowing replicate only the flag is compared")


def _batch_defined(torch, counts, totals):
    ok = totals[:, 2] == 0
    return dict(counts=counts[ok], totals=totals[ok], flags=totals[:, 2].clone())


def _batch_cases(torch, ops, name, run, refuse, code):
    """the shapes both batched simulators share; run(R, nb, spb, n_start, capacity, growth [R]) -> (counts, totals)"""
    for R, nb, spb, cap in SIMBATCH_SHAPES[:2]:
        g = np.full(R, 0.3)
        label = "%s replicates %d" % (name, R)
        got = contract(ops, torch, lambda: _batch_defined(torch, *run(R, nb, spb, 5, cap, g)), partial=BATCH_PARTIAL, label=label)
        assert not got["flags"].any()
        contract(ops, torch, lambda: run(R, nb, spb, 5, cap, g), label=label + " (whole outputs)")
        refuses(ops, torch, lambda: run(R, nb, spb, 5, cap, g), "LR_ERR_WORKSPACE", short=1, label=label, entry="lr_" + name)
        say(label, "ok")
    # 16000 founders fit the LDS part of the list (LR_SIMBATCH_LDS_SLOTS = 16384); at 0.5 births and 0.05 deaths per lineage
    # and step the first step outgrows it into the workgroup's slice of the workspace (~23200 living, then ~33600 of the
    # 40000 the capacity allows): two steps in all
    R, nb, spb, cap = SIMBATCH_SHAPES[2]
    g = np.full(R, 0.5)
    got = contract(ops, torch, lambda: _batch_defined(torch, *run(R, nb, spb, 16000, cap, g)), partial=BATCH_PARTIAL, label=name + " beyond LDS")
    assert not got["flags"].any() and int(got["counts"][:, 2, 1].min()) > 16384, got["counts"][:, 2]
    refuses(ops, torch, lambda: run(R, nb, spb, 16000, cap, g), "LR_ERR_WORKSPACE", short=1, label=name + " beyond LDS",
            entry="lr_" + name)
    say(name, "beyond LDS ok, living at the second bin's start", got["counts"][:, 2, 1].tolist())
    # an overflowing replicate between two ordinary ones
    calm, wild = np.array([.05, .05, .05]), np.array([.05, .9, .05])
    a = contract(ops, torch, lambda: _batch_defined(torch, *run(3, 4, 3, 5, 50, calm)), partial=BATCH_PARTIAL, label=name + " calm")
    b = contract(ops, torch, lambda: _batch_defined(torch, *run(3, 4, 3, 5, 50, wild)), partial=BATCH_PARTIAL, label=name + " overflow")
    assert a["flags"].tolist() == [0, 0, 0] and b["flags"].tolist() == [0, 1, 0], (a["flags"], b["flags"])
    assert torch.equal(a["counts"][[0, 2]], b["counts"]) and torch.equal(a["totals"][[0, 2]], b["totals"]), "the neighbours keep their bits"
    refuses(ops, torch, refuse, code, label=name + " " + code, entry="lr_" + name)
    say(name, "overflow between two ordinary replicates ok")


@case("lr_simulate_bd_batch", "lr_simulate_bd_batch_workspace_bytes")
def case_sim_batch():
    torch, ops, _hip, lib = _gpu()

    def run(R, nb, spb, n_start, cap, growth):
        lam = np.repeat(growth[:, None] * spb, nb, axis=1)
        return ops.simulate_bd_batch(lam, np.full((R, nb), .05 * spb), spb, n_start, 77, capacity=cap)
    P = _hip.ptr

    def no_step():
        ra = dev(torch, np.full((3, 4), .1))
        n0 = dev(torch, np.full(3, 5, dtype=np.int64))
        counts, totals = ops.alloc_output((3, 4, 4), torch.int64, "cuda"), ops.alloc_output((3, 4), torch.int64, "cuda")
        ws = ops.alloc_workspace(4096, "cuda")
        abi("lr_simulate_bd_batch", P(ra), P(ra), 3, 4, 0, P(n0), 50, 1, P(counts), P(totals), P(ws), ws.numel())
    _batch_cases(torch, ops, "simulate_bd_batch", run, no_step, "LR_ERR_SIZE")


@case("lr_simulate_dd_batch", "lr_simulate_dd_batch_workspace_bytes")
def case_dd_batch():
    torch, ops, _hip, lib = _gpu()

    def run(R, nb, spb, n_start, cap, growth, mb=0, md=0):
        # m_birth = m_death = 0: the constant rates l_max, m_max; the rate map itself runs in the last case below
        par = np.column_stack([growth * spb, np.full(R, .1), np.full(R, 2.), np.full(R, 20.), np.full(R, 30.), np.full(R, .05 * spb),
                               np.ones(R), np.ones(R)])
        return ops.simulate_dd_batch(par, np.arange(nb, dtype=float), spb, n_start, 77, mb, md, capacity=cap)
    g = np.full(3, 0.3)
    _batch_cases(torch, ops, "simulate_dd_batch", run, lambda: run(3, 4, 3, 5, 50, g, 5, 2), "LR_ERR_MODEL")
    got = contract(ops, torch, lambda: run(3, 4, 3, 5, 1000, g, 2, 2), label="simulate_dd_batch DDRate map")
    assert not got[1][:, 2].any()


def _engine_trace(torch, n_slots=20, C=3):
    """trace rows [n_slots, C, LR_TRACE_W] of a short run of the launch-based engine: valid rows for lr_rtt_summary"""
    from literate_amd import synth
    from literate_amd.engine import ChainEngine
    ts, te, _ = synth.make_lineages(300, n_bins=30, n_shifts=3, seed=1)
    eng = ChainEngine(ts, te, C, model=0, seed=3, s_freq=10, n_trace_slots=n_slots, engine="launch")
    eng.init()
    eng.steps(10 * n_slots)
    eng.check_status()
    tr = eng.trace[:n_slots].clone()
    a, b = eng.cfg.start_time, eng.cfg.end_time
    eng.close()
    return tr, a, b


@case("lr_rtt_summary", "lr_rtt_summary_workspace_bytes", "lr_col_summary", "lr_col_summary_workspace_bytes", "lr_curve_summary",
      "lr_curve_summary_workspace_bytes")
def case_summaries():
    """the three chunking summaries: the whole problem in one pass and the one-per-pass floor, pooled and per chain, and the
    smallest legal group (n_in = 2); one byte below the floor refused"""
    torch, ops, _hip, lib = _gpu()
    trace, a, b = _engine_trace(torch)
    nb = int(np.ceil(b - a)) - 1
    up = lambda x: (x + 255) // 256 * 256
    for S, pooled, burn in ((20, True, 0.2), (20, False, 0.2), (2, False, 0.0), (2, True, 0.0)):
        Cn = int(trace.shape[1])
        G = 1 if pooled else Cn
        full = lib.lr_rtt_summary_workspace_bytes(S, Cn, a, b, burn, int(pooled))
        # the one-bin floor: the query has no per-pass argument; the workspace of a pass of one bin is that of the same
        # samples over a span of one bin, except for the counters, which always cover all n_bins + 1 edges (lr_rtt_layout)
        one = lib.lr_rtt_summary_workspace_bytes(S, Cn, a, a + 1.5, burn, int(pooled))
        floor = one - up(8 * G * 2 * 2) + up(8 * G * 2 * (nb + 1))
        assert 0 < floor <= full, (floor, full)
        label = "rtt_summary samples %d pooled %d (whole %d, one bin %d bytes)" % (S, pooled, full, floor)
        whole = contract(ops, torch, lambda: tuple(ops.rtt_summary(trace, S, a, b, burn, pooled, full)[1:4]), label=label)
        chunk = contract(ops, torch, lambda: tuple(ops.rtt_summary(trace, S, a, b, burn, pooled, floor)[1:4]), label=label + " floor")
        assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(whole, chunk)), "chunks change the bits"
        refuses(ops, torch, lambda: ops.rtt_summary(trace, S, a, b, burn, pooled, floor - 1), "LR_ERR_WORKSPACE", label=label,
                entry="lr_rtt_summary")
        say(label, "ok")
    P = _hip.ptr

    def one_sample():
        # one sample per chain, not pooled: n_in = round(0.95) = 1 < 2
        o = [ops.alloc_output((Cn, 3, 3, nb), torch.float64, "cuda"), ops.alloc_output((Cn, 2, nb), torch.float64, "cuda"),
             ops.alloc_output((Cn, 2, LR_KMAX), torch.int64, "cuda")]
        ws = ops.alloc_workspace(1 << 20, "cuda")
        abi("lr_rtt_summary", P(trace), 1, Cn, a, b, 0.0, 0, P(o[0]), P(o[1]), P(o[2]), P(ws), ws.numel())
    refuses(ops, torch, one_sample, "LR_ERR_SIZE", label="rtt_summary one sample", entry="lr_rtt_summary")

    rng = np.random.default_rng(8)
    for S, Cn, pooled, burn in ((20, 3, True, 0.2), (20, 3, False, 0.2), (2, 3, False, 0.0), (2, 1, True, 0.0)):
        rows = dev(torch, rng.normal(size=(S, Cn, 12)))
        cols = np.array([0, 11, 3], dtype=np.int32)
        cp = cols.ctypes.data_as(_hip.c_vp)
        full = lib.lr_col_summary_workspace_bytes(S, Cn, 12, cp, 3, burn, int(pooled), 0)
        floor = lib.lr_col_summary_workspace_bytes(S, Cn, 12, cp, 3, burn, int(pooled), 1)
        assert 0 < floor <= full
        label = "col_summary samples %d chains %d pooled %d (whole %d, one column %d bytes)" % (S, Cn, pooled, full, floor)
        whole = contract(ops, torch, lambda: tuple(ops.col_summary(rows, S, cols, burn, pooled, full)[:3]), label=label)
        chunk = contract(ops, torch, lambda: tuple(ops.col_summary(rows, S, cols, burn, pooled, floor)[:3]), label=label + " floor")
        assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(whole, chunk))
        refuses(ops, torch, lambda: ops.col_summary(rows, S, cols, burn, pooled, floor - 1), "LR_ERR_WORKSPACE", label=label,
                entry="lr_col_summary")
        # curves: DDRate parameter vectors in columns 4 .. 11, trend_rate's in 4 .. 9
        par = np.column_stack([rng.uniform(.1, .5, S * Cn), rng.uniform(.05, .3, S * Cn), rng.uniform(2, 6, S * Cn), rng.uniform(5, 50, S * Cn),
                               rng.uniform(10, 200, S * Cn), rng.uniform(.05, .4, S * Cn), rng.uniform(.5, 2, S * Cn), rng.uniform(.5, 2, S * Cn)])
        r2 = rng.normal(size=(S, Cn, 12))
        r2[:, :, 4:12] = par.reshape(S, Cn, 8)
        r2 = dev(torch, r2)
        for sampler, bins in ((1, 5), (2, 5), (1, 1)):
            aux = dev(torch, rng.uniform(0.1, 1.0, bins) * (100.0 if sampler == 1 else 1.0))
            m = 2 if sampler == 1 else 0
            full = lib.lr_curve_summary_workspace_bytes(S, Cn, 12, 4, sampler, bins, burn, int(pooled), 0)
            floor = lib.lr_curve_summary_workspace_bytes(S, Cn, 12, 4, sampler, bins, burn, int(pooled), 1)
            assert 0 < floor <= full
            lab = "curve_summary sampler %d bins %d samples %d chains %d pooled %d" % (sampler, bins, S, Cn, pooled)
            whole = contract(ops, torch, lambda: ops.curve_summary(r2, S, sampler, aux, m, m, 4, burn, pooled, full)[1], label=lab)
            chunk = contract(ops, torch, lambda: ops.curve_summary(r2, S, sampler, aux, m, m, 4, burn, pooled, floor)[1], label=lab + " floor")
            assert torch.equal(whole.view(torch.int64), chunk.view(torch.int64))
            refuses(ops, torch, lambda: ops.curve_summary(r2, S, sampler, aux, m, m, 4, burn, pooled, floor - 1), "LR_ERR_WORKSPACE", label=lab,
                    entry="lr_curve_summary")
        say(label, "and its curves ok")
    bad = np.array([12], dtype=np.int32)

    def column_12():
        out, ws = ops.alloc_output((1, 1, 3), torch.float64, "cuda"), ops.alloc_workspace(1 << 20, "cuda")
        abi("lr_col_summary", P(rows), S, Cn, 12, bad.ctypes.data_as(_hip.c_vp), 1, burn, int(pooled), P(out), P(ws), ws.numel())
    refuses(ops, torch, column_12, "LR_ERR_SIZE", label="col_summary column 12", entry="lr_col_summary")
    refuses(ops, torch, lambda: ops.curve_summary(r2, S, 1, aux, 5, 2, 4, burn, pooled, 1 << 20), "LR_ERR_MODEL", label="curve_summary m_birth 5",
            entry="lr_curve_summary")


@case("lr_ess_summary", "lr_ess_summary_workspace_bytes")
def case_ess():
    """lr_ess_summary with the kept series in LDS (4 and LR_ESS_LDS_ROWS rows) and in the workspace (one row more)"""
    torch, ops, _hip, lib = _gpu()
    assert ESS_ROWS == (4, _hip.LR_ESS_LDS_ROWS, _hip.LR_ESS_LDS_ROWS + 1)
    rng = np.random.default_rng(2)
    for n in ESS_ROWS:
        for Cn in (1, 3):
            x = np.cumsum(rng.normal(size=(n, Cn, 3)), axis=0) * 0.1 + rng.normal(size=(n, Cn, 3))
            x[:, :, 1] = 2.5                                   # a constant column: NaN ESS by the header's rule
            rows = dev(torch, x)
            label = "ess_summary rows %d chains %d" % (n, Cn)

            def call(burn=0.0):
                return tuple(ops.ess_summary(rows, n, [0, 1, 2], burn, 64))[:8]
            contract(ops, torch, call, label=label)
            refuses(ops, torch, call, "LR_ERR_WORKSPACE", short=1, label=label, entry="lr_ess_summary")
            say(label, "ok")
    cols, P = np.array([0, 1, 2], dtype=np.int32), _hip.ptr

    def burn_in_1():
        o = [ops.alloc_output((3, Cn, 4), torch.float64, "cuda"), ops.alloc_output((3, Cn), torch.int32, "cuda"),
             ops.alloc_output((3, 3), torch.float64, "cuda")]
        ws = ops.alloc_workspace(1 << 20, "cuda")
        abi("lr_ess_summary", P(rows), n, Cn, 3, cols.ctypes.data_as(_hip.c_vp), 3, 1.0, 64, P(o[0]), P(o[1]), P(o[2]), P(ws), ws.numel())
    refuses(ops, torch, burn_in_1, "LR_ERR_SIZE", label="ess_summary burn-in 1", entry="lr_ess_summary")


@case("lr_waic_pointwise", "lr_waic_workspace_bytes")
def case_waic(model):
    """lr_waic_pointwise under one model: one case per shape of lr_waic_plan (several draws per LDS chunk, one draw and two
    buffers, one buffer), one slice and three (LR_WAIC_SLICES), n one below and one above a tile of 512"""
    model = int(model)
    torch, ops, _hip, lib = _gpu()
    S = WAIC_DRAWS
    for nb in WAIC_BINS[model]:
        if nb is None:
            nb = max_bins(lambda b: lib.lr_waic_workspace_bytes(WAIC_N[1], b, S, model))
            assert lib.lr_waic_workspace_bytes(WAIC_N[1], nb + 1, S, model) == _hip.LR_ERR_SIZE
        lam, mu, br = rates(S, nb)
        lam_d, mu_d, br_d = dev(torch, lam), dev(torch, mu), dev(torch, br)
        end = float(T0 + nb // 2 + 0.5)
        for n in WAIC_N:
            ts, te = lineages(n, nb)
            ts_d, te_d = dev(torch, ts), dev(torch, te)
            for sl in WAIC_SLICES:
                os.environ["LR_WAIC_SLICES"] = sl
                plan = ops.waic_plan(n, nb, S, model)
                assert plan[0] == 512 and plan[2] == int(sl) and plan[3] == 2 - (n < 512), plan
                label = "waic model %d n %d bins %d plan %s" % (model, n, nb, plan)

                def call(t0=T0):
                    return ops.waic_pointwise(ts_d, te_d, t0, lam_d, mu_d, model, br_d, end)[:2]
                contract(ops, torch, call, label=label)
                refuses(ops, torch, call, "LR_ERR_WORKSPACE", short=1, label=label, entry="lr_waic_pointwise")
        say("waic model %d bins %d ok" % (model, nb))
    refuses(ops, torch, lambda: call(T0 + 0.5), "LR_ERR_T0", label="waic t0", entry="lr_waic_pointwise")
    os.environ.pop("LR_WAIC_SLICES")


def _flagging(n, nb, S):
    """lineages and rates with exactly one flagged lineage: lineage 0 alone is born in the last bin, whose birth rate is
    zero under draw 0 (log 0 = -inf)"""
    ts, te = lineages(n, nb)
    ts = np.minimum(ts, T0 + nb - 1.5)
    ts[0] = T0 + nb - 0.5
    te = np.maximum(te, ts + 1e-3)
    lam, mu, br = rates(S, nb)
    lam[0, nb - 1] = 0.0
    return ts, te, lam, mu, br


@case("lr_loo_pointwise", "lr_loo_workspace_bytes")
def case_loo():
    """lr_loo_pointwise: the tail lengths M = 0, 4, 5 and 272, one batch and two (LR_LOO_BATCH), one flagged lineage"""
    torch, ops, _hip, lib = _gpu()
    n, nb = LOO_N, LOO_BINS
    for model in (2, 0, 3):
        for S in (LOO_DRAWS if model == 2 else (25,)):
            for flagged in (False, True):
                ts, te, lam, mu, br = _flagging(n, nb, S)
                if not flagged:
                    lam[0, nb - 1] = 0.3
                a = [dev(torch, x) for x in (ts, te, lam, mu, br)]
                for batch in ("", "4"):
                    os.environ["LR_LOO_BATCH"] = batch
                    if not batch:
                        os.environ.pop("LR_LOO_BATCH")
                    plan = ops.loo_plan(n, nb, S, model)
                    assert plan[3] == (2 if batch else 1) and plan[0] == min(S // 5, int(np.ceil(3 * np.sqrt(S)))), plan
                    label = "loo model %d draws %d flagged %d plan %s" % (model, S, flagged, plan)

                    def call(t0=T0):
                        return ops.loo_pointwise(a[0], a[1], t0, a[2], a[3], model, a[4], T0 + 3.5)[:2]
                    got = contract(ops, torch, call, label=label)
                    n_flag = int(got[1][1])
                    assert (n_flag >= 1) == flagged and n_flag == int(torch.isnan(got[0][:, 0]).sum()), (label, got[1])
                    assert bool(torch.isnan(got[0][0]).all()) == flagged, label
                    refuses(ops, torch, call, "LR_ERR_WORKSPACE", short=1, label=label, entry="lr_loo_pointwise")
            say("loo model %d draws %d ok" % (model, S))
    refuses(ops, torch, lambda: call(T0 + 0.5), "LR_ERR_T0", label="loo t0", entry="lr_loo_pointwise")


@case("lr_psis_rows", "lr_psis_rows_workspace_bytes")
def case_psis():
    """lr_psis_rows: the same tail lengths, one row and five, one flagged row; the tail indices the call leaves in its
    workspace are defined (the -1 of a flagged row included) and compared too"""
    torch, ops, _hip, lib = _gpu()
    rng = np.random.default_rng(4)
    for S in LOO_DRAWS:
        for n in (1, 5):
            for flagged in (False, True):
                L = -3.0 + rng.normal(size=(n, S)) * 1.5
                if flagged:
                    L[n - 1, S // 2] = -np.inf
                L_d = dev(torch, L)
                label = "psis_rows rows %d draws %d flagged %d" % (n, S, flagged)
                got = contract(ops, torch, lambda: ops.psis_loo_rows(L_d, return_tail=True), label=label)
                assert int(got[1][1]) == int(flagged)
                if flagged and got[2].numel():
                    assert bool((got[2][n - 1] == -1).all())
                refuses(ops, torch, lambda: ops.psis_loo_rows(L_d), "LR_ERR_WORKSPACE", short=1, label=label, entry="lr_psis_rows")
        say("psis_rows draws %d ok" % S)
    P = _hip.ptr

    def one_draw():
        pw, tot = ops.alloc_output((5, 4), torch.float64, "cuda"), ops.alloc_output(10, torch.float64, "cuda")
        ws = ops.alloc_workspace(4096, "cuda")
        abi("lr_psis_rows", P(L_d), 5, 1, P(pw), P(tot), P(ws), ws.numel())
    refuses(ops, torch, one_draw, "LR_ERR_SIZE", label="psis_rows one draw", entry="lr_psis_rows")


# ---- the engine --------------------------------------------------------------------------------
N_LINEAGES, N_BINS, N_IT, S_FREQ = 300, 30, 200, 10
# engine -> (ChainEngine arguments, chains, what the layout must say).  5 chains is the least the resident streaming kernel
# plans at unit resolution (3 on general times) and leaves the last block of the pair and four-chain kernels ragged; the
# pipelined schedule needs 32 chains at unit resolution (17 on general times): 33 leave its second half ragged.
ENGINES = {
    "launch": (dict(engine="launch"), 5, dict(persistent=0, pipelined=0, streaming=0, packed_scan=0)),
    "pipelined": (dict(engine="launch"), 33, dict(persistent=0, pipelined=1)),
    "packed": (dict(engine="packed"), 5, dict(persistent=0, packed_scan=1)),
    "stream": (dict(engine="stream"), 5, dict(persistent=0, streaming=1)),
    "persistent2": (dict(engine="persistent2"), 5, dict(persistent=1)),
    "persistent4": (dict(engine="persistent4"), 5, dict(persistent=2)),
    "spec1": (dict(engine="spec", team=1), 5, dict(persistent=3, team_blocks=1)),
    "spec4": (dict(engine="spec", team=4), 5, dict(persistent=3, team_blocks=4)),
}
# times: unit (integer births, deaths at .5) or general (jitter on the 2^-32 grid); sampler: rj, dd, trend
ENGINE_RUNS = [(e, "unit", "rj") for e in ENGINES] + [(e, "general", "rj") for e in ENGINES if e != "persistent2"] + \
              [("persistent4", "unit", "dd"), ("spec1", "unit", "trend")]


def _engine_data(times):
    from literate_amd import synth
    ts, te, _ = synth.make_lineages(N_LINEAGES, n_bins=N_BINS, n_shifts=3, seed=2)
    if times == "general":
        rng = np.random.default_rng(3)
        grid = lambda x: np.round(x * 2.0 ** 32) / 2.0 ** 32
        keep_s, keep_e = ts == ts.min(), te >= te.max()
        ts = np.where(keep_s, ts, ts + grid(rng.uniform(0.0, 0.45, len(ts))))
        te = np.where(keep_e, te, te + grid(rng.uniform(0.0, 0.45, len(te))))
    return ts, te


_BINS = {}


def _create_bins(times):
    if times not in _BINS:
        from literate_amd.literate_library import create_bins
        ts, te = _engine_data(times)
        origin, present, _, _, DT, bins, _ = create_bins(float(ts.min()), float(te.max()), ts, te, 0)
        _BINS[times] = (float(origin), float(present), np.asarray(DT, dtype=float), int(bins))
    return _BINS[times]


def _make_engine(name, times, sampler, seed=11, table=None):
    """the engine on host-binned statistics (the binning kernel has its own case), so that the workspace is the only
    buffer the constructor allocates through the seam.  table: ENGINES, or a table with further entries (stream_cases)"""
    from literate_amd.engine import ChainEngine
    from oracle import literate_oracle as lo
    kw, Cn, want = (table or ENGINES)[name]
    ts, te = _engine_data(times)
    common = dict(seed=seed, s_freq=S_FREQ, n_trace_slots=N_IT // S_FREQ, **kw)
    if sampler == "rj":
        t0, sp, ex, br = lo.bin_events_cli(ts, te)
        eng = ChainEngine(ts, te, Cn, model=0, stats=(float(t0), len(br), br), **common)
    else:
        # what DDRateEngine / TrendRateEngine pass on: create_bins' statistics (binned once, outside any guarded run)
        origin, present, DT, bins = _create_bins(times)
        if sampler == "dd":
            eng = ChainEngine(ts, te, Cn, model=2, stats=(origin, bins, DT),
                              dd=dict(m_birth=2, m_death=2, present=present, init_death=0.1), **common)
        else:
            trend = np.maximum((np.arange(bins) % 7) / 6.0, 1e-15)
            eng = ChainEngine(ts, te, Cn, model=2, stats=(origin, bins, trend), dd=dict(kind="trend", m_birth=0, m_death=0), **common)
    for k, v in want.items():
        assert getattr(eng.layout, k) == v, (name, k, getattr(eng.layout, k), eng.kernel_name())
    assert eng.unit_resolution == (times == "unit")
    return eng


# the documented scalar slots every launch stores: all sixteen under the RJ sampler; under the parametric samplers the
# accepted and the pending likelihood and prior, the Hastings term and the acceptance draw (csrc/lr_spec.h, lr_step.h)
PARAM_SCALARS = (0, 1, 6, 7, 11, 15)


def _engine_state(torch, eng, sampler):
    """the defined part of an engine's workspace: the trace slots written, the accepted state (lanes below K of the rate
    and time rows, the scalar rows), the warning word and the status word"""
    from literate_amd import _hip
    eng.check_status()
    warn = eng.warnings()
    S, I = eng.state_f64, eng.state_i32
    isc = I[:, _hip.IROW_SCALARS, :_hip.I_SLOT + 1].clone()
    sc = S[:, _hip.ROW_SCALARS, :16] if sampler == "rj" else S[:, _hip.ROW_SCALARS][:, list(PARAM_SCALARS)]
    out = dict(trace=eng.trace[:eng.samples_done()].clone(), scalars=sc.clone(), iscalars=isc,
               words=eng.workspace[eng.layout.status:eng.layout.status + 8].clone())
    if sampler == "rj":
        KL, KM = isc[:, _hip.I_KL].tolist(), isc[:, _hip.I_KM].tolist()
        for c in range(eng.n_chains):
            out["L%d" % c], out["M%d" % c] = S[c, _hip.ROW_L, :KL[c]].clone(), S[c, _hip.ROW_M, :KM[c]].clone()
            out["tL%d" % c], out["tM%d" % c] = S[c, _hip.ROW_TL, :KL[c] + 1].clone(), S[c, _hip.ROW_TM, :KM[c] + 1].clone()
            out["eL%d" % c], out["eM%d" % c] = I[c, _hip.IROW_EL, :KL[c] + 1].clone(), I[c, _hip.IROW_EM, :KM[c] + 1].clone()
    else:
        out["args"] = S[:, _hip.ROW_L, :8 if sampler == "dd" else 6].clone()
    assert warn == int(out["words"].view(torch.int32)[1])
    return out


ENGINE_PARTIAL = ("int32_t n_trace_slots; /* capacity of the trace buffer in samples */ and LR_ROW_L /* accepted birth rates [K_l] */: "
                  "trace slots not yet written, state lanes at or above K and the engine's scratch regions are not defined")


@case("lr_mcmc_create", "lr_mcmc_init", "lr_mcmc_steps", "lr_mcmc_restore", "lr_mcmc_status", "lr_mcmc_warnings", "lr_mcmc_time_scan",
      "lr_mcmc_time_steps")
def case_engine(name, times, sampler):
    """One engine on a workspace of exactly total_bytes between guards, filled before lr_mcmc_create: 200 iterations in
    two lr_mcmc_steps calls, the defined state compared bit for bit across plain, 0x00 and 0xFF; then a run saved at
    iteration 100, restored into a second engine whose own workspace was filled with 0xFF, and continued; one byte short
    and a model without its br_length refused by lr_mcmc_create, a bad kmax by lr_mcmc_init, with nothing written."""
    torch, ops, _hip, lib = _gpu()
    assert os.environ.get("LR_SHARED_DEVICE", "0") != "1", "team requests are part of the case"

    def run():
        eng = _make_engine(name, times, sampler)
        try:
            assert eng.workspace.numel() == eng.layout.total_bytes
            eng.init()
            eng.steps(N_IT // 2)
            eng.steps(N_IT - N_IT // 2)
            return _engine_state(torch, eng, sampler)
        finally:
            eng.close()
    full = contract(ops, torch, run, partial=ENGINE_PARTIAL, label="engine %s %s %s" % (name, times, sampler))
    assert int(full["words"].view(torch.int32)[0]) == 0 and full["trace"].shape[0] == N_IT // S_FREQ
    say("engine %s %s %s: %d trace rows, bit-identical on plain, 0x00 and 0xFF workspaces" % (name, times, sampler, full["trace"].shape[0]))

    # restore: the dirty run's workspace at iteration 100 -> a second engine on a 0xFF workspace -> continue
    saved = ops.alloc_workspace, ops.alloc_output
    try:
        g = Guarded(torch, 0x00)
        ops.alloc_workspace, ops.alloc_output = g.workspace, g.output
        first = _make_engine(name, times, sampler)
        first.init()
        first.steps(N_IT // 2)
        first.check_status()
        image = first.workspace.clone()
        first.close()
        g2 = Guarded(torch, 0xFF)
        ops.alloc_workspace, ops.alloc_output = g2.workspace, g2.output
        second = _make_engine(name, times, sampler)
        assert bool((second.workspace == 0xFF).all()), "lr_mcmc_create writes nothing"
        second.workspace.copy_(image)
        _hip.check(_hip.launch(lib.lr_mcmc_restore, second.device, second.handle), "lr_mcmc_restore")
        second.iterations = N_IT // 2
        second.steps(N_IT - N_IT // 2)
        resumed = _engine_state(torch, second, sampler)
        if name == "launch":
            # the two measurement hooks: a timed scan changes nothing, timed steps are steps
            before = _engine_state(torch, second, sampler)
            second.time_scan(2)
            after = _engine_state(torch, second, sampler)
            _compare("dirty", "time_scan", {k: _bits(torch, v) for k, v in after.items()}, {k: _bits(torch, v) for k, v in before.items()},
                     "lr_mcmc_time_scan changed the state")
            second.timed_steps(S_FREQ)
            assert second.snapshot()["it"].tolist() == [N_IT + S_FREQ] * second.n_chains
        second.close()
        _sync(torch)
        g.check_guards("restore, first engine")
        g2.check_guards("restore, second engine")
    finally:
        ops.alloc_workspace, ops.alloc_output = saved
    _compare("dirty", "engine %s restore" % name, {k: _bits(torch, v) for k, v in resumed.items()}, {k: _bits(torch, v) for k, v in full.items()},
             "a run restored at iteration %d into a 0xFF workspace differs from the uninterrupted one" % (N_IT // 2))
    say("engine %s %s %s: restored run identical" % (name, times, sampler))

    # errors: nothing is written
    refuses(ops, torch, lambda: _make_engine(name, times, sampler), "LR_ERR_WORKSPACE", short=1, label="lr_mcmc_create one byte short",
            entry="lr_mcmc_create")
    if sampler == "rj":
        def no_br():
            eng = _make_engine(name, times, sampler)
            try:
                h = C.c_void_p()
                _hip.check(lib.lr_mcmc_create(C.byref(eng.cfg), _hip.ptr(eng.ts), _hip.ptr(eng.te), None, _hip.ptr(eng.workspace),
                                              eng.workspace.numel(), C.byref(h)), "lr_mcmc_create")
            finally:
                eng.close()

        def bad_kmax():
            eng = _make_engine(name, times, sampler)
            try:
                x = eng.ts[:1]
                _hip.check(_hip.launch(lib.lr_mcmc_init, eng.device, eng.handle, _hip.ptr(x), _hip.ptr(x), _hip.ptr(x), _hip.ptr(x), _hip.ptr(x),
                                       _hip.ptr(x), LR_KMAX + 1), "lr_mcmc_init")
            finally:
                eng.close()
        refuses(ops, torch, no_br, "LR_ERR_MODEL", label="lr_mcmc_create without br_length", entry="lr_mcmc_create")
        refuses(ops, torch, bad_kmax, "LR_ERR_SIZE", label="lr_mcmc_init kmax 33", entry="lr_mcmc_init")
    say("engine %s %s %s: errors leave the workspace alone" % (name, times, sampler))


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
