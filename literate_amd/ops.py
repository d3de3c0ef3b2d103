"""Tensor-level wrappers of the C ABI: torch tensors in HBM in, torch tensors out.

Every function enqueues on torch's current HIP stream and raises if the HIP library or a GPU is
missing (no CPU path).  Shapes follow include/literate_hip.h.
"""
import os
from collections import namedtuple

import numpy as np

from . import _hip

_ws_cache = {}


def _torch():
    return _hip.require_gpu()


def _dev(x, dtype, device=None):
    torch = _torch()
    if isinstance(x, torch.Tensor):
        # a tensor that already lives on a GPU stays there unless the caller names another device
        t = x.to(device=device or (x.device if x.is_cuda else "cuda"), dtype=dtype)
    else:
        t = torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(device or "cuda")
    return t.contiguous()


def _host_f64(x):
    """host numpy float64 view / copy of a tensor or array-like"""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def _workspace(nbytes, device):
    """A reusable byte workspace per device (grown on demand)."""
    torch = _torch()
    key = str(device)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def alloc_workspace(nbytes, device, zero=False, cached=False):
    """The one place a workspace of the C ABI is allocated (the wrappers here, LoglikSession, engine.ChainEngine): a uint8
    tensor whose numel() the caller passes on as workspace_bytes.  cached: the reusable per-device buffer (_workspace, at
    least `nbytes`); zero: cleared memory (the engine's workspace, lr_simulate_bd's 64 bytes); otherwise exactly `nbytes`
    of uninitialised memory.  tests/helpers/abi_cases.py replaces this and alloc_output with guarded buffers."""
    torch = _torch()
    if cached:
        return _workspace(nbytes, device)
    return (torch.zeros if zero else torch.empty)(int(nbytes), dtype=torch.uint8, device=device)


def alloc_output(shape, dtype, device, zero=False):
    """The one place an output of the C ABI is allocated: a contiguous tensor, cleared when `zero`."""
    torch = _torch()
    return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)


def _unit_windows(win_lo, win_hi):
    """(t0, n_bins) when the windows are the unit bins [t0 + w, t0 + w + 1] with t0 integer valued - what the reference
    always bins into (LRF:519-523, lib create_bins) - else None.  Decided on host arrays only (no device read-back)."""
    if hasattr(win_lo, "data_ptr") or hasattr(win_hi, "data_ptr"):     # torch tensors: possibly on the device, not inspected
        return None
    lo, hi = np.asarray(win_lo, dtype=float).ravel(), np.asarray(win_hi, dtype=float).ravel()
    if lo.size < 1 or hi.size != lo.size or lo.size > _hip.LR_MAX_BINS:
        return None
    t0 = float(lo[0])
    if not (np.isfinite(t0) and t0 == np.floor(t0) and abs(t0) < 1e9):
        return None
    grid = t0 + np.arange(lo.size, dtype=float)
    if np.array_equal(lo, grid) and np.array_equal(hi, grid + 1.0):
        return t0, int(lo.size)
    return None


def bin_unit_events(ts, te, t0, n_bins):
    """(sp_events int64[n_bins], ex_events, br_length f64) of the unit windows [t0 + w, t0 + w + 1]: one pass over the
    lineages (lr_bin_unit_events; the loop LRF:519-523 / lib create_bins:231-245)."""
    torch = _torch()
    lib = _hip.load()
    ts = _dev(ts, torch.float64)
    te = _dev(te, torch.float64, ts.device)
    n = ts.numel()
    if te.numel() != n:
        raise ValueError("ts and te differ in length")
    sp = alloc_output(n_bins, torch.int64, ts.device)
    ex = alloc_output(n_bins, torch.int64, ts.device)
    br = alloc_output(n_bins, torch.float64, ts.device)
    nbytes = lib.lr_bin_unit_events_workspace_bytes(n, n_bins)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_bin_unit_events_workspace_bytes")
    ws = alloc_workspace(nbytes, ts.device, cached=True)
    rc = _hip.launch(lib.lr_bin_unit_events, ts.device, _hip.ptr(ts), _hip.ptr(te), n, float(t0), int(n_bins), _hip.ptr(sp),
                     _hip.ptr(ex), _hip.ptr(br), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_bin_unit_events")
    return sp, ex, br


def bin_events(ts, te, win_lo, win_hi):
    """(sp_events int64[W], ex_events int64[W], br_length f64[W]) for windows [lo_w, hi_w]
    (precompute_events / get_br, lib:74-85, for all windows in one launch).  Unit windows on an integer origin - every
    binning call of the reference's CLIs - take the one-pass kernel (bin_unit_events)."""
    torch = _torch()
    lib = _hip.load()
    unit = _unit_windows(win_lo, win_hi)
    if unit is not None:
        return bin_unit_events(ts, te, unit[0], unit[1])
    ts = _dev(ts, torch.float64)
    te = _dev(te, torch.float64, ts.device)
    lo, hi = _dev(win_lo, torch.float64, ts.device), _dev(win_hi, torch.float64, ts.device)
    n, w = ts.numel(), lo.numel()
    if te.numel() != n or hi.numel() != w:
        raise ValueError("ts/te or window arrays differ in length")
    sp = alloc_output(w, torch.int64, ts.device)
    ex = alloc_output(w, torch.int64, ts.device)
    br = alloc_output(w, torch.float64, ts.device)
    nbytes = lib.lr_bin_events_workspace_bytes(n, w)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_bin_events_workspace_bytes")
    ws = alloc_workspace(nbytes, ts.device, cached=True)
    rc = _hip.launch(lib.lr_bin_events, ts.device, _hip.ptr(ts), _hip.ptr(te), n, _hip.ptr(lo), _hip.ptr(hi), w, _hip.ptr(sp), _hip.ptr(ex),
                           _hip.ptr(br), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_bin_events")
    return sp, ex, br


def _check_host_K(K, kmax, what, room=None):
    """K given as a host array: 1 <= K <= kmax (and K + 1 <= kmax where `room` marks an add move), or ValueError - the
    kernels index the padded rows by K unchecked.  A K that already lives on the device is not read back."""
    if hasattr(K, "is_cuda") and K.is_cuda:
        return
    k = np.asarray(K.cpu().numpy() if hasattr(K, "detach") else K).astype(np.int64).ravel()
    if k.size and (k.min() < 1 or k.max() > kmax):
        raise ValueError("%s: K must lie in 1..kmax = %d (got %d..%d)" % (what, kmax, k.min(), k.max()))
    if room is not None:
        room = np.asarray(room.cpu().numpy() if hasattr(room, "detach") else room).ravel()
        if room.shape == k.shape and np.any(room & (k + 1 > kmax)):
            raise ValueError("%s: an add move at K = kmax = %d has no room for the new rate" % (what, kmax))


def expand_rates(rates, times, K, n_bins, mode=0):
    """[C,n_bins] per-bin rates from K segment rates (get_rate_index + L[ind], LRF:125-135).  K as a host array is
    checked against kmax (ValueError); a device-resident K is passed on unchecked."""
    torch = _torch()
    lib = _hip.load()
    rates, times = _dev(rates, torch.float64), _dev(times, torch.float64)
    _check_host_K(K, rates.shape[1], "expand_rates")
    K = _dev(K, torch.int32)
    C, kmax = rates.shape
    if times.shape != (C, kmax + 1) or K.shape != (C,):
        raise ValueError("shape mismatch: rates [C,kmax], times [C,kmax+1], K [C]")
    out = alloc_output((C, n_bins), torch.float64, rates.device)
    rc = _hip.launch(lib.lr_expand_rates, rates.device, _hip.ptr(rates), _hip.ptr(times), _hip.ptr(K), kmax, C, n_bins, mode, _hip.ptr(out))
    _hip.check(rc, "lr_expand_rates")
    return out


def bd_loglik_batch(ts, te, t0, lam_bins, mu_bins, model=2, br_length=None, end_time=0.0):
    """out[C]: per-lineage birth-death log-likelihood of C per-bin rate vectors (LRF:137-162,
    BDIx:124-146).  ts/te are scanned once per group of chains."""
    torch = _torch()
    lib = _hip.load()
    ts = _dev(ts, torch.float64)
    te = _dev(te, torch.float64, ts.device)
    lam, mu = _dev(lam_bins, torch.float64, ts.device), _dev(mu_bins, torch.float64, ts.device)
    if lam.dim() == 1:
        lam, mu = lam[None, :], mu[None, :]
    C, n_bins = lam.shape
    if mu.shape != lam.shape or te.numel() != ts.numel():
        raise ValueError("shape mismatch")
    br = None if br_length is None else _dev(br_length, torch.float64, ts.device)
    if br is not None and br.numel() != n_bins:
        raise ValueError("br_length must have n_bins entries")
    out = alloc_output(C, torch.float64, ts.device)
    nbytes = lib.lr_bd_loglik_workspace_bytes(ts.numel(), n_bins, C, model)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_bd_loglik_workspace_bytes")
    ws = alloc_workspace(nbytes, ts.device, cached=True)
    rc = _hip.launch(lib.lr_bd_loglik_batch, ts.device, _hip.ptr(ts), _hip.ptr(te), ts.numel(), float(t0), n_bins, _hip.ptr(lam), _hip.ptr(mu),
                                C, model, _hip.ptr(br), float(end_time), _hip.ptr(out), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_bd_loglik_batch")
    return out


WAIC_TOTALS = ("lineages_used", "lineages_flagged", "lppd", "p_waic", "elpd_waic", "se_elpd", "n_var_gt_0.4", "max_var")
WAIC_PLAN = ("lineages_per_tile", "draws_per_chunk", "draw_slices", "tiles")


def waic_plan(n, n_bins, n_draws, model=2):
    """lr_waic_plan: (lineages per tile, draws per LDS chunk, draw slices, tiles) - a function of the sizes alone (host)."""
    import ctypes as C
    import torch  # noqa: F401  (before the library, as everywhere here: both must bind the HIP runtime torch ships)
    lib = _hip.load()
    out = (C.c_int32 * 4)()
    _hip.check(lib.lr_waic_plan(int(n), int(n_bins), int(n_draws), int(model), out), "lr_waic_plan")
    return tuple(int(v) for v in out)


def _draws_pointwise(workspace_bytes, plan_of, pointwise, width, n_totals, ts, te, t0, lam_bins, mu_bins, model, br_length,
                     end_time):
    """waic_pointwise / loo_pointwise around their three entry points: the arguments on the device and checked, the plan, the
    outputs [n, width] and [n_totals], the cached workspace, the launch -> (pointwise, totals, plan, workspace, n, S)"""
    torch = _torch()
    ts = _dev(ts, torch.float64)
    te = _dev(te, torch.float64, ts.device)
    lam, mu = _dev(lam_bins, torch.float64, ts.device), _dev(mu_bins, torch.float64, ts.device)
    if lam.dim() != 2 or mu.shape != lam.shape or te.numel() != ts.numel() or ts.dim() != 1:
        raise ValueError("shape mismatch: ts, te [n]; lam_bins, mu_bins [draws, n_bins]")
    S, n_bins = lam.shape
    n = ts.numel()
    br = None if br_length is None else _dev(br_length, torch.float64, ts.device)
    if br is not None and br.numel() != n_bins:
        raise ValueError("br_length must have n_bins entries")
    nbytes = workspace_bytes(n, n_bins, S, int(model))
    if nbytes < 0:
        _hip.check(int(nbytes), workspace_bytes.__name__)
    plan = plan_of(n, n_bins, S, model)
    pw = alloc_output((n, width), torch.float64, ts.device)
    tot = alloc_output(n_totals, torch.float64, ts.device)
    ws = alloc_workspace(nbytes, ts.device, cached=True)
    rc = _hip.launch(pointwise, ts.device, _hip.ptr(ts), _hip.ptr(te), n, float(t0), n_bins, _hip.ptr(lam), _hip.ptr(mu), S,
                     int(model), _hip.ptr(br), float(end_time), _hip.ptr(pw), _hip.ptr(tot), _hip.ptr(ws), ws.numel())
    _hip.check(rc, pointwise.__name__)
    return pw, tot, plan, ws, n, S


def waic_pointwise(ts, te, t0, lam_bins, mu_bins, model=2, br_length=None, end_time=0.0):
    """Pointwise WAIC terms of S posterior draws of per-bin rates [S, n_bins] (lr_waic_pointwise): returns
    (pointwise [n, 3] = lppd_i, mean_i, var_i - NaN where a lineage's term is not finite under some draw -,
    totals [8] (WAIC_TOTALS), plan (WAIC_PLAN, host tuple)), tensors on the device.  The [n, S] matrix of terms is never
    stored.  Models 0, 2 and 3."""
    lib = _hip.load()
    return _draws_pointwise(lib.lr_waic_workspace_bytes, waic_plan, lib.lr_waic_pointwise, 3, 8, ts, te, t0, lam_bins, mu_bins,
                            model, br_length, end_time)[:3]


LOO_TOTALS = ("lineages_used", "lineages_flagged", "elpd_loo", "se_elpd", "p_loo", "lppd", "n_k_gt_0.5", "n_k_gt_0.7",
              "n_unsmoothed", "max_k")
LOO_POINTWISE = ("elpd_loo", "pareto_k", "lppd", "n_eff")
LOO_PLAN = ("tail_length", "grid_points", "lineages_per_batch", "batches")


def loo_plan(n, n_bins, n_draws, model=2):
    """lr_loo_plan: (tail length M, grid points m of the fit - 0 without one -, lineages per batch, batches): a function of
    the sizes alone (host; LR_LOO_BATCH in the environment is read per call)."""
    import ctypes as C
    import torch  # noqa: F401  (before the library, as everywhere here: both must bind the HIP runtime torch ships)
    lib = _hip.load()
    out = (C.c_int32 * 4)()
    _hip.check(lib.lr_loo_plan(int(n), int(n_bins), int(n_draws), int(model), out), "lr_loo_plan")
    return tuple(int(v) for v in out)


def loo_pointwise(ts, te, t0, lam_bins, mu_bins, model=2, br_length=None, end_time=0.0, return_terms=False):
    """PSIS-LOO of S posterior draws of per-bin rates [S, n_bins] (lr_loo_pointwise): returns (pointwise [n, 4] =
    elpd_loo_i, pareto_k_i, lppd_i, n_eff_i - NaN where a lineage's term is not finite under some draw -, totals [10]
    (LOO_TOTALS), plan (LOO_PLAN, host tuple)), tensors on the device.  Models 0, 2 and 3; 2 <= S <= 8192.
    return_terms (a test hook; one batch only): also a copy of the [n, S] matrix of terms the first stage wrote."""
    lib = _hip.load()
    pw, tot, plan, ws, n, S = _draws_pointwise(lib.lr_loo_workspace_bytes, loo_plan, lib.lr_loo_pointwise, 4, 10, ts, te, t0,
                                               lam_bins, mu_bins, model, br_length, end_time)
    if return_terms:
        if plan[3] != 1:
            raise ValueError("return_terms: the call took %d batches; the workspace holds the last one only" % plan[3])
        return pw, tot, plan, ws[:n * S * 8].view(pw.dtype).reshape(n, S).clone()
    return pw, tot, plan


def psis_loo_rows(loglik, return_tail=False):
    """PSIS-LOO of a pointwise log-likelihood matrix [n_rows, S] (lr_psis_rows): (pointwise [n_rows, 4] (LOO_POINTWISE),
    totals [10] (LOO_TOTALS)) on the device.  return_tail: also the tail's draw indices int32 [n_rows, M] in the tail's
    sorted order (-1 in a flagged row), which the call leaves in its workspace."""
    torch = _torch()
    lib = _hip.load()
    L = _dev(loglik, torch.float64)
    if L.dim() != 2:
        raise ValueError("loglik must be [n_rows, draws]")
    n, S = L.shape
    nbytes = lib.lr_psis_rows_workspace_bytes(n, S)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_psis_rows_workspace_bytes")
    pw = alloc_output((n, 4), torch.float64, L.device)
    tot = alloc_output(10, torch.float64, L.device)
    ws = alloc_workspace(nbytes, L.device, cached=True)
    rc = _hip.launch(lib.lr_psis_rows, L.device, _hip.ptr(L), n, S, _hip.ptr(pw), _hip.ptr(tot), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_psis_rows")
    if return_tail:
        import math
        M = min(S // 5, math.isqrt(9 * S - 1) + 1)                  # min(floor(0.2 S), ceil(3 sqrt S))
        tail = ws[:n * max(M, 1) * 4].view(torch.int32).reshape(n, max(M, 1))[:, :M].clone()
        return pw, tot, tail
    return pw, tot


class LoglikSession:
    """The calc_likelihood seam (LRF:305-308: one call per MCMC iteration) with everything that does not change
    between calls prepared once: lineages and workspace resident in HBM, ONE pinned staging buffer for what a call may
    change - the per-bin rates of `n_states` states and br_length (the reference's operator reads the module global
    br_length_bin on every call, LRF:150-162, so the session takes it per call too) - and one for the result.
    Few states on few lineages: one launch that reads the pinned buffer and writes its result into pinned host memory
    the host polls (no copy, no stream synchronisation).  Otherwise: one host-to-device copy, the three launches of
    lr_bd_loglik_batch, one device-to-host copy and one stream synchronisation."""

    def __init__(self, ts, te, t0, n_bins, n_states, model=2, br_length=None, end_time=0.0):
        torch = _torch()
        self.lib = _hip.load()
        self.ts = _dev(ts, torch.float64)
        self.te = _dev(te, torch.float64, self.ts.device)
        dev = self.device = self.ts.device
        self.n, self.n_bins, self.C, self.model = self.ts.numel(), int(n_bins), int(n_states), int(model)
        self.has_br = br_length is not None
        # [lam: C x n_bins | mu: C x n_bins | br_length: n_bins], one pinned block and its device mirror
        self.stage_host = torch.zeros((2 * self.C + 1) * self.n_bins, dtype=torch.float64).pin_memory()
        self.stage_np = self.stage_host.numpy()
        self.rates_np = self.stage_np[:2 * self.C * self.n_bins].reshape(2, self.C, self.n_bins)
        self.br_np = self.stage_np[2 * self.C * self.n_bins:]
        if self.has_br:
            self.br_np[:] = _host_f64(br_length)
        self.stage = torch.empty_like(self.stage_host, device=dev)
        self.out = alloc_output(self.C, torch.float64, dev)
        self.out_host = torch.empty(self.C, dtype=torch.float64).pin_memory()
        self.out_np = self.out_host.numpy()
        nbytes = self.lib.lr_bd_loglik_workspace_bytes(self.n, self.n_bins, self.C, self.model)
        if nbytes < 0:
            _hip.check(int(nbytes), "lr_bd_loglik_workspace_bytes")
        self.ws = alloc_workspace(int(nbytes), dev)   # the session's own: nothing else scribbles on it
        self.stream = torch.cuda.current_stream(dev)
        self.zero_copy = (self.C <= 16 and self.n <= (1 << 18) and self.n * self.C <= (1 << 21) and self.n_bins <= 900
                          and os.environ.get("LR_LOGLIK_SMALL", "1") != "0")
        self.out_bits = self.out_np.view(np.uint64)
        self._t0, self._end_time = float(t0), float(end_time)
        self.args_zero = self._args(self.stage_host, self.out_host)
        self.args_copy = self._args(self.stage, self.out)

    def _args(self, stage, out):
        nb, C = self.n_bins, self.C
        base = stage.data_ptr()
        br = _hip.c_vp(base + 16 * C * nb) if self.has_br else None
        return (_hip.ptr(self.ts), _hip.ptr(self.te), self.n, self._t0, nb, _hip.c_vp(base), _hip.c_vp(base + 8 * C * nb),
                C, self.model, br, self._end_time, _hip.ptr(out), _hip.ptr(self.ws), self.ws.numel(),
                _hip.c_vp(self.stream.cuda_stream))

    _SENTINEL = np.uint64(0x7FF8DEAD0000BEEF)      # a NaN payload no arithmetic produces: "not written yet"

    def __call__(self, L, M, br_length=None):
        """L, M: [n_states, n_bins] (or [n_bins] when n_states == 1) host arrays, br_length: this call's [n_bins]
        (None: the one given at construction) -> numpy [n_states] (a view of the session's pinned result buffer:
        valid until the next call)."""
        torch = _torch()
        self.rates_np[0] = L
        self.rates_np[1] = M
        if br_length is not None and self.has_br:
            self.br_np[:] = br_length
        # the launch goes to the stream captured at construction: that stream's device must be current for the call
        switch = torch.cuda.current_device() != self.device.index
        if switch:
            prev = torch.cuda.current_device()
            torch.cuda.set_device(self.device)
        try:
            if self.zero_copy:
                self.out_bits[:] = self._SENTINEL
                rc = self.lib.lr_bd_loglik_batch(*self.args_zero)
                _hip.check(rc, "lr_bd_loglik_batch")
                bits, sent = self.out_bits, self._SENTINEL
                for _ in range(200000):                       # ~0.2 s of polling at most, then the ordinary wait
                    if not (bits == sent).any():
                        return self.out_np
                # the result did not become visible to the polling host (non-coherent pinned memory, a stalled device):
                # wait the ordinary way, and do not poll again in this session
                self.zero_copy = False
                self.stream.synchronize()
                if (bits == sent).any():
                    raise _hip.HipLibraryError("lr_bd_loglik_batch: the result never arrived in host memory")
                return self.out_np
            with torch.cuda.stream(self.stream):
                self.stage.copy_(self.stage_host, non_blocking=True)
                rc = self.lib.lr_bd_loglik_batch(*self.args_copy)
                _hip.check(rc, "lr_bd_loglik_batch")
                self.out_host.copy_(self.out, non_blocking=True)
            self.stream.synchronize()
            return self.out_np
        finally:
            if switch:
                torch.cuda.set_device(prev)


def rj_propose_score(rates, times, K, move, index, draws, mult_d=1.1):
    """Batched explicit-draw proposal scorer (LRF:29-69, 165-176).  Returns
    (rates'[C,kmax], times'[C,kmax+1], K'[C], score[C]).  K as a host array is checked (1 <= K <= kmax, and K + 1 <= kmax
    for the add moves when `move` is a host array too: ValueError); a device-resident K is passed on unchecked."""
    torch = _torch()
    lib = _hip.load()
    rates, times = _dev(rates, torch.float64), _dev(times, torch.float64)
    is_dev = hasattr(move, "is_cuda") and move.is_cuda
    _check_host_K(K, rates.shape[1], "rj_propose_score",
                  None if is_dev else (move.cpu().numpy() if hasattr(move, "detach") else np.asarray(move)) == 1)
    K, move, index = _dev(K, torch.int32), _dev(move, torch.int32), _dev(index, torch.int32)
    draws = _dev(draws, torch.float64)
    C, kmax = rates.shape
    if times.shape != (C, kmax + 1) or draws.shape != (C, 2 * kmax):
        raise ValueError("shape mismatch: times [C,kmax+1], draws [C,2*kmax]")
    o_r, o_t = alloc_output(rates.shape, rates.dtype, rates.device), alloc_output(times.shape, times.dtype, rates.device)
    o_k = alloc_output(K.shape, K.dtype, rates.device)
    o_s = alloc_output(C, torch.float64, rates.device)
    rc = _hip.launch(lib.lr_rj_propose_score, rates.device, _hip.ptr(rates), _hip.ptr(times), _hip.ptr(K), kmax, C, _hip.ptr(move), _hip.ptr(index),
                                 _hip.ptr(draws), float(mult_d), _hip.ptr(o_r), _hip.ptr(o_t), _hip.ptr(o_k),
                                 _hip.ptr(o_s))
    _hip.check(rc, "lr_rj_propose_score")
    return o_r, o_t, o_k, o_s


def log_priors(rates, K, shape, gamma_rate, poi_rate=None):
    """out[C] = prior_gamma(rates[:K], shape, gamma_rate) (+ Poisson_prior(K, poi_rate)) (LRF:198-202).  K as a host array
    is checked against kmax (ValueError); a device-resident K is passed on unchecked."""
    torch = _torch()
    lib = _hip.load()
    rates = _dev(rates, torch.float64)
    _check_host_K(K, rates.shape[1], "log_priors")
    K = _dev(K, torch.int32)
    C, kmax = rates.shape
    g = _dev(gamma_rate, torch.float64)
    p = None if poi_rate is None else _dev(poi_rate, torch.float64)
    out = alloc_output(C, torch.float64, rates.device)
    rc = _hip.launch(lib.lr_log_priors, rates.device, _hip.ptr(rates), _hip.ptr(K), kmax, C, float(shape), _hip.ptr(g), _hip.ptr(p), _hip.ptr(out))
    _hip.check(rc, "lr_log_priors")
    return out


def dd_rates(args, DT, m_birth=2, m_death=2):
    """DDRate per-bin (birth, death, niche, niche_frac), each [C,n_bins] (DD:71-100)."""
    torch = _torch()
    lib = _hip.load()
    args, DT = _dev(args, torch.float64), _dev(DT, torch.float64)
    if args.dim() == 1:
        args = args[None, :]
    if args.shape[1] != 8:
        raise ValueError("DDRate takes 8 parameters per state")
    C, n_bins = args.shape[0], DT.numel()
    outs = [alloc_output((C, n_bins), torch.float64, args.device) for _ in range(4)]
    rc = _hip.launch(lib.lr_dd_rates, args.device, _hip.ptr(args), _hip.ptr(DT), n_bins, C, m_birth, m_death, *[_hip.ptr(o) for o in outs])
    _hip.check(rc, "lr_dd_rates")
    return tuple(outs)


def ddv2_rates(args, DT, m_birth=2, m_death=2):
    """DDRatev2 per-bin (birth, death, niche, niche_frac), each [C,n_bins] (DDRatev2.py:73-104); args [C,9]."""
    torch = _torch()
    lib = _hip.load()
    args, DT = _dev(args, torch.float64), _dev(DT, torch.float64)
    if args.dim() == 1:
        args = args[None, :]
    if args.shape[1] != 9:
        raise ValueError("DDRatev2 takes 9 parameters per state")
    C, n_bins = args.shape[0], DT.numel()
    outs = [alloc_output((C, n_bins), torch.float64, args.device) for _ in range(4)]
    rc = _hip.launch(lib.lr_ddv2_rates, args.device, _hip.ptr(args), _hip.ptr(DT), n_bins, C, m_birth, m_death, *[_hip.ptr(o) for o in outs])
    _hip.check(rc, "lr_ddv2_rates")
    return tuple(outs)


def trend_rates(args, trend, const_birth=False, const_death=False):
    """trend_rate.py:73-88 per-bin (birth, death), each [C,n_bins]; args [C,6], trend = normalised covariate."""
    torch = _torch()
    lib = _hip.load()
    args, trend = _dev(args, torch.float64), _dev(trend, torch.float64)
    if args.dim() == 1:
        args = args[None, :]
    if args.shape[1] != 6:
        raise ValueError("trend_rate takes 6 parameters per state")
    C, n_bins = args.shape[0], trend.numel()
    outs = [alloc_output((C, n_bins), torch.float64, args.device) for _ in range(2)]
    rc = _hip.launch(lib.lr_trend_rates, args.device, _hip.ptr(args), _hip.ptr(trend), n_bins, C, int(bool(const_birth)), int(bool(const_death)),
                            *[_hip.ptr(o) for o in outs])
    _hip.check(rc, "lr_trend_rates")
    return tuple(outs)


def binned_keiding(birth, death, n_spec, n_exti, DT):
    """(birth_lik[C], death_lik[C]) = sum_b log(rate) * events - rate * DT (DD:86, 101) for C per-bin rate vectors."""
    torch = _torch()
    lib = _hip.load()
    birth, death, DT = _dev(birth, torch.float64), _dev(death, torch.float64), _dev(DT, torch.float64)
    n_spec, n_exti = _dev(n_spec, torch.int64), _dev(n_exti, torch.int64)
    if birth.dim() == 1:
        birth, death = birth[None, :], death[None, :]
    C, n_bins = birth.shape
    if death.shape != birth.shape or DT.numel() != n_bins or n_spec.numel() != n_bins or n_exti.numel() != n_bins:
        raise ValueError("shape mismatch")
    ob = alloc_output(C, torch.float64, birth.device)
    od = alloc_output(C, torch.float64, birth.device)
    rc = _hip.launch(lib.lr_binned_keiding, birth.device, _hip.ptr(birth), _hip.ptr(death), _hip.ptr(n_spec), _hip.ptr(n_exti), _hip.ptr(DT),
                               n_bins, C, _hip.ptr(ob), _hip.ptr(od))
    _hip.check(rc, "lr_binned_keiding")
    return ob, od


def simulate_bd(n_start, n_steps, seed, lam_steps=None, mu_steps=None, mode=0, l0=0.0, m0=0.0, K=1.0, scale=1.0,
                capacity=None, device=None):
    """Discrete-time birth-death simulation on the device (simulateRateABC.v2.py:103-234 / notebook 4 Simulator).
    Returns (ts, te, alive_trace) as device tensors: birth / death step per lineage (te = n_steps: extant), trimmed to
    the lineages created, in slot order, and the living count per step.  Raises OverflowError when `capacity`
    (default 64 x n_start, at least 1M) was hit."""
    torch = _torch()
    lib = _hip.load()
    dev = device or "cuda"
    capacity = int(capacity or max(64 * n_start, 1 << 20))
    lam = None if lam_steps is None else _dev(lam_steps, torch.float64, dev)
    mu = None if mu_steps is None else _dev(mu_steps, torch.float64, dev)
    if mode == 0 and (lam is None or mu is None or lam.numel() < n_steps or mu.numel() < n_steps):
        raise ValueError("mode 0 needs lam_steps and mu_steps with n_steps entries")
    ts = alloc_output(capacity, torch.float64, dev)
    te = alloc_output(capacity, torch.float64, dev)
    counters = alloc_output(4, torch.int64, dev, zero=True)
    trace = alloc_output(int(n_steps), torch.int64, dev, zero=True)
    ws = alloc_workspace(64, dev, zero=True)
    rc = _hip.launch(lib.lr_simulate_bd, ts.device, _hip.ptr(lam), _hip.ptr(mu), int(n_steps), int(mode), float(l0), float(m0), float(K),
                            float(scale), int(n_start), capacity, int(seed) & 0xFFFFFFFFFFFFFFFF, _hip.ptr(ts), _hip.ptr(te),
                            _hip.ptr(counters), _hip.ptr(trace), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_simulate_bd")
    n, alive, overflow, _ = [int(v) for v in counters.cpu()]
    if overflow:
        raise OverflowError("simulate_bd: more than %d lineages; pass a larger capacity" % capacity)
    return ts[:n], te[:n], trace


def simulate_bd_batch(lam_bins, mu_bins, steps_per_bin, n_start, seed, capacity=None, device=None):
    """Many independent birth-death simulations in one launch (lr_simulate_bd_batch).  lam_bins, mu_bins [n_reps, n_bins]:
    rates per time unit; replicate r is simulate_bd(n_start[r], n_bins * steps_per_bin, seed + r, lam_bins[r, t //
    steps_per_bin] / steps_per_bin, ...) bit for bit.  n_start: an int or [n_reps].  Returns (counts int64 [n_reps, 4,
    n_bins]: births, deaths, living at the bin's start, lineage-steps; totals int64 [n_reps, 4]: created, living at the
    end, overflow flag, first empty step or -1) as device tensors.  capacity (per replicate): default max(64 x max
    n_start, 1M); a replicate that exceeds it only sets its flag - nothing is raised, the flags are the caller's to read."""
    torch = _torch()
    lib = _hip.load()
    lam = _dev(lam_bins, torch.float64, device)
    dev = lam.device
    mu = _dev(mu_bins, torch.float64, dev)
    if lam.dim() != 2 or mu.shape != lam.shape:
        raise ValueError("lam_bins and mu_bins must both be [n_reps, n_bins]")
    R, nb = int(lam.shape[0]), int(lam.shape[1])
    if isinstance(n_start, (int, np.integer)):
        most = int(n_start)
        n0 = torch.full((R,), most, dtype=torch.int64, device=dev)
    else:
        n0 = _dev(n_start, torch.int64, dev).reshape(-1)
        if n0.numel() != R:
            raise ValueError("n_start must be an int or hold one entry per replicate")
        most = int(n0.max()) if capacity is None and R else 0
    capacity = int(capacity or max(64 * most, 1 << 20))
    nbytes = lib.lr_simulate_bd_batch_workspace_bytes(R, nb, int(steps_per_bin), capacity)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_simulate_bd_batch_workspace_bytes")
    counts = alloc_output((R, 4, nb), torch.int64, dev)
    totals = alloc_output((R, 4), torch.int64, dev)
    ws = alloc_workspace(int(nbytes), dev)
    rc = _hip.launch(lib.lr_simulate_bd_batch, dev, _hip.ptr(lam), _hip.ptr(mu), R, nb, int(steps_per_bin), _hip.ptr(n0),
                     capacity, int(seed) & 0xFFFFFFFFFFFFFFFF, _hip.ptr(counts), _hip.ptr(totals), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_simulate_bd_batch")
    return counts, totals


def simulate_dd_batch(params, x_bins, steps_per_bin, n_start, seed, m_birth=2, m_death=2, capacity=None, device=None):
    """Many independent diversity-dependent simulations in one launch (lr_simulate_dd_batch): simulate_bd_batch's
    replicate with the thresholds of every step recomputed from the count living at its start by DDRate's rate map
    (dd_rates' expressions with that count in the place of DT).  params [n_reps, 8]: l_max, k, x0, div_0, L, m_max, nuB,
    nuD as the trace holds them; x_bins [n_bins] (shared by all replicates) or [n_reps, n_bins]: the TIME_RANGE value of
    each simulated bin; n_start: an int or [n_reps].  Returns (counts, totals) and takes capacity as simulate_bd_batch."""
    torch = _torch()
    lib = _hip.load()
    par = _dev(params, torch.float64, device)
    dev = par.device
    if par.dim() == 1:
        par = par[None, :]
    if par.dim() != 2 or par.shape[1] != 8:
        raise ValueError("params must be [n_reps, 8]")
    R = int(par.shape[0])
    x = _dev(x_bins, torch.float64, dev)
    if x.dim() == 1:
        x = x[None, :].expand(R, -1)
    if x.dim() != 2 or x.shape[0] != R:
        raise ValueError("x_bins must be [n_bins] or [n_reps, n_bins]")
    x = x.contiguous()
    nb = int(x.shape[1])
    if isinstance(n_start, (int, np.integer)):
        most = int(n_start)
        n0 = torch.full((R,), most, dtype=torch.int64, device=dev)
    else:
        n0 = _dev(n_start, torch.int64, dev).reshape(-1)
        if n0.numel() != R:
            raise ValueError("n_start must be an int or hold one entry per replicate")
        most = int(n0.max()) if capacity is None and R else 0
    capacity = int(capacity or max(64 * most, 1 << 20))
    nbytes = lib.lr_simulate_dd_batch_workspace_bytes(R, nb, int(steps_per_bin), capacity)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_simulate_dd_batch_workspace_bytes")
    counts = alloc_output((R, 4, nb), torch.int64, dev)
    totals = alloc_output((R, 4), torch.int64, dev)
    ws = alloc_workspace(int(nbytes), dev)
    rc = _hip.launch(lib.lr_simulate_dd_batch, dev, _hip.ptr(par), _hip.ptr(x), int(m_birth), int(m_death), R, nb,
                     int(steps_per_bin), _hip.ptr(n0), capacity, int(seed) & 0xFFFFFFFFFFFFFFFF, _hip.ptr(counts),
                     _hip.ptr(totals), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_simulate_dd_batch")
    return counts, totals


RttSummary = namedtuple("RttSummary", "time rates shift_freq k_counts n_samples")
RttSummary.__doc__ = """lr_rtt_summary's results.  time [n_bins] (host): bin centres in ascending time; rates [G, 3, 3, n_bins]:
(birth, death, net) x (mean, HPD low, HPD high); shift_freq [G, 2, n_bins]; k_counts int64 [G, 2, LR_KMAX] (K = 1 ..
LR_KMAX); n_samples: samples per group.  G = 1 pooled, one per chain otherwise.  Device tensors, bins aligned with time."""


def rtt_time(start_age, end_age):
    """The bin centres get_marginal_rates returns (plotRJforward.v3.py:129-130): edges np.arange(a, b), e_{i+1} - 0.5."""
    edges = np.arange(start_age, end_age)
    if edges.size < 2:
        return np.zeros(0)
    return (edges - abs(edges[1] - edges[0]) / 2.)[1:]


def rtt_summary(trace, n_samples, start_age, end_age, burnin=0.2, pooled=True, workspace_bytes=None):
    """Posterior rates through time from trace rows [>= n_samples, C, LR_TRACE_W] (lr_rtt_summary: get_marginal_rates,
    plot_net_rate, get_r_plot's shift histogram and get_K_values of plotRJforward.v3.py) -> RttSummary.
    start_age / end_age: the root_age / death_age columns.  pooled: the rows of every chain pooled after dropping
    int(burnin S) of each (-combine 1); else one summary per chain (burn-in capped at 0.9 S).  workspace_bytes: cap the
    workspace (the call then works through the bins in chunks; the same results)."""
    torch = _torch()
    lib = _hip.load()
    trace = _dev(trace, torch.float64)
    if trace.dim() != 3 or trace.shape[2] != _hip.LR_TRACE_W or trace.shape[0] < int(n_samples):
        raise ValueError("trace must be [>= n_samples, chains, LR_TRACE_W]")
    S, C = int(n_samples), int(trace.shape[1])
    a, b = float(start_age), float(end_age)
    full = lib.lr_rtt_summary_workspace_bytes(S, C, a, b, float(burnin), int(bool(pooled)))
    if full < 0:
        _hip.check(int(full), "lr_rtt_summary_workspace_bytes")
    time = rtt_time(a, b)
    nb = time.size
    G = 1 if pooled else C
    dev = trace.device
    rates = alloc_output((G, 3, 3, nb), torch.float64, dev)
    freq = alloc_output((G, 2, nb), torch.float64, dev)
    kc = alloc_output((G, 2, _hip.LR_KMAX), torch.int64, dev)
    # by default at most a quarter of the free device memory (and never less than 1 GiB): the sort of a chunk's columns
    # runs a block per column, so the more columns a pass holds, the more CUs it keeps busy (a thousand chains pooled over
    # 123 bins: 7.3 GB in one pass)
    if workspace_bytes is not None:
        cap = int(workspace_bytes)
    elif os.environ.get("LR_RTT_WORKSPACE"):
        cap = int(os.environ["LR_RTT_WORKSPACE"])
    else:
        cap = max(1 << 30, torch.cuda.mem_get_info(dev)[0] // 4)
    ws = alloc_workspace(max(1, min(int(full), cap)), dev)
    rc = _hip.launch(lib.lr_rtt_summary, dev, _hip.ptr(trace), S, C, a, b, float(burnin), int(bool(pooled)), _hip.ptr(rates),
                     _hip.ptr(freq), _hip.ptr(kc), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_rtt_summary")
    burn = int(burnin * S)
    per = S - (burn if pooled else min(burn, int(0.9 * S)))
    return RttSummary(time, rates, freq, kc, per * C if pooled else per)


RttScore = namedtuple("RttScore", "time rates shift_freq k_counts covered score n_samples")
RttScore.__doc__ = """lr_rtt_score's results (include/literate_hip_score.h).  time [n_bins] (host): rtt_time's bin centres; rates
[G, 3, 3, n_bins], shift_freq [G, 2, n_bins], k_counts int64 [G, 2, LR_KMAX]: RttSummary's, one group per chains_per_group
chains; covered int32 [G, 3, n_bins] and score [3, n_bins, 6] (groups, coverage, bias, mean absolute error, root mean squared
error, mean HPD width), both None without a truth; n_samples: samples per group.  Device tensors."""


def rtt_score(trace, n_samples, chains_per_group, start_age, end_age, truth=None, burnin=0.2):
    """lr_rtt_summary(pooled) for every group of `chains_per_group` consecutive chains of trace rows [>= n_samples, C,
    LR_TRACE_W] in one launch without a workspace (lr_rtt_score), bit for bit rtt_summary's values on the group's slice, and -
    with truth [G, 2, n_bins] (birth, death; [2, n_bins]: the same for every group) - whether each group's 95 % HPD holds it
    and the coverage, bias, errors and band width over the groups -> RttScore.  A group holds at most LR_SCORE_MAX_SAMPLES
    samples after the burn-in."""
    torch = _torch()
    lib = _hip.load()
    trace = _dev(trace, torch.float64)
    if trace.dim() != 3 or trace.shape[2] != _hip.LR_TRACE_W or trace.shape[0] < int(n_samples):
        raise ValueError("trace must be [>= n_samples, chains, LR_TRACE_W]")
    S, C, cpg = int(n_samples), int(trace.shape[1]), int(chains_per_group)
    if cpg < 1:
        raise ValueError("chains_per_group must be at least 1, not %d" % cpg)
    a, b = float(start_age), float(end_age)
    time = rtt_time(a, b)
    nb = time.size
    G = C // cpg          # (chains that do not fill the groups: the library refuses, the outputs stay as they are)
    dev = trace.device
    rates = alloc_output((G, 3, 3, nb), torch.float64, dev)
    freq = alloc_output((G, 2, nb), torch.float64, dev)
    kc = alloc_output((G, 2, _hip.LR_KMAX), torch.int64, dev)
    covered = score = None
    if truth is not None:
        truth = _dev(truth, torch.float64, dev)
        if truth.dim() == 2:
            truth = truth[None].expand(G, -1, -1).contiguous()
        if tuple(truth.shape) != (G, 2, nb):
            raise ValueError("truth must be [G, 2, n_bins] or [2, n_bins]: %d groups, %d bins" % (G, nb))
        covered = alloc_output((G, 3, nb), torch.int32, dev)
        score = alloc_output((3, nb, _hip.LR_SCORE_COLS), torch.float64, dev)
    prob = _hip.RttScoreProblem(_hip.ptr(trace), _hip.ptr(truth), _hip.ptr(rates), _hip.ptr(freq), _hip.ptr(kc), _hip.ptr(covered),
                                _hip.ptr(score), S, C, cpg, 0, a, b, float(burnin), None)
    rc = _hip.launch_problem(lib.lr_rtt_score, dev, prob)
    if rc == _hip.LR_ERR_SIZE and C % cpg:
        raise ValueError("lr_rtt_score: LR_ERR_SIZE (%d chains are not a multiple of chains_per_group = %d)" % (C, cpg))
    _hip.check(rc, "lr_rtt_score")
    return RttScore(time, rates, freq, kc, covered, score, cpg * (S - int(burnin * S)))


AbcSims = namedtuple("AbcSims", "dist flags counts k_end")
AbcSims.__doc__ = """lr_abc_simulate's results (include/literate_hip_abc.h).  dist [n_sims] (+inf where flagged); flags int32 [n_sims]
(1 overflowed max_living, 2 extinct before the last step, 4 refused); counts int64 [n_sims, 4, n_bins] (births, deaths, living at
the bin's start, lineage-steps) and k_end [n_sims], each None when not asked for.  Device tensors."""


def abc_simulate(theta, n_start, obs, weight, steps_per_bin, max_living, seed, id0=0, sim_id=None, counts=False, k_end=False,
                 device=None):
    """Many simulations of the niche-construction model in one launch, one per lane, each with its distance to the observed
    per-bin statistics (lr_abc_simulate) -> AbcSims.  theta [n_sims, 6]: l0, m0, K0, Kmax, g, h; n_start: an int or [n_sims];
    obs, weight [3, n_bins]: birth rate, death rate, diversity at the start of the bin, and what each entry counts for (0: not
    at all).  Simulation i has the id id0 + i, or sim_id[i]; what it computes depends on (seed, id, its theta and n_start, the
    sizes, the tables) alone, so a second launch of chosen ids reproduces them."""
    torch = _torch()
    lib = _hip.load()
    th = _dev(theta, torch.float64, device)
    dev = th.device
    if th.dim() == 1:
        th = th[None, :]
    if th.dim() != 2 or th.shape[1] != _hip.LR_ABC_NPAR:
        raise ValueError("theta must be [n_sims, %d]" % _hip.LR_ABC_NPAR)
    N = int(th.shape[0])
    ob, w = _dev(obs, torch.float64, dev), _dev(weight, torch.float64, dev)
    if ob.dim() != 2 or ob.shape[0] != 3 or w.shape != ob.shape:
        raise ValueError("obs and weight must both be [3, n_bins]")
    nb = int(ob.shape[1])
    if isinstance(n_start, (int, np.integer)):
        n0 = torch.full((N,), int(n_start), dtype=torch.int32, device=dev)
    else:
        n0 = _dev(n_start, torch.int32, dev).reshape(-1)
        if n0.numel() != N:
            raise ValueError("n_start must be an int or hold one entry per simulation")
    ids = None
    if sim_id is not None:
        ids = _dev(sim_id, torch.int64, dev).reshape(-1)
        if ids.numel() != N:
            raise ValueError("sim_id must hold one entry per simulation")
    dist = alloc_output(N, torch.float64, dev)
    flags = alloc_output(N, torch.int32, dev)
    cnt = alloc_output((N, 4, nb), torch.int64, dev) if counts else None
    ke = alloc_output(N, torch.float64, dev) if k_end else None
    prob = _hip.AbcProblem(_hip.ptr(th), _hip.ptr(n0), _hip.ptr(ids), _hip.ptr(ob), _hip.ptr(w), _hip.ptr(dist), _hip.ptr(flags),
                           _hip.ptr(cnt), _hip.ptr(ke), N, int(id0), nb, int(steps_per_bin), int(max_living), 0,
                           int(seed) & 0xFFFFFFFFFFFFFFFF, None)
    _hip.check(_hip.launch_problem(lib.lr_abc_simulate, dev, prob), "lr_abc_simulate")
    return AbcSims(dist, flags, cnt, ke)


def abc_binomial(n, p, u, device=None):
    """The simulator's binomial draw on given uniforms (lr_abc_binomial): n int32 [N], p [N], u [N, n_u] -> (x int32 [N], used
    int32 [N]): the draws and the uniforms each consumed; x = -1 where the draw needs more than n_u uniforms (used: how many)
    or its arguments are refused."""
    torch = _torch()
    lib = _hip.load()
    n = _dev(n, torch.int32, device).reshape(-1)
    dev = n.device
    p = _dev(p, torch.float64, dev).reshape(-1)
    u = _dev(u, torch.float64, dev)
    N = int(n.numel())
    if p.numel() != N or u.dim() != 2 or u.shape[0] != N:
        raise ValueError("n and p must be [N], u [N, n_u]")
    x = alloc_output(N, torch.int32, dev)
    used = alloc_output(N, torch.int32, dev)
    prob = _hip.AbcBinomialProblem(_hip.ptr(n), _hip.ptr(p), _hip.ptr(u), _hip.ptr(x), _hip.ptr(used), N, int(u.shape[1]), 0, None)
    _hip.check(_hip.launch_problem(lib.lr_abc_binomial, dev, prob), "lr_abc_binomial")
    return x, used


ShiftPrior = namedtuple("ShiftPrior", "totals shift_hist k_drawn k_accepted")
ShiftPrior.__doc__ = """lr_shift_prior's counts (int64 device tensors).  totals [4]: accepted replicates, their shift times that fall
in a bin, replicates the cap on K stopped, their shift times in all; shift_hist [n_bins]: the accepted shift times per unit
bin (the bins of rtt_summary); k_drawn / k_accepted [LR_SHIFT_PRIOR_KCAP]: replicates / accepted replicates with K = 1 ..."""


def shift_prior(start_age, end_age, n_reps=1 << 20, seed=0, poi_lambda=None, rep0=0, out=None):
    """The prior on the times of rate shifts over [start_age, end_age] by Monte Carlo (lr_shift_prior: get_prior_shift of
    plotRJforward.v3.py) -> ShiftPrior.  Replicates rep0 .. rep0 + n_reps - 1 of the stream `seed` names; poi_lambda None
    (or <= 0): the reference's Gamma(2, 1) hyper-prior on the Poisson rate, > 0: that fixed rate (a run made with
    -Poisson_prior).  out: a ShiftPrior of an earlier call over the same span to ADD this range's counts to (a replicate
    range sharded over calls); it is returned.  literate_amd.shift_bf turns the counts into Bayes-factor thresholds.
    The default of 2^20 replicates (0.14 ms on an MI355X, 0.1 % of Monte Carlo noise on the prior frequency, a third of
    the reference's) stays below the cost of a small run's rtt_summary; 2^24 takes 1.6 ms (profiles/EXPERIMENTS.md)."""
    torch = _torch()
    lib = _hip.load()
    a, b = float(start_age), float(end_age)
    lam = 0.0 if poi_lambda is None else float(poi_lambda)
    nb = int(np.ceil(b - a)) - 1 if 1.0 < b - a <= _hip.LR_MAX_BINS + 1.0 else 0      # (else the library refuses the span)
    if out is None:
        dev = "cuda"
        # (a span the library refuses still gets a histogram to point at: the refusal is the library's, LR_ERR_SIZE)
        res = ShiftPrior(alloc_output(4, torch.int64, dev), alloc_output(max(nb, 1), torch.int64, dev),
                         alloc_output(_hip.LR_SHIFT_PRIOR_KCAP, torch.int64, dev),
                         alloc_output(_hip.LR_SHIFT_PRIOR_KCAP, torch.int64, dev))
    else:
        res = out
        sizes = (4, nb, _hip.LR_SHIFT_PRIOR_KCAP, _hip.LR_SHIFT_PRIOR_KCAP)
        if any(t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous() or not t.is_cuda for t, n in zip(res, sizes)):
            raise ValueError("out must be the ShiftPrior of a call over the same span")
    dev = res.totals.device
    rc = _hip.launch(lib.lr_shift_prior, dev, a, b, int(rep0), int(n_reps), int(seed) & 0xFFFFFFFFFFFFFFFF, lam,
                     int(out is not None), _hip.ptr(res.totals), _hip.ptr(res.shift_hist), _hip.ptr(res.k_drawn),
                     _hip.ptr(res.k_accepted))
    _hip.check(rc, "lr_shift_prior")
    return res


PPC_AGE_TOTALS = ("lineages_used", "lineages_unused", "draws_used", "draws_flagged")
PPC_AGE_PLAN = ("lineages_per_tile", "draws_per_slice", "draw_slices", "tiles")


def ppc_age_plan(n, n_bins, n_draws):
    """lr_ppc_age_plan: (lineages per tile, draws per slice, slices, tiles) - a function of the sizes alone (host;
    LR_PPC_AGE_SLICES in the environment is read per call)."""
    import ctypes as C
    import torch  # noqa: F401  (before the library, as everywhere here: both must bind the HIP runtime torch ships)
    lib = _hip.load()
    out = (C.c_int32 * 4)()
    _hip.check(lib.lr_ppc_age_plan(int(n), int(n_bins), int(n_draws), out), "lr_ppc_age_plan")
    return tuple(int(v) for v in out)


def ppc_age(ts, te, t0, mu_bins, seed, out=None):
    """Posterior predictive deaths by age (lr_ppc_age, include/literate_hip_age.h): every lineage, born at its ts, dies
    under every one of the S draws of per-bin death rates mu_bins [S, n_bins] -> (obs [2, A] observed dead / censored per
    age class, rep [S, 2, A] simulated dead / survivors per draw and class - all -1 for a flagged draw -, totals [4]
    (PPC_AGE_TOTALS), plan (PPC_AGE_PLAN, host tuple)); int64 tensors on the device, A = n_bins.  The Philox counter of a
    pair is (position of the lineage in ts / te, draw), the key `seed`.  out: the (obs, rep, totals) of an earlier call of
    the same sizes to write into (they may hold anything)."""
    torch = _torch()
    lib = _hip.load()
    ts = _dev(ts, torch.float64)
    te = _dev(te, torch.float64, ts.device)
    mu = _dev(mu_bins, torch.float64, ts.device)
    if mu.dim() != 2 or ts.dim() != 1 or te.numel() != ts.numel():
        raise ValueError("shape mismatch: ts, te [n]; mu_bins [draws, n_bins]")
    S, A = (int(v) for v in mu.shape)
    n, dev = ts.numel(), ts.device
    nbytes = lib.lr_ppc_age_workspace_bytes(n, A, S)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_ppc_age_workspace_bytes")
    plan = ppc_age_plan(n, A, S)
    if out is None:
        obs, rep, tot = (alloc_output(shape, torch.int64, dev) for shape in ((2, A), (S, 2, A), 4))
    else:
        obs, rep, tot = out[:3]
        if any(t.dtype != torch.int64 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev
               for t, shape in zip((obs, rep, tot), ((2, A), (S, 2, A), (4,)))):
            raise ValueError("out must be the (obs, rep, totals) of a call of the same sizes")
    ws = alloc_workspace(nbytes, dev, cached=True)
    rc = _hip.launch(lib.lr_ppc_age, dev, _hip.ptr(ts), _hip.ptr(te), n, float(t0), A, _hip.ptr(mu), S,
                     int(seed) & 0xFFFFFFFFFFFFFFFF, _hip.ptr(obs), _hip.ptr(rep), _hip.ptr(tot), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_ppc_age")
    return obs, rep, tot, plan


ADE_TOTALS = ("lineages_used", "lineages_unused")


def _ade_out(out, shapes, dtypes, dev, what):
    """the outputs of an earlier call of the same sizes, checked - or fresh ones"""
    torch = _torch()
    if out is None:
        return tuple(alloc_output(shape, dt, dev) for shape, dt in zip(shapes, dtypes))
    got = tuple(out[:len(shapes)])
    if any(t.dtype != dt or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev
           for t, shape, dt in zip(got, shapes, dtypes)):
        raise ValueError("out must be the %s of a call of the same sizes" % what)
    return got


def ade_classes(ts, te, t0, n_bins, out=None):
    """The lineages per (birth bin, age at death) class (lr_ade_classes, include/literate_hip_ade.h) -> (dead [A, A]: dead[jb][a]
    lineages born in bin jb that died a bins later, cens [A]: alive at the end of the window per birth bin, totals [2]
    (ADE_TOTALS)); int64 tensors on the device, A = n_bins <= LR_ADE_MAX_BINS.  out: the (dead, cens, totals) of an earlier
    call of the same sizes to write into (they may hold anything)."""
    torch = _torch()
    lib = _hip.load()
    ts = _dev(ts, torch.float64)
    te = _dev(te, torch.float64, ts.device)
    if ts.dim() != 1 or te.numel() != ts.numel():
        raise ValueError("shape mismatch: ts, te [n]")
    A, n, dev = int(n_bins), ts.numel(), ts.device
    if not 1 <= A <= _hip.LR_ADE_MAX_BINS:
        _hip.check(_hip.LR_ERR_SIZE, "lr_ade_classes")
    dead, cens, tot = _ade_out(out, ((A, A), (A,), (2,)), (torch.int64,) * 3, dev, "(dead, cens, totals)")
    rc = _hip.launch(lib.lr_ade_classes, dev, _hip.ptr(ts), _hip.ptr(te), n, float(t0), A, _hip.ptr(dead), _hip.ptr(cens),
                     _hip.ptr(tot))
    _hip.check(rc, "lr_ade_classes")
    return dead, cens, tot


def ade_profile(dead, cens, mu_bins, shapes, out=None):
    """The profile likelihood of the Weibull shape (lr_ade_profile, include/literate_hip_ade.h): for every one of the S draws of
    per-bin death rates mu_bins [S, A] and every one of the G shapes, the multiplier c that maximises the interval-censored
    likelihood of the classes (dead [A, A], cens [A]: ade_classes') and the value there -> (ll [S, G], c [S, G] float64,
    flag [S] int32: 1 for a draw with a rate that is not finite or negative, or zero in a bin that holds a death - its rows
    are NaN); device tensors.  out: the (ll, c, flag) of an earlier call of the same sizes to write into."""
    torch = _torch()
    lib = _hip.load()
    dead = _dev(dead, torch.int64)
    dev = dead.device
    cens = _dev(cens, torch.int64, dev)
    mu = _dev(mu_bins, torch.float64, dev)
    sh = _dev(shapes, torch.float64, dev).reshape(-1)
    if mu.dim() != 2 or dead.dim() != 2 or dead.shape[0] != dead.shape[1] or cens.numel() != dead.shape[0] \
            or mu.shape[1] != dead.shape[0]:
        raise ValueError("shape mismatch: dead [A, A]; cens [A]; mu_bins [draws, A]; shapes [G]")
    S, A = (int(v) for v in mu.shape)
    G = int(sh.numel())
    nbytes = lib.lr_ade_profile_workspace_bytes(A, S, G)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_ade_profile_workspace_bytes")
    ll, c, flag = _ade_out(out, ((S, G), (S, G), (S,)), (torch.float64, torch.float64, torch.int32), dev, "(ll, c, flag)")
    ws = alloc_workspace(nbytes, dev, cached=True)
    rc = _hip.launch(lib.lr_ade_profile, dev, _hip.ptr(dead), _hip.ptr(cens), A, _hip.ptr(mu), S, _hip.ptr(sh), G, _hip.ptr(ll),
                     _hip.ptr(c), _hip.ptr(flag), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_ade_profile")
    return ll, c, flag


ADEJ_MOVES = ("mult", "shape", "add", "remove", "gibbs")
ADEJ_ROW_HEAD = ("it", "posterior", "lik", "prior", "shape", "log_shape", "K", "mean_rate", "rate_hp", "poi_hp")
ADEJ_STATE = {"K": 0, "log_shape": 1, "rate_hp": 2, "poi_hp": 3, "lik": 4, "prior": 5, "proposed": 6, "accepted": 11, "rates": 16,
              "times": 48}
AdejSettings = namedtuple("AdejSettings", "const use_rate_hp poisson_prior win", defaults=(0, 1, 0.0, 0.4))
AdejSettings.__doc__ = """The joint sampler's switches (include/literate_hip_adej.h): const - one rate, no RJ moves; use_rate_hp - 0: the
rates' Gamma prior keeps rate 1; poisson_prior - 0: hyper-prior on the Poisson rate of K, > 0: that fixed rate; win - width of
the window of the log-shape move."""


class AdejData:
    """lr_adej_prepare's workspace (a uint8 device tensor of exactly the queried size) and its bin count"""

    def __init__(self, ws, n_bins):
        self.ws, self.n_bins, self.device = ws, int(n_bins), ws.device


def adej_prepare(dead, cens, out=None):
    """The data side of the joint sampler of (death-rate skyline, Weibull shape) (lr_adej_prepare,
    include/literate_hip_adej.h): from ade_classes' dead [A, A] and cens [A] the numbers at risk and the class list ->
    AdejData, A <= LR_ADEJ_MAX_BINS.  out: the AdejData of an earlier call of the same size to write into."""
    torch = _torch()
    lib = _hip.load()
    dead = _dev(dead, torch.int64)
    dev = dead.device
    cens = _dev(cens, torch.int64, dev)
    if dead.dim() != 2 or dead.shape[0] != dead.shape[1] or cens.numel() != dead.shape[0]:
        raise ValueError("shape mismatch: dead [A, A]; cens [A]")
    A = int(cens.numel())
    nbytes = lib.lr_adej_workspace_bytes(A)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_adej_workspace_bytes")
    if out is None:
        ws = alloc_workspace(nbytes, dev)
    else:
        ws = out.ws
        if out.n_bins != A or ws.numel() != nbytes or ws.device != dev:
            raise ValueError("out must be the AdejData of a call of the same size")
    rc = _hip.launch(lib.lr_adej_prepare, dev, _hip.ptr(dead), _hip.ptr(cens), A, _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_adej_prepare")
    return AdejData(ws, A)


def adej_loglik(data, mu_bins, shapes, out=None):
    """l(mu, k) of the joint sampler's model for the S rows of mu_bins [S, A] and shapes [S] (lr_adej_loglik) -> (ll [S]
    float64, flag [S] int32: bit 0 a bad rate, bit 1 a bad shape; a flagged row is NaN); device tensors."""
    torch = _torch()
    lib = _hip.load()
    dev = data.device
    mu = _dev(mu_bins, torch.float64, dev)
    sh = _dev(shapes, torch.float64, dev).reshape(-1)
    if mu.dim() != 2 or mu.shape[1] != data.n_bins or sh.numel() != mu.shape[0]:
        raise ValueError("shape mismatch: mu_bins [S, A]; shapes [S]")
    S = int(mu.shape[0])
    ll, flag = _ade_out(out, ((S,), (S,)), (torch.float64, torch.int32), dev, "(ll, flag)")
    rc = _hip.launch(lib.lr_adej_loglik, dev, _hip.ptr(data.ws), data.ws.numel(), data.n_bins, _hip.ptr(mu), _hip.ptr(sh), S,
                     _hip.ptr(ll), _hip.ptr(flag))
    _hip.check(rc, "lr_adej_loglik")
    return ll, flag


def _adej_args(data, t0, st, seed, chain0, n_chains):
    return (_hip.ptr(data.ws), data.ws.numel(), data.n_bins, float(t0), int(st.const), int(st.use_rate_hp), float(st.poisson_prior),
            float(st.win), int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain0), int(n_chains))


def adej_init(data, t0, n_chains, seed, settings=AdejSettings(), chain0=0, out=None):
    """The initial state of chains chain0 .. chain0 + n_chains - 1 (lr_adej_init) -> state [n_chains, LR_ADEJ_STATE_W]
    (slots: ADEJ_STATE)."""
    torch = _torch()
    lib = _hip.load()
    (state,) = _ade_out(out, ((max(int(n_chains), 0), _hip.LR_ADEJ_STATE_W),), (torch.float64,), data.device, "(state,)")
    rc = _hip.launch(lib.lr_adej_init, data.device, *_adej_args(data, t0, settings, seed, chain0, n_chains), _hip.ptr(state))
    _hip.check(rc, "lr_adej_init")
    return state


def rows_due(it0, n_iters, s_freq):
    """the rows of a `steps` call (adej_steps, mlik_steps): one per iteration it0 .. it0 + n_iters - 1 with it % s_freq == 0"""
    s = int(s_freq)
    return (int(it0) + int(n_iters) + s - 1) // s - (int(it0) + s - 1) // s


def adej_steps(data, t0, state, it0, n_iters, s_freq, seed, settings=AdejSettings(), chain0=0, out=None):
    """Iterations it0 .. it0 + n_iters - 1 of every chain of `state` (updated in place; lr_adej_steps) -> rows [n, C,
    LR_ADEJ_ROW_W], one per chain and iteration with it % s_freq == 0 (columns: ADEJ_ROW_HEAD, then LR_KMAX rates and
    LR_KMAX - 1 shift times, NaN where unused)."""
    torch = _torch()
    lib = _hip.load()
    if state.dtype != torch.float64 or state.dim() != 2 or state.shape[1] != _hip.LR_ADEJ_STATE_W or not state.is_contiguous() \
            or state.device != data.device:
        raise ValueError("state must be adej_init's [chains, LR_ADEJ_STATE_W] float64 tensor on the data's device")
    C = int(state.shape[0])
    n = rows_due(it0, n_iters, s_freq) if int(s_freq) >= 1 and int(n_iters) >= 0 and int(it0) >= 0 else 0
    (rows,) = _ade_out(out, ((max(n, 0), C, _hip.LR_ADEJ_ROW_W),), (torch.float64,), data.device, "(rows,)")
    rc = _hip.launch(lib.lr_adej_steps, data.device, *_adej_args(data, t0, settings, seed, chain0, C), _hip.ptr(state), int(it0),
                     int(n_iters), int(s_freq), _hip.ptr(rows) if rows.numel() else None, n)
    _hip.check(rc, "lr_adej_steps")
    return rows


def adej_run(data, t0, n_chains, n_iter, s_freq, seed, settings=AdejSettings(), chain0=0):
    """A whole run of the joint sampler: lr_adej_init, then n_iter iterations in one launch -> (rows [n_iter / s_freq
    rounded up, n_chains, LR_ADEJ_ROW_W], state [n_chains, LR_ADEJ_STATE_W]); device tensors."""
    state = adej_init(data, t0, n_chains, seed, settings, chain0)
    rows = adej_steps(data, t0, state, 0, n_iter, s_freq, seed, settings, chain0)
    return rows, state


MLIK_ROW = ("it", "beta", "lik", "prior", "l_max", "k", "x0", "div_0", "L", "m_max", "nuB", "nuD")
MLIK_STATE = {"args": 0, "lik": 8, "prior": 9, "proposed": 10, "accepted": 12, "beta": 14, "scale": 15}
MlikEstimate = namedtuple("MlikEstimate", "stone ss lik_mean lik_var ti pooled")
MlikEstimate.__doc__ = """lr_mlik_estimate's results (include/literate_hip_mlik.h).  stone [R, T - 1], ss [R], lik_mean, lik_var [R, T], ti [R],
pooled [T] (the pooled stones and, last, their sum).  Device tensors."""


class MlikData:
    """The statistics the DDRate likelihood is a function of (create_bins' N_SPEC, N_EXTI, DT as float64 device tensors), the
    window and the model: what every lr_mlik_* call of one run shares."""

    def __init__(self, n_spec, n_exti, DT, origin, present, m_birth=2, m_death=2, init_death=0.1, device=None):
        torch = _torch()
        self.n_spec = _dev(n_spec, torch.float64, device).reshape(-1)
        self.device = self.n_spec.device
        self.n_exti = _dev(n_exti, torch.float64, self.device).reshape(-1)
        self.DT = _dev(DT, torch.float64, self.device).reshape(-1)
        if self.n_exti.numel() != self.n_spec.numel() or self.DT.numel() != self.n_spec.numel():
            raise ValueError("shape mismatch: n_spec, n_exti, DT [n_bins]")
        self.n_bins = int(self.DT.numel())
        self.origin, self.present, self.init_death = float(origin), float(present), float(init_death)
        self.m_birth, self.m_death = int(m_birth), int(m_death)


def _mlik_temps(betas, scales):
    b = np.ascontiguousarray(np.asarray(betas, dtype=np.float64).ravel())
    s = np.ascontiguousarray(np.asarray(scales, dtype=np.float64).ravel())
    if s.size != b.size:
        raise ValueError("shape mismatch: betas, scales [T]")
    return b, s


def _mlik_args(data, b, s, seed, rep0, n_reps):
    return (_hip.ptr(data.n_spec), _hip.ptr(data.n_exti), _hip.ptr(data.DT), data.n_bins, data.origin, data.present, data.m_birth,
            data.m_death, data.init_death, b.ctypes.data_as(_hip.c_vp), s.ctypes.data_as(_hip.c_vp), int(b.size),
            int(seed) & 0xFFFFFFFFFFFFFFFF, int(rep0), int(n_reps))


def mlik_init(data, betas, scales, n_reps, seed, rep0=0, out=None):
    """The initial state of replicates rep0 .. rep0 + n_reps - 1 at every temperature (lr_mlik_init) -> state [n_reps, T,
    LR_MLIK_STATE_W] (slots: MLIK_STATE)."""
    torch = _torch()
    lib = _hip.load()
    b, s = _mlik_temps(betas, scales)
    (state,) = _ade_out(out, ((max(int(n_reps), 0), int(b.size), _hip.LR_MLIK_STATE_W),), (torch.float64,), data.device, "(state,)")
    rc = _hip.launch(lib.lr_mlik_init, data.device, *_mlik_args(data, b, s, seed, rep0, n_reps), _hip.ptr(state))
    _hip.check(rc, "lr_mlik_init")
    return state


def mlik_steps(data, betas, scales, state, it0, n_iters, s_freq, seed, rep0=0, out=None):
    """Iterations it0 .. it0 + n_iters - 1 of every chain of `state` (updated in place; lr_mlik_steps) -> rows [n, R, T,
    LR_MLIK_ROW_W], one per chain and iteration with it % s_freq == 0 (columns: MLIK_ROW)."""
    torch = _torch()
    lib = _hip.load()
    b, s = _mlik_temps(betas, scales)
    if state.dtype != torch.float64 or state.dim() != 3 or state.shape[1] != b.size or state.shape[2] != _hip.LR_MLIK_STATE_W \
            or not state.is_contiguous() or state.device != data.device:
        raise ValueError("state must be mlik_init's [replicates, T, LR_MLIK_STATE_W] float64 tensor on the data's device")
    R = int(state.shape[0])
    n = rows_due(it0, n_iters, s_freq) if int(s_freq) >= 1 and int(n_iters) >= 0 and int(it0) >= 0 else 0
    (rows,) = _ade_out(out, ((max(n, 0), R, int(b.size), _hip.LR_MLIK_ROW_W),), (torch.float64,), data.device, "(rows,)")
    rc = _hip.launch(lib.lr_mlik_steps, data.device, *_mlik_args(data, b, s, seed, rep0, R), _hip.ptr(state), int(it0), int(n_iters),
                     int(s_freq), _hip.ptr(rows) if rows.numel() else None, n)
    _hip.check(rc, "lr_mlik_steps")
    return rows


def mlik_run(data, betas, scales, n_reps, n_iter, s_freq, seed, rep0=0):
    """A whole run of the power-posterior chains: lr_mlik_init, then n_iter iterations in one launch -> (rows [n_iter / s_freq
    rounded up, n_reps, T, LR_MLIK_ROW_W], state [n_reps, T, LR_MLIK_STATE_W]); device tensors."""
    state = mlik_init(data, betas, scales, n_reps, seed, rep0)
    rows = mlik_steps(data, betas, scales, state, 0, n_iter, s_freq, seed, rep0)
    return rows, state


def mlik_estimate(rows, betas, row0=0, n_rows=None, out=None):
    """Stepping-stone and thermodynamic-integration estimates of log Z from rows [>= n_rows, R, T, LR_MLIK_ROW_W], rows
    row0 .. n_rows - 1 of every chain (lr_mlik_estimate) -> MlikEstimate."""
    torch = _torch()
    lib = _hip.load()
    rows = _dev(rows, torch.float64)
    b = np.ascontiguousarray(np.asarray(betas, dtype=np.float64).ravel())
    if rows.dim() != 4 or rows.shape[2] != b.size or rows.shape[3] != _hip.LR_MLIK_ROW_W:
        raise ValueError("rows must be [n_rows, replicates, T, LR_MLIK_ROW_W] with T = len(betas)")
    n = int(rows.shape[0]) if n_rows is None else int(n_rows)
    if n > rows.shape[0]:
        raise ValueError("rows holds fewer than n_rows rows")
    R, T = int(rows.shape[1]), int(b.size)
    res = _ade_out(out, ((R, max(T - 1, 0)), (R,), (R, T), (R, T), (R,), (T,)), (torch.float64,) * 6, rows.device, "MlikEstimate")
    rc = _hip.launch(lib.lr_mlik_estimate, rows.device, _hip.ptr(rows), n, R, T, int(row0), b.ctypes.data_as(_hip.c_vp),
                     *[_hip.ptr(t) for t in res])
    _hip.check(rc, "lr_mlik_estimate")
    return MlikEstimate(*res)


TMLIK_ROW = ("it", "beta", "lik", "prior", "l_min", "m_min", "alpha", "beta_slope", "delta", "gamma", "win", "model")
TMLIK_STATE = {"args": 0, "lik": 6, "prior": 7, "proposed": 8, "accepted": 10, "beta": 12, "scale": 13, "win": 14, "model": 15}


class TmlikData:
    """The statistics the trend likelihood is a function of (create_bins' N_SPEC, N_EXTI, DT [n_bins]) and the normalised
    covariates trends [n_cols, n_bins], as float64 device tensors: what every lr_tmlik_* call of one run shares."""

    def __init__(self, n_spec, n_exti, DT, trends, device=None):
        torch = _torch()
        self.n_spec = _dev(n_spec, torch.float64, device).reshape(-1)
        self.device = self.n_spec.device
        self.n_exti = _dev(n_exti, torch.float64, self.device).reshape(-1)
        self.DT = _dev(DT, torch.float64, self.device).reshape(-1)
        self.trends = _dev(trends, torch.float64, self.device)
        if self.trends.dim() == 1:
            self.trends = self.trends.reshape(1, -1)
        self.n_bins = int(self.DT.numel())
        if self.n_exti.numel() != self.n_bins or self.n_spec.numel() != self.n_bins or self.trends.dim() != 2 \
                or self.trends.shape[1] != self.n_bins:
            raise ValueError("shape mismatch: n_spec, n_exti, DT [n_bins]; trends [n_cols, n_bins]")
        self.n_cols = int(self.trends.shape[0])


class TmlikGrid:
    """The chain grid of one run of lr_tmlik_*: the models (col, flags: bit 0 const_B, bit 1 const_D, key0) [M], the ladder
    betas, scales [T] - host arrays that travel in the kernel arguments - and the replicates."""

    def __init__(self, col, flags, key0, betas, scales, n_reps):
        self.col = np.ascontiguousarray(np.asarray(col, dtype=np.int32).ravel())
        self.flags = np.ascontiguousarray(np.asarray(flags, dtype=np.int32).ravel())
        self.key0 = np.ascontiguousarray(np.asarray(key0, dtype=np.int64).ravel())
        self.betas, self.scales = _mlik_temps(betas, scales)
        if self.flags.size != self.col.size or self.key0.size != self.col.size:
            raise ValueError("shape mismatch: col, flags, key0 [M]")
        self.M, self.T, self.R = int(self.col.size), int(self.betas.size), int(n_reps)

    def part(self, models=None, reps=None):
        """the grid of models [a, b) and / or replicates [a, b) of this one: the same chains, by key0"""
        ma, mb = models if models is not None else (0, self.M)
        ra, rb = reps if reps is not None else (0, self.R)
        return TmlikGrid(self.col[ma:mb], self.flags[ma:mb], self.key0[ma:mb] + ra, self.betas, self.scales, rb - ra)


def tmlik_problem(data, grid, wins, state, seed):
    """The descriptor of a call (_hip.TmlikProblem; it refers to the arrays of data, grid, wins and state: keep them alive
    while it is used).  wins [M, T], state [M, R, T, LR_TMLIK_STATE_W]: float64 device tensors."""
    vp = lambda a: a.ctypes.data_as(_hip.c_vp)
    return _hip.TmlikProblem(_hip.ptr(data.n_spec), _hip.ptr(data.n_exti), _hip.ptr(data.DT), _hip.ptr(data.trends), _hip.ptr(wins),
                             _hip.ptr(state), vp(grid.betas), vp(grid.scales), vp(grid.col), vp(grid.flags), vp(grid.key0),
                             data.n_bins, data.n_cols, grid.M, grid.R, grid.T, int(seed) & 0xFFFFFFFFFFFFFFFF, None)


def _tmlik_wins(data, grid, wins):
    torch = _torch()
    w = _dev(np.full((grid.M, grid.T), float(wins)) if np.isscalar(wins) else wins, torch.float64, data.device)
    if tuple(w.shape) != (grid.M, grid.T):
        raise ValueError("wins must be [models, T]")
    return w


def tmlik_init(data, grid, wins, seed, out=None):
    """The initial state of every chain of the grid (lr_tmlik_init) -> state [M, R, T, LR_TMLIK_STATE_W] (slots: TMLIK_STATE).
    wins: the additive windows [M, T] (a device tensor is used as it is; a number: that window everywhere)."""
    torch = _torch()
    lib = _hip.load()
    w = _tmlik_wins(data, grid, wins)
    (state,) = _ade_out(out, ((grid.M, max(grid.R, 0), grid.T, _hip.LR_TMLIK_STATE_W),), (torch.float64,), data.device, "(state,)")
    rc = _hip.launch_problem(lib.lr_tmlik_init, data.device, tmlik_problem(data, grid, w, state, seed))
    _hip.check(rc, "lr_tmlik_init")
    return state


def tmlik_steps(data, grid, wins, state, it0, n_iters, s_freq, seed, rows=None, slot0=0, out=None):
    """Iterations it0 .. it0 + n_iters - 1 of every chain of `state` (updated in place; lr_tmlik_steps) -> rows [M, cap, R, T,
    LR_TMLIK_ROW_W] (columns: TMLIK_ROW), models outermost: rows[m] is what mlik_estimate reads.  rows: an earlier call's
    buffer to go on writing into at slot `slot0`; otherwise a fresh one of exactly the rows due."""
    torch = _torch()
    lib = _hip.load()
    w = _tmlik_wins(data, grid, wins)
    if state.dtype != torch.float64 or tuple(state.shape) != (grid.M, grid.R, grid.T, _hip.LR_TMLIK_STATE_W) \
            or not state.is_contiguous() or state.device != data.device:
        raise ValueError("state must be tmlik_init's [models, replicates, T, LR_TMLIK_STATE_W] float64 tensor on the data's device")
    n = rows_due(it0, n_iters, s_freq) if int(s_freq) >= 1 and int(n_iters) >= 0 and int(it0) >= 0 else 0
    if rows is None:
        (rows,) = _ade_out(out, ((grid.M, max(n, 0), grid.R, grid.T, _hip.LR_TMLIK_ROW_W),), (torch.float64,), data.device, "(rows,)")
    elif rows.dtype != torch.float64 or rows.dim() != 5 or not rows.is_contiguous() or rows.device != data.device \
            or (rows.shape[0], rows.shape[2], rows.shape[3], rows.shape[4]) != (grid.M, grid.R, grid.T, _hip.LR_TMLIK_ROW_W):
        raise ValueError("rows must be a [models, cap, replicates, T, LR_TMLIK_ROW_W] float64 tensor on the data's device")
    rc = _hip.launch_problem(lib.lr_tmlik_steps, data.device, tmlik_problem(data, grid, w, state, seed), int(it0), int(n_iters),
                             int(s_freq), _hip.ptr(rows) if rows.numel() else None, int(rows.shape[1]), int(slot0))
    _hip.check(rc, "lr_tmlik_steps")
    return rows


def tmlik_run(data, grid, wins, n_iter, s_freq, seed):
    """A whole run at fixed windows: lr_tmlik_init, then n_iter iterations in one launch -> (rows [M, n_iter / s_freq rounded
    up, R, T, LR_TMLIK_ROW_W], state [M, R, T, LR_TMLIK_STATE_W]); device tensors."""
    w = _tmlik_wins(data, grid, wins)
    state = tmlik_init(data, grid, w, seed)
    rows = tmlik_steps(data, grid, w, state, 0, n_iter, s_freq, seed)
    return rows, state


RJBIN_ROWS = {"L": 0, "M": 1, "tL": 2, "tM": 3, "eL": 4, "eM": 5, "scalars": 6}
RJBIN_SCALARS = {"likA": 0, "priorA": 1, "priorPoiA": 2, "Gamma_rate_l": 3, "Gamma_rate_m": 4, "Poi_lambda": 5, "K_l": 6, "K_m": 7,
                 "accepted": 8}
RjbinSettings = namedtuple("RjbinSettings", "model const_rates const_death_rate use_rate_HP poisson_HP update_fraction",
                           defaults=(2, 0, 0, 1, 0.0, 0.75))


class RjbinData:
    """The per-replicate statistics the RJ sampler's likelihood is a function of: sp, ex, br [R, n_bins] (and ex_dead, br_dead
    for model 3) with start_time, end_time [R], as float64 device tensors, and the warning word: what every lr_rjbin_* call
    of one run shares.  Chain c belongs to replicate c // chains_per_rep."""

    def __init__(self, sp, ex, br, start_time, end_time, chains_per_rep, ex_dead=None, br_dead=None, device=None):
        torch = _torch()
        self.sp = _dev(sp, torch.float64, device)
        if self.sp.dim() == 1:
            self.sp = self.sp.reshape(1, -1)
        self.device = self.sp.device
        two = lambda x: None if x is None else _dev(x, torch.float64, self.device).reshape(-1, self.sp.shape[-1])
        self.ex, self.br, self.ex_dead, self.br_dead = two(ex), two(br), two(ex_dead), two(br_dead)
        self.start_time = _dev(start_time, torch.float64, self.device).reshape(-1)
        self.end_time = _dev(end_time, torch.float64, self.device).reshape(-1)
        self.R, self.n_bins = int(self.sp.shape[0]), int(self.sp.shape[1])
        if self.sp.dim() != 2 or any(t is not None and tuple(t.shape) != (self.R, self.n_bins)
                                     for t in (self.ex, self.br, self.ex_dead, self.br_dead)) \
                or self.start_time.numel() != self.R or self.end_time.numel() != self.R:
            raise ValueError("shape mismatch: sp, ex, br[, ex_dead, br_dead] [R, n_bins]; start_time, end_time [R]")
        self.chains_per_rep = int(chains_per_rep)
        self.n_chains = self.R * self.chains_per_rep
        # (read and written, bits OR-ed in: the caller's to clear, so not an output of the seam)
        self.warn = torch.zeros(1, dtype=torch.int32, device=self.device)

    def warnings(self):
        """the warning word (LR_WARN_* bits; a device read-back)"""
        return int(self.warn.item())


def rjbin_problem(data, state, seed, settings=RjbinSettings(), chain0=0):
    """The descriptor of a call (_hip.RjbinProblem; it refers to the tensors of data and state: keep them alive while it is
    used)."""
    st = settings
    return _hip.RjbinProblem(_hip.ptr(data.sp), _hip.ptr(data.ex), _hip.ptr(data.br), _hip.ptr(data.ex_dead), _hip.ptr(data.br_dead),
                             _hip.ptr(data.start_time), _hip.ptr(data.end_time), _hip.ptr(state), _hip.ptr(data.warn),
                             data.n_bins, data.R, data.chains_per_rep, int(st.model), int(st.const_rates), int(st.const_death_rate),
                             int(st.use_rate_HP), int(chain0), float(st.poisson_HP), float(st.update_fraction),
                             int(seed) & 0xFFFFFFFFFFFFFFFF, None)


def rjbin_init(data, seed, settings=RjbinSettings(), chain0=0, init=None, out=None):
    """The initial state of every chain (lr_rjbin_init) -> state [C, LR_RJBIN_STATE_W] (rows: RJBIN_ROWS, scalars:
    RJBIN_SCALARS).  init: (L, M [C, <= LR_KMAX], tL, tM [C, <= LR_KMAX + 1], K_l, K_m [C]) to start from, padded here to the
    ABI's widths; None: the CLI's start."""
    torch = _torch()
    lib = _hip.load()
    C = data.n_chains
    (state,) = _ade_out(out, ((max(C, 0), _hip.LR_RJBIN_STATE_W),), (torch.float64,), data.device, "(state,)")
    six = [None] * 6
    if init is not None:
        L, M, tL, tM, KL, KM = init

        def pad(x, w):
            x = _host_f64(x).reshape(C, -1)
            if x.shape[1] > w:
                raise ValueError("init: at most LR_KMAX = %d rates (and one more time) per chain" % _hip.LR_KMAX)
            full = np.zeros((C, w))
            full[:, :x.shape[1]] = x
            return _dev(full, torch.float64, data.device)
        _check_host_K(KL, _hip.LR_KMAX, "K_l"), _check_host_K(KM, _hip.LR_KMAX, "K_m")
        six = [pad(L, _hip.LR_KMAX), pad(M, _hip.LR_KMAX), pad(tL, _hip.LR_KMAX + 1), pad(tM, _hip.LR_KMAX + 1),
               _dev(KL, torch.int32, data.device).reshape(-1), _dev(KM, torch.int32, data.device).reshape(-1)]
        if six[4].numel() != C or six[5].numel() != C:
            raise ValueError("init: K_l, K_m [C]")
    rc = _hip.launch_problem(lib.lr_rjbin_init, data.device, rjbin_problem(data, state, seed, settings, chain0),
                             *[_hip.ptr(t) for t in six])
    _hip.check(rc, "lr_rjbin_init")
    return state


def rjbin_steps(data, state, it0, n_iters, s_freq, seed, settings=RjbinSettings(), chain0=0, rows=None, slot0=0, out=None):
    """Iterations it0 .. it0 + n_iters - 1 of every chain of `state` (updated in place; lr_rjbin_steps) -> rows [cap, C,
    LR_TRACE_W], the engines' trace rows.  rows: an earlier call's buffer to go on writing into at slot `slot0`; otherwise a
    fresh one of exactly the rows due."""
    torch = _torch()
    lib = _hip.load()
    C = data.n_chains
    if state.dtype != torch.float64 or tuple(state.shape) != (C, _hip.LR_RJBIN_STATE_W) or not state.is_contiguous() \
            or state.device != data.device:
        raise ValueError("state must be rjbin_init's [C, LR_RJBIN_STATE_W] float64 tensor on the data's device")
    n = rows_due(it0, n_iters, s_freq) if int(s_freq) >= 1 and int(n_iters) >= 0 and int(it0) >= 0 else 0
    if rows is None:
        (rows,) = _ade_out(out, ((max(n, 0), C, _hip.LR_TRACE_W),), (torch.float64,), data.device, "(rows,)")
    elif rows.dtype != torch.float64 or rows.dim() != 3 or not rows.is_contiguous() or rows.device != data.device \
            or tuple(rows.shape[1:]) != (C, _hip.LR_TRACE_W):
        raise ValueError("rows must be a [cap, C, LR_TRACE_W] float64 tensor on the data's device")
    rc = _hip.launch_problem(lib.lr_rjbin_steps, data.device, rjbin_problem(data, state, seed, settings, chain0), int(it0),
                             int(n_iters), int(s_freq), _hip.ptr(rows) if rows.numel() else None, int(rows.shape[0]), int(slot0))
    _hip.check(rc, "lr_rjbin_steps")
    return rows


PARBIN_STATE = {"args": 0, "lik": 8, "prior": 9, "proposed": 10, "accepted": 12}
PARBIN_NPAR = {1: 8, 2: 6}
# sampler 1: DDRate (m_birth, m_death as dd_rates; init_death = -fix_death); 2: trend_rate (m_birth, m_death = -const_B, -const_D)
ParbinSettings = namedtuple("ParbinSettings", "sampler m_birth m_death init_death", defaults=(1, 2, 2, 0.1))


class ParbinData:
    """The per-replicate statistics the parametric samplers' likelihoods are functions of: n_spec, n_exti, DT [R, n_bins] with
    origin, present [R] (create_bins' values) and, for trend_rate, the normalised covariate trend [n_bins] all replicates
    share, as float64 device tensors: what every lr_parbin_* call of one run shares.  Chain c belongs to replicate c //
    chains_per_rep."""

    def __init__(self, n_spec, n_exti, DT, origin, present, chains_per_rep, trend=None, device=None):
        torch = _torch()
        self.n_spec = _dev(n_spec, torch.float64, device)
        if self.n_spec.dim() == 1:
            self.n_spec = self.n_spec.reshape(1, -1)
        self.device = self.n_spec.device
        two = lambda x: _dev(x, torch.float64, self.device).reshape(-1, self.n_spec.shape[-1])
        self.n_exti, self.DT = two(n_exti), two(DT)
        one = lambda x: _dev(x if isinstance(x, torch.Tensor) else np.atleast_1d(np.asarray(x, dtype=np.float64)), torch.float64,
                             self.device).reshape(-1)
        self.origin, self.present = one(origin), one(present)
        self.trend = None if trend is None else _dev(trend, torch.float64, self.device).reshape(-1)
        self.R, self.n_bins = int(self.n_spec.shape[0]), int(self.n_spec.shape[1])
        if self.n_spec.dim() != 2 or any(tuple(t.shape) != (self.R, self.n_bins) for t in (self.n_exti, self.DT)) \
                or self.origin.numel() != self.R or self.present.numel() != self.R \
                or (self.trend is not None and self.trend.numel() != self.n_bins):
            raise ValueError("shape mismatch: n_spec, n_exti, DT [R, n_bins]; origin, present [R]; trend [n_bins]")
        self.chains_per_rep = int(chains_per_rep)
        self.n_chains = self.R * self.chains_per_rep


def parbin_problem(data, state, seed, settings=ParbinSettings(), chain0=0):
    """The descriptor of a call (_hip.ParbinProblem; it refers to the tensors of data and state: keep them alive while it is
    used)."""
    st = settings
    return _hip.ParbinProblem(_hip.ptr(data.n_spec), _hip.ptr(data.n_exti), _hip.ptr(data.DT), _hip.ptr(data.origin),
                              _hip.ptr(data.present), _hip.ptr(data.trend), _hip.ptr(state), data.n_bins, data.R,
                              data.chains_per_rep, int(st.sampler), int(st.m_birth), int(st.m_death), float(st.init_death),
                              int(chain0), int(seed) & 0xFFFFFFFFFFFFFFFF, None)


def parbin_init(data, seed, settings=ParbinSettings(), chain0=0, out=None):
    """The initial state of every chain (lr_parbin_init) -> state [C, LR_PARBIN_STATE_W] (elements: PARBIN_STATE)."""
    torch = _torch()
    lib = _hip.load()
    (state,) = _ade_out(out, ((max(data.n_chains, 0), _hip.LR_PARBIN_STATE_W),), (torch.float64,), data.device, "(state,)")
    rc = _hip.launch_problem(lib.lr_parbin_init, data.device, parbin_problem(data, state, seed, settings, chain0))
    _hip.check(rc, "lr_parbin_init")
    return state


def parbin_steps(data, state, it0, n_iters, s_freq, seed, settings=ParbinSettings(), chain0=0, rows=None, slot0=0, out=None):
    """Iterations it0 .. it0 + n_iters - 1 of every chain of `state` (updated in place; lr_parbin_steps) -> rows [cap, C,
    LR_TRACE_W], the engines' trace rows of the sampler.  rows: an earlier call's buffer to go on writing into at slot
    `slot0`; otherwise a fresh one of exactly the rows due."""
    torch = _torch()
    lib = _hip.load()
    C = data.n_chains
    if state.dtype != torch.float64 or tuple(state.shape) != (C, _hip.LR_PARBIN_STATE_W) or not state.is_contiguous() \
            or state.device != data.device:
        raise ValueError("state must be parbin_init's [C, LR_PARBIN_STATE_W] float64 tensor on the data's device")
    n = rows_due(it0, n_iters, s_freq) if int(s_freq) >= 1 and int(n_iters) >= 0 and int(it0) >= 0 else 0
    if rows is None:
        (rows,) = _ade_out(out, ((max(n, 0), C, _hip.LR_TRACE_W),), (torch.float64,), data.device, "(rows,)")
    elif rows.dtype != torch.float64 or rows.dim() != 3 or not rows.is_contiguous() or rows.device != data.device \
            or tuple(rows.shape[1:]) != (C, _hip.LR_TRACE_W):
        raise ValueError("rows must be a [cap, C, LR_TRACE_W] float64 tensor on the data's device")
    rc = _hip.launch_problem(lib.lr_parbin_steps, data.device, parbin_problem(data, state, seed, settings, chain0), int(it0),
                             int(n_iters), int(s_freq), _hip.ptr(rows) if rows.numel() else None, int(rows.shape[0]), int(slot0))
    _hip.check(rc, "lr_parbin_steps")
    return rows


MTE_STATE = {"m": 0, "beta_hp": 1, "lik": 2, "prior": 3, "proposed": 4, "accepted": 7, "I": 16, "sd": 32, "Y": 48}
MTE_MOVES = ("Y", "m", "indicator")
# bvs: Bayesian variable selection (-bvs); constant: only m moves (-const 1); bvs_from: the first iteration an indicator may flip
# at (the reference's `iteration > 1000`); pI: the prior probability of an indicator
MteSettings = namedtuple("MteSettings", "bvs constant bvs_from pI", defaults=(1, 0, 1001, 0.05))


def mte_row_columns(n_states):
    """where a row of lr_mte_steps keeps what: {"I": slice, "q": slice, "sd": slice, "beta_hp": int, "width": int} (it, posterior,
    likelihood, prior, m are columns 0 .. 4)"""
    T, nc = len(n_states), int(np.sum(n_states))
    return {"I": slice(5, 5 + T), "q": slice(5 + T, 5 + T + nc), "sd": slice(5 + T + nc, 5 + 2 * T + nc), "beta_hp": 5 + 2 * T + nc,
            "width": 6 + 2 * T + nc}


def mte_slice(ts, te, t0, t1):
    """The time slice (t0, t1], t0 > t1 in time before the present (MTEmodel.py:145-155): the lineages with te < t0 and ts > t1,
    ts clipped to t0, both times shifted by -t1, te <= 0 set to 0 (extant in the slice) -> (kept [n] bool, bl, ex of the kept)"""
    ts, te = np.asarray(ts, dtype=np.float64), np.asarray(te, dtype=np.float64)
    kept = (te < t0) & (ts > t1)
    s, e = np.minimum(ts[kept], t0) - t1, te[kept] - t1
    e = np.where(e <= 0, 0.0, e)
    return kept, s - e, (e > 0).astype(np.float64)


def mte_tables(ts, te, traits, slices):
    """The sufficient statistics of the multi-trait extinction model, in numpy: traits [n, T] of any sortable values; slices
    [(t0, t1)].  The states of a column are its distinct values in the WHOLE table, mapped in sorted order to 0 .. S_t - 1; the
    combinations are the distinct rows of the mapped table, in lexicographic order, shared by all slices.
    -> {"code" [G, T] uint8, "n_states" [T] int32, "states" [per trait the sorted values], "combo" [n] (the combination of every
    lineage), "n", "E", "B" [P, G] float64 (lineages, extinctions, lineage-time per slice and combination)}"""
    traits = np.asarray(traits)
    if traits.ndim == 1:
        traits = traits.reshape(-1, 1)
    n_lin, T = traits.shape
    states, mapped = [], np.zeros((n_lin, T), dtype=np.int64)
    for t in range(T):
        u, inv = np.unique(traits[:, t], return_inverse=True)
        states.append(u)
        mapped[:, t] = inv.reshape(-1)
    code, combo = np.unique(mapped, axis=0, return_inverse=True)
    combo = combo.reshape(-1)
    G, P = code.shape[0], len(slices)
    n, E, B = np.zeros((P, G)), np.zeros((P, G)), np.zeros((P, G))
    for p, (t0, t1) in enumerate(slices):
        kept, bl, ex = mte_slice(ts, te, t0, t1)
        g = combo[kept]
        n[p] = np.bincount(g, minlength=G)
        E[p] = np.bincount(g, weights=ex, minlength=G)
        B[p] = np.bincount(g, weights=bl, minlength=G)
    return {"code": code.astype(np.uint8) if code.max(initial=0) < 256 else code, "n_states": np.array([len(u) for u in states], dtype=np.int32),
            "states": states, "combo": combo, "n": n, "E": E, "B": B}


class MteData:
    """What every lr_mte_* call of one run shares (include/literate_hip_mte.h): code [G, T] uint8 and n_states [T] int32 with
    its host copy, n, E, B [P, G] float64 - device tensors -, the traits' names and the slices' bounds.  Chain c belongs to
    problem c // chains_per_problem.  Host arrays are checked here (a code must lie below its trait's number of states);
    device tensors are used as they are, with n_states_host given beside them."""

    def __init__(self, code, n_states, n, E, B, chains_per_problem=1, names=None, slices=None, n_states_host=None, device=None):
        torch = _torch()
        if n_states_host is None:
            n_states_host = n_states.cpu().numpy() if hasattr(n_states, "cpu") else n_states
        self.n_states_host = np.ascontiguousarray(np.asarray(n_states_host, dtype=np.int32).reshape(-1))
        if not hasattr(code, "is_cuda"):
            code = np.asarray(code)
            if code.ndim != 2 or code.shape[1] != self.n_states_host.size or code.shape[0] < 1:
                raise ValueError("code must be [G, T] with one column per entry of n_states")
            if (code < 0).any() or (code >= self.n_states_host[None, :]).any():
                raise ValueError("a code lies outside 0 .. S_t - 1 of its trait")
        self.code = _dev(code, torch.uint8, device)
        self.device = self.code.device
        self.n_states = _dev(n_states, torch.int32, self.device).reshape(-1)
        self.G, self.T = int(self.code.shape[0]), int(self.code.shape[1]) if self.code.dim() == 2 else 0
        two = lambda x: _dev(x, torch.float64, self.device).reshape(-1, self.G)
        self.n, self.E, self.B = two(n), two(E), two(B)
        self.P = int(self.n.shape[0])
        if self.code.dim() != 2 or self.n_states.numel() != self.T or self.n_states_host.size != self.T \
                or any(tuple(t.shape) != (self.P, self.G) for t in (self.E, self.B)):
            raise ValueError("shape mismatch: code [G, T]; n_states [T]; n, E, B [P, G]")
        self.n_cats = int(self.n_states_host.sum())
        self.chains_per_problem = int(chains_per_problem)
        self.n_chains = self.P * self.chains_per_problem
        self.names = list(names) if names is not None else ["t%d" % t for t in range(self.T)]
        self.slices = list(slices) if slices is not None else [(np.inf, 0.0)] * self.P

    @classmethod
    def from_lineages(cls, ts, te, traits, slices, chains_per_problem=1, names=None, device=None):
        """the slicing, state mapping and grouping of mte_tables, uploaded; the tables stay in .tables"""
        tab = mte_tables(ts, te, traits, slices)
        if tab["code"].dtype != np.uint8:
            raise ValueError("a trait with more than 255 states")
        data = cls(tab["code"], tab["n_states"], tab["n"], tab["E"], tab["B"], chains_per_problem, names, slices, device=device)
        data.tables = tab
        return data


def mte_problem(data, state, seed, settings=MteSettings(), chain0=0):
    """The descriptor of a call (_hip.MteProblem; it refers to the tensors of data and state and to data.n_states_host: keep
    them alive while it is used)."""
    st = settings
    return _hip.MteProblem(_hip.ptr(data.code), _hip.ptr(data.n_states), data.n_states_host.ctypes.data_as(_hip.c_vp), _hip.ptr(data.n),
                           _hip.ptr(data.E), _hip.ptr(data.B), _hip.ptr(state), data.G, data.T, data.P, data.chains_per_problem,
                           int(st.bvs), int(st.constant), int(st.bvs_from), float(st.pI), int(chain0), int(seed) & 0xFFFFFFFFFFFFFFFF,
                           None)


def mte_state(data, m, Y, I, sd=None, beta_hp=1.0):
    """A host state [C, LR_MTE_STATE_W] holding the parameters of every chain, for mte_init(given=...): m [C]; Y [C, sum S_t],
    the traits concatenated; I [C, T]; sd [C, T] (1 where not given); beta_hp [C] or a number.  Likelihood, prior and counters 0."""
    C, S = data.n_chains, MTE_STATE
    st = np.zeros((C, _hip.LR_MTE_STATE_W))
    st[:, S["m"]] = np.broadcast_to(np.asarray(m, dtype=np.float64), (C,))
    st[:, S["beta_hp"]] = np.broadcast_to(np.asarray(beta_hp, dtype=np.float64), (C,))
    st[:, S["I"]:S["I"] + data.T] = np.broadcast_to(np.asarray(I, dtype=np.float64), (C, data.T))
    st[:, S["sd"]:S["sd"] + data.T] = 1.0 if sd is None else np.broadcast_to(np.asarray(sd, dtype=np.float64), (C, data.T))
    st[:, S["Y"]:S["Y"] + data.n_cats] = np.broadcast_to(np.asarray(Y, dtype=np.float64), (C, data.n_cats))
    return st


def mte_init(data, seed, settings=MteSettings(), chain0=0, given=None, out=None):
    """The initial state of every chain (lr_mte_init) -> state [C, LR_MTE_STATE_W] (elements: MTE_STATE).  given: a state whose
    m, beta_hp, I, sd and Y the caller wrote (mte_state): they are kept, and their likelihood, prior and zeroed counters
    added."""
    torch = _torch()
    lib = _hip.load()
    (state,) = _ade_out(out, ((max(data.n_chains, 0), _hip.LR_MTE_STATE_W),), (torch.float64,), data.device, "(state,)")
    if given is not None:
        g = _dev(given, torch.float64, data.device)
        if tuple(g.shape) != tuple(state.shape):
            raise ValueError("given must be a [C, LR_MTE_STATE_W] state")
        state.copy_(g)
    rc = _hip.launch_problem(lib.lr_mte_init, data.device, mte_problem(data, state, seed, settings, chain0), 0 if given is None else 1)
    _hip.check(rc, "lr_mte_init")
    return state


def mte_steps(data, state, it0, n_iters, s_freq, seed, settings=MteSettings(), chain0=0, rows=None, slot0=0, out=None):
    """Iterations it0 .. it0 + n_iters - 1 of every chain of `state` (updated in place; lr_mte_steps) -> rows [cap, C,
    LR_MTE_ROW_W] (columns: mte_row_columns).  rows: an earlier call's buffer to go on writing into at slot `slot0`; otherwise a
    fresh one of exactly the rows due."""
    torch = _torch()
    lib = _hip.load()
    C = data.n_chains
    if state.dtype != torch.float64 or tuple(state.shape) != (C, _hip.LR_MTE_STATE_W) or not state.is_contiguous() \
            or state.device != data.device:
        raise ValueError("state must be mte_init's [C, LR_MTE_STATE_W] float64 tensor on the data's device")
    n = rows_due(it0, n_iters, s_freq) if int(s_freq) >= 1 and int(n_iters) >= 0 and int(it0) >= 0 else 0
    if rows is None:
        (rows,) = _ade_out(out, ((max(n, 0), C, _hip.LR_MTE_ROW_W),), (torch.float64,), data.device, "(rows,)")
    elif rows.dtype != torch.float64 or rows.dim() != 3 or not rows.is_contiguous() or rows.device != data.device \
            or tuple(rows.shape[1:]) != (C, _hip.LR_MTE_ROW_W):
        raise ValueError("rows must be a [cap, C, LR_MTE_ROW_W] float64 tensor on the data's device")
    rc = _hip.launch_problem(lib.lr_mte_steps, data.device, mte_problem(data, state, seed, settings, chain0), int(it0), int(n_iters),
                             int(s_freq), _hip.ptr(rows) if rows.numel() else None, int(rows.shape[0]), int(slot0))
    _hip.check(rc, "lr_mte_steps")
    return rows


def mte_run(data, n_iter, s_freq, seed, settings=MteSettings(), chain0=0):
    """mte_init, then iterations 0 .. n_iter - 1 in one launch -> (rows, state)"""
    state = mte_init(data, seed, settings, chain0)
    return mte_steps(data, state, 0, n_iter, s_freq, seed, settings, chain0), state


def mte_loglik(data, m, Y, I, sd=None, beta_hp=1.0, settings=MteSettings()):
    """The log-likelihood and log prior of given parameters, one set per chain (lr_mte_init with given = 1; arguments as
    mte_state's) -> (lik [C], prior [C]), device tensors"""
    state = mte_init(data, 0, settings, given=mte_state(data, m, Y, I, sd, beta_hp))
    return state[:, MTE_STATE["lik"]].clone(), state[:, MTE_STATE["prior"]].clone()


MTREND_STATE = {"l0": 0, "m0": 1, "lik_b": 2, "lik_d": 3, "prior": 4, "E_b": 5, "E_d": 6, "proposed": 8, "accepted": 16, "I_l": 32, "a": 48,
                "I_m": 64, "b": 80}
# the counters' elements; the last two count the coefficient moves where I_j = 1, what a window is tuned from
MTREND_MOVES = ("multiplier", "coef_birth", "coef_death", "flip", "coef_birth_included", "coef_death_included")
# m_birth / m_death: 1 = the side is constant (-const_B / -const_D); no_death: the death side leaves the likelihood; bvs: the
# indicators flip, from iteration bvs_from on; pI: the prior probability of an indicator; slab_sd: the sd of the Normal prior on
# a coefficient; win: the sd of a coefficient's step (birth, death)
MtrendSettings = namedtuple("MtrendSettings", "m_birth m_death no_death bvs bvs_from pI slab_sd win", defaults=(0, 0, 0, 1, 0, 0.1, 1.0, (0.1, 0.1)))


def mtrend_row_columns(P):
    """where a row of lr_mtrend_steps keeps what: {"I_l", "a", "I_m", "b": slices, "width": int} (it, posterior, likelihood,
    likelihood_birth, likelihood_death, prior, l0, m0 are columns 0 .. 7)"""
    P = int(P)
    return {"I_l": slice(8, 8 + P), "a": slice(8 + P, 8 + 2 * P), "I_m": slice(8 + 2 * P, 8 + 3 * P), "b": slice(8 + 3 * P, 8 + 4 * P),
            "width": 8 + 4 * P}


class MtrendData:
    """What every lr_mtrend_* call of one run shares (include/literate_hip_mtrend.h): n_spec, n_exti, DT [n_bins] and X [P,
    n_bins] float64 - device tensors -, SX of both sides [P] on the host, the number of chains and the covariates' names.  Host
    arrays are uploaded and SX is taken from them; device tensors are used as they are (sx = (sx_spec, sx_exti) given beside
    them spares the read-back)."""

    def __init__(self, n_spec, n_exti, DT, X, n_chains=1, names=None, sx=None, device=None):
        torch = _torch()
        if sx is None:
            ns, ne, Xh = _host_f64(n_spec).reshape(-1), _host_f64(n_exti).reshape(-1), _host_f64(X)
            Xh = Xh.reshape(-1, ns.size) if ns.size else Xh
            sx = ((Xh * ns[None, :]).sum(axis=1), (Xh * ne[None, :]).sum(axis=1))
        self.sx_spec, self.sx_exti = [np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1)) for v in sx]
        self.n_spec = _dev(n_spec, torch.float64, device).reshape(-1)
        self.device = self.n_spec.device
        self.n_exti, self.DT = _dev(n_exti, torch.float64, self.device).reshape(-1), _dev(DT, torch.float64, self.device).reshape(-1)
        self.n_bins = int(self.n_spec.numel())
        self.X = _dev(X, torch.float64, self.device)
        if self.X.dim() != 2 or self.X.shape[1] != self.n_bins or self.n_exti.numel() != self.n_bins or self.DT.numel() != self.n_bins \
                or self.sx_spec.size != self.X.shape[0] or self.sx_exti.size != self.X.shape[0]:
            raise ValueError("shape mismatch: n_spec, n_exti, DT [n_bins]; X [P, n_bins]; sx_spec, sx_exti [P]")
        self.P = int(self.X.shape[0])
        self.n_chains = int(n_chains)
        self.names = list(names) if names is not None else ["x%d" % j for j in range(self.P)]


def mtrend_problem(data, state, seed, settings=MtrendSettings(), chain0=0):
    """The descriptor of a call (_hip.MtrendProblem; it refers to the tensors of data and state and to data's host arrays: keep
    them alive while it is used)."""
    st = settings
    return _hip.MtrendProblem(_hip.ptr(data.n_spec), _hip.ptr(data.n_exti), _hip.ptr(data.DT), _hip.ptr(data.X),
                              data.sx_spec.ctypes.data_as(_hip.c_vp), data.sx_exti.ctypes.data_as(_hip.c_vp), _hip.ptr(state),
                              data.n_bins, data.P, data.n_chains, int(st.m_birth), int(st.m_death), int(st.no_death), int(st.bvs), 0,
                              int(st.bvs_from), float(st.pI), float(st.slab_sd), (_hip.c_f64 * 2)(float(st.win[0]), float(st.win[1])),
                              int(chain0), int(seed) & 0xFFFFFFFFFFFFFFFF, None)


def mtrend_state(data, l0, m0, a, I_l, b, I_m):
    """A host state [C, LR_MTREND_STATE_W] holding the parameters of every chain, for mtrend_init(given=...): l0, m0 [C] or
    numbers; a, I_l, b, I_m [C, P] or [P].  Everything else 0."""
    C, P, S = data.n_chains, data.P, MTREND_STATE
    st = np.zeros((C, _hip.LR_MTREND_STATE_W))
    st[:, S["l0"]] = np.broadcast_to(np.asarray(l0, dtype=np.float64), (C,))
    st[:, S["m0"]] = np.broadcast_to(np.asarray(m0, dtype=np.float64), (C,))
    for key, v in (("a", a), ("I_l", I_l), ("b", b), ("I_m", I_m)):
        st[:, S[key]:S[key] + P] = np.broadcast_to(np.asarray(v, dtype=np.float64), (C, P))
    return st


def mtrend_init(data, seed, settings=MtrendSettings(), chain0=0, given=None, out=None):
    """The initial state of every chain (lr_mtrend_init) -> state [C, LR_MTREND_STATE_W] (elements: MTREND_STATE).  given: a
    state whose l0, m0, coefficients and indicators the caller wrote (mtrend_state): they are kept, and E, the likelihoods, the
    prior and zeroed counters added."""
    torch = _torch()
    lib = _hip.load()
    (state,) = _ade_out(out, ((max(data.n_chains, 0), _hip.LR_MTREND_STATE_W),), (torch.float64,), data.device, "(state,)")
    if given is not None:
        g = _dev(given, torch.float64, data.device)
        if tuple(g.shape) != tuple(state.shape):
            raise ValueError("given must be a [C, LR_MTREND_STATE_W] state")
        state.copy_(g)
    rc = _hip.launch_problem(lib.lr_mtrend_init, data.device, mtrend_problem(data, state, seed, settings, chain0), 0 if given is None else 1)
    _hip.check(rc, "lr_mtrend_init")
    return state


def mtrend_steps(data, state, it0, n_iters, s_freq, seed, settings=MtrendSettings(), chain0=0, rows=None, slot0=0, out=None):
    """Iterations it0 .. it0 + n_iters - 1 of every chain of `state` (updated in place; lr_mtrend_steps) -> rows [cap, C,
    LR_MTREND_ROW_W] (columns: mtrend_row_columns).  rows: an earlier call's buffer to go on writing into at slot `slot0`;
    otherwise a fresh one of exactly the rows due."""
    torch = _torch()
    lib = _hip.load()
    C = data.n_chains
    if state.dtype != torch.float64 or tuple(state.shape) != (C, _hip.LR_MTREND_STATE_W) or not state.is_contiguous() \
            or state.device != data.device:
        raise ValueError("state must be mtrend_init's [C, LR_MTREND_STATE_W] float64 tensor on the data's device")
    n = rows_due(it0, n_iters, s_freq) if int(s_freq) >= 1 and int(n_iters) >= 0 and int(it0) >= 0 else 0
    if rows is None:
        (rows,) = _ade_out(out, ((max(n, 0), C, _hip.LR_MTREND_ROW_W),), (torch.float64,), data.device, "(rows,)")
    elif rows.dtype != torch.float64 or rows.dim() != 3 or not rows.is_contiguous() or rows.device != data.device \
            or tuple(rows.shape[1:]) != (C, _hip.LR_MTREND_ROW_W):
        raise ValueError("rows must be a [cap, C, LR_MTREND_ROW_W] float64 tensor on the data's device")
    rc = _hip.launch_problem(lib.lr_mtrend_steps, data.device, mtrend_problem(data, state, seed, settings, chain0), int(it0), int(n_iters),
                             int(s_freq), _hip.ptr(rows) if rows.numel() else None, int(rows.shape[0]), int(slot0))
    _hip.check(rc, "lr_mtrend_steps")
    return rows


def mtrend_run(data, n_iter, s_freq, seed, settings=MtrendSettings(), chain0=0):
    """mtrend_init, then iterations 0 .. n_iter - 1 in one launch -> (rows, state)"""
    state = mtrend_init(data, seed, settings, chain0)
    return mtrend_steps(data, state, 0, n_iter, s_freq, seed, settings, chain0), state


def mtrend_loglik(data, l0, m0, a, I_l, b, I_m, settings=MtrendSettings()):
    """The log-likelihoods and log prior of given parameters, one set per chain (lr_mtrend_init with given = 1; arguments as
    mtrend_state's) -> (lik [C], lik_birth [C], lik_death [C], prior [C]), device tensors; lik counts a NaN as -inf"""
    torch = _torch()
    state = mtrend_init(data, 0, settings, given=mtrend_state(data, l0, m0, a, I_l, b, I_m))
    S = MTREND_STATE
    lb, ld = state[:, S["lik_b"]].clone(), state[:, S["lik_d"]].clone()
    tot = lb + ld
    return torch.where(torch.isnan(tot), torch.full_like(tot, float("-inf")), tot), lb, ld, state[:, S["prior"]].clone()


def rjmc3_problem(data, state, swaps, seed, betas, swap_every=0, settings=RjbinSettings(), chain0=0):
    """The descriptor of a call on temperature ladders (_hip.Rjmc3Problem; it refers to the tensors of data, state and swaps
    and holds the host array of the betas: keep them alive while it is used).  betas: host floats [T], betas[0] = 1."""
    import ctypes
    st = settings
    b = [float(x) for x in np.asarray(betas, dtype=float).ravel()]
    host = (ctypes.c_double * max(len(b), 1))(*b)
    prob = _hip.Rjmc3Problem(_hip.ptr(data.sp), _hip.ptr(data.ex), _hip.ptr(data.br), _hip.ptr(data.ex_dead), _hip.ptr(data.br_dead),
                             _hip.ptr(data.start_time), _hip.ptr(data.end_time), _hip.ptr(state), _hip.ptr(data.warn),
                             data.n_bins, data.R, data.chains_per_rep, int(st.model), int(st.const_rates), int(st.const_death_rate),
                             int(st.use_rate_HP), int(chain0), float(st.poisson_HP), float(st.update_fraction),
                             int(seed) & 0xFFFFFFFFFFFFFFFF, ctypes.cast(host, ctypes.c_void_p), _hip.ptr(swaps), len(b),
                             int(swap_every), None)
    prob.betas_host = host
    return prob


def rjmc3_init(data, seed, betas, settings=RjbinSettings(), chain0=0, init=None, out=None):
    """The initial state of every replica of every ladder (lr_rjmc3_init) -> (state [G T, LR_RJBIN_STATE_W], swaps [G, T - 1, 2]
    int64, zero): G = data.n_chains ladders of T = len(betas) replicas, replica w of ladder g at row g T + w, its position
    (scalar LR_RJMC3_S_POS) = w.  init: as rjbin_init's, per replica [G T, ...].  A ladder of more than 4 temperatures holds at
    most LR_RJMC3_WIDE_MAX_BINS = 256 bins (LR_ERR_SIZE)."""
    torch = _torch()
    lib = _hip.load()
    T = int(np.asarray(betas).size)
    G, C = data.n_chains, data.n_chains * T
    state, swaps = _ade_out(out, ((max(C, 0), _hip.LR_RJBIN_STATE_W), (max(G, 0), max(T - 1, 0), 2)), (torch.float64, torch.int64),
                            data.device, "(state, swaps)")
    six = [None] * 6
    if init is not None:
        L, M, tL, tM, KL, KM = init

        def pad(x, w):
            x = _host_f64(x).reshape(C, -1)
            if x.shape[1] > w:
                raise ValueError("init: at most LR_KMAX = %d rates (and one more time) per replica" % _hip.LR_KMAX)
            full = np.zeros((C, w))
            full[:, :x.shape[1]] = x
            return _dev(full, torch.float64, data.device)
        _check_host_K(KL, _hip.LR_KMAX, "K_l"), _check_host_K(KM, _hip.LR_KMAX, "K_m")
        six = [pad(L, _hip.LR_KMAX), pad(M, _hip.LR_KMAX), pad(tL, _hip.LR_KMAX + 1), pad(tM, _hip.LR_KMAX + 1),
               _dev(KL, torch.int32, data.device).reshape(-1), _dev(KM, torch.int32, data.device).reshape(-1)]
        if six[4].numel() != C or six[5].numel() != C:
            raise ValueError("init: K_l, K_m [G T]")
    prob = rjmc3_problem(data, state, swaps if swaps.numel() else None, seed, betas, 0, settings, chain0)
    rc = _hip.launch_problem(lib.lr_rjmc3_init, data.device, prob, *[_hip.ptr(t) for t in six])
    _hip.check(rc, "lr_rjmc3_init")
    return state, swaps


def rjmc3_steps(data, state, swaps, it0, n_iters, s_freq, seed, betas, swap_every, settings=RjbinSettings(), chain0=0, rows=None,
                ladder=None, slot0=0, with_ladder=True, out=None):
    """Iterations it0 .. it0 + n_iters - 1 of every replica (state and swaps updated in place; lr_rjmc3_steps), a swap round
    after every iteration with (it + 1) % swap_every == 0 (0: never) -> (rows [cap, G, LR_TRACE_W], the trace rows of the
    replica at position 0, the cold chain; ladder [cap, G, T, 4]: per position the replica there, its likA, K_l, K_m - None
    when with_ladder is False).  rows, ladder: an earlier call's buffers to go on writing into at slot `slot0`; otherwise fresh
    ones of exactly the rows due."""
    torch = _torch()
    lib = _hip.load()
    T = int(np.asarray(betas).size)
    G, C = data.n_chains, data.n_chains * T
    if state.dtype != torch.float64 or tuple(state.shape) != (C, _hip.LR_RJBIN_STATE_W) or not state.is_contiguous() \
            or state.device != data.device:
        raise ValueError("state must be rjmc3_init's [G T, LR_RJBIN_STATE_W] float64 tensor on the data's device")
    if swaps.dtype != torch.int64 or tuple(swaps.shape) != (G, max(T - 1, 0), 2) or not swaps.is_contiguous() or swaps.device != data.device:
        raise ValueError("swaps must be rjmc3_init's [G, T - 1, 2] int64 tensor on the data's device")
    n = rows_due(it0, n_iters, s_freq) if int(s_freq) >= 1 and int(n_iters) >= 0 and int(it0) >= 0 else 0
    if rows is None:
        shapes, dts = [(max(n, 0), G, _hip.LR_TRACE_W)], [torch.float64]
        if with_ladder and ladder is None:
            shapes.append((max(n, 0), G, T, _hip.LR_RJMC3_LADDER_W)), dts.append(torch.float64)
        got = _ade_out(out, tuple(shapes), tuple(dts), data.device, "(rows, ladder)")
        rows = got[0]
        ladder = got[1] if len(got) > 1 else ladder
    elif rows.dtype != torch.float64 or rows.dim() != 3 or not rows.is_contiguous() or rows.device != data.device \
            or tuple(rows.shape[1:]) != (G, _hip.LR_TRACE_W):
        raise ValueError("rows must be a [cap, G, LR_TRACE_W] float64 tensor on the data's device")
    if ladder is not None and (ladder.dtype != torch.float64 or not ladder.is_contiguous() or ladder.device != data.device
                               or tuple(ladder.shape) != (int(rows.shape[0]), G, T, _hip.LR_RJMC3_LADDER_W)):
        raise ValueError("ladder must be a [cap, G, T, 4] float64 tensor with the rows' cap on the data's device")
    prob = rjmc3_problem(data, state, swaps if swaps.numel() else None, seed, betas, swap_every, settings, chain0)
    rc = _hip.launch_problem(lib.lr_rjmc3_steps, data.device, prob, int(it0), int(n_iters), int(s_freq),
                             _hip.ptr(rows) if rows.numel() else None, _hip.ptr(ladder) if ladder is not None and ladder.numel() else None,
                             int(rows.shape[0]), int(slot0))
    _hip.check(rc, "lr_rjmc3_steps")
    return rows, ladder


EssSummary = namedtuple("EssSummary", "mean ess act se_mean stop_lag pooled_mean pooled_ess rhat n")
EssSummary.__doc__ = """lr_ess_summary's results.  mean, ess, act (in samples), se_mean float64 and stop_lag int32: [C, K] per chain and
column; pooled_mean, pooled_ess, rhat: [K]; n: rows kept per chain.  ESS and ACT are NaN, SE 0 and the stop lag 0 where a
chain's column is constant after burn-in.  Device tensors."""


def trait_weights_plan(n, n_bins, n_states):
    """The launch shape lr_trait_weights uses (lr_trait_weights_plan) -> dict(cb, tiles, passes, copies)"""
    import ctypes
    lib = _hip.load()
    out = (ctypes.c_int32 * 4)()
    _hip.check(lib.lr_trait_weights_plan(int(n), int(n_bins), int(n_states), out), "lr_trait_weights_plan")
    return dict(cb=out[0], tiles=out[1], passes=out[2], copies=out[3])


def trait_weights(ts, te, x, t0, n_bins, params, out=None):
    """The trait-weighted exposures of C states (lr_trait_weights, include/literate_hip_trait.h): params [C, 2] = (x0, kappa)
    -> (W [C, n_bins], Slog_birth [C], Slog_death [C]) with s_i = 1 / (1 + exp(-kappa (x_i - x0))), W_b = sum_i s_i e_ib and
    Slog the sum of log s_i over the births / deaths bin_unit_events counts.  out: the triple of an earlier call."""
    torch = _torch()
    lib = _hip.load()
    ts = _dev(ts, torch.float64)
    te, x = _dev(te, torch.float64, ts.device), _dev(x, torch.float64, ts.device)
    params = _dev(params, torch.float64, ts.device).reshape(-1, 2)
    n, C = ts.numel(), int(params.shape[0])
    if te.numel() != n or x.numel() != n:
        raise ValueError("ts, te and x differ in length")
    W, sb, sd = _ade_out(out, ((max(C, 0), max(int(n_bins), 0)), (max(C, 0),), (max(C, 0),)), (torch.float64,) * 3, ts.device,
                         "(W, Slog_birth, Slog_death)")
    nbytes = lib.lr_trait_weights_workspace_bytes(n, int(n_bins), C)
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_trait_weights_workspace_bytes")
    ws = alloc_workspace(nbytes, ts.device)
    prob = _hip.TraitWeightsProblem(_hip.ptr(ts), _hip.ptr(te), _hip.ptr(x), _hip.ptr(params), _hip.ptr(W), _hip.ptr(sb), _hip.ptr(sd),
                                    _hip.ptr(ws), ws.numel(), n, float(t0), int(n_bins), C, None)
    _hip.check(_hip.launch_problem(lib.lr_trait_weights, ts.device, prob), "lr_trait_weights")
    return W, sb, sd


TRAIT_SCALARS = {"x0_l": 0, "kappa_l": 1, "x0_m": 2, "kappa_m": 3, "SlogL": 4, "SlogM": 5, "proposed_l": 6, "accepted_l": 7,
                 "proposed_m": 8, "accepted_m": 9}
TRAIT_ROW_TAIL = ("x0_l", "kappa_l", "x0_m", "kappa_m", "SlogL", "SlogM", "accepted_l", "accepted_m")
TraitSettings = namedtuple("TraitSettings", "const_rates const_death_rate use_rate_HP poisson_HP update_fraction trait_every "
                           "win_x0 win_kappa x0_lo x0_hi", defaults=(0, 0, 1, 0.0, 0.75, 10, (0.5, 0.5), (0.1, 0.1), -10.0, 10.0))


class TraitData:
    """What every lr_trait_* call of one run shares: the lineages with their traits on the device, the unit-bin event counts
    as doubles, the window and the warning word."""

    def __init__(self, ts, te, x, t0, n_bins, start_time=None, end_time=None, device=None):
        torch = _torch()
        self.ts = _dev(ts, torch.float64, device)
        self.device = self.ts.device
        self.te, self.x = _dev(te, torch.float64, self.device), _dev(x, torch.float64, self.device)
        self.n, self.t0, self.n_bins = int(self.ts.numel()), float(t0), int(n_bins)
        if self.te.numel() != self.n or self.x.numel() != self.n:
            raise ValueError("ts, te and x differ in length")
        sp, ex, _ = bin_unit_events(self.ts, self.te, self.t0, self.n_bins)
        self.sp, self.ex = sp.to(torch.float64), ex.to(torch.float64)
        self.start_time = float(self.ts.min().item()) if start_time is None else float(start_time)
        self.end_time = float(self.te.max().item()) if end_time is None else float(end_time)
        self.warn = torch.zeros(1, dtype=torch.int32, device=self.device)

    def warnings(self):
        return int(self.warn.item())


def trait_problem(data, state, ws, n_chains, seed, settings=TraitSettings(), chain0=0):
    """The descriptor of a call (_hip.TraitProblem; it refers to the tensors of data, state and ws: keep them alive)."""
    st = settings
    two = _hip.c_f64 * 2
    return _hip.TraitProblem(_hip.ptr(data.ts), _hip.ptr(data.te), _hip.ptr(data.x), _hip.ptr(data.sp), _hip.ptr(data.ex),
                             _hip.ptr(state), _hip.ptr(data.warn), _hip.ptr(ws), 0 if ws is None else ws.numel(), data.n, int(chain0),
                             data.t0, data.start_time, data.end_time, float(st.poisson_HP), float(st.update_fraction),
                             two(*[float(v) for v in st.win_x0]), two(*[float(v) for v in st.win_kappa]), float(st.x0_lo),
                             float(st.x0_hi), data.n_bins, int(n_chains), int(st.const_rates), int(st.const_death_rate),
                             int(st.use_rate_HP), int(st.trait_every), int(seed) & 0xFFFFFFFFFFFFFFFF, None)


def _trait_ws(data, n_chains):
    lib = _hip.load()
    nbytes = lib.lr_trait_workspace_bytes(data.n, data.n_bins, int(n_chains))
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_trait_workspace_bytes")
    return alloc_workspace(nbytes, data.device)


def trait_init(data, n_chains, seed, settings=TraitSettings(), chain0=0, params0=None, out=None):
    """The initial state of every chain (lr_trait_init) -> state [C, LR_TRAIT_STATE_W]: lr_rjbin's rows, then the trait
    scalars (TRAIT_SCALARS) and the chain's WL, WM.  params0 [C, 4] = (x0_l, kappa_l, x0_m, kappa_m); None: zeros."""
    torch = _torch()
    lib = _hip.load()
    C = int(n_chains)
    (state,) = _ade_out(out, ((max(C, 0), _hip.LR_TRAIT_STATE_W),), (torch.float64,), data.device, "(state,)")
    p0 = None
    if params0 is not None:
        p0 = _dev(params0, torch.float64, data.device).reshape(-1)
        if p0.numel() != 4 * C:
            raise ValueError("params0 [C, 4]")
    ws = _trait_ws(data, C)
    rc = _hip.launch_problem(lib.lr_trait_init, data.device, trait_problem(data, state, ws, C, seed, settings, chain0), _hip.ptr(p0))
    _hip.check(rc, "lr_trait_init")
    return state


def trait_steps(data, state, it0, n_iters, s_freq, seed, settings=TraitSettings(), chain0=0, rows=None, slot0=0, out=None):
    """Iterations it0 .. it0 + n_iters - 1 of every chain of `state` (updated in place; lr_trait_steps) -> rows [cap, C,
    LR_TRAIT_ROW_W]: the engines' trace row, then TRAIT_ROW_TAIL.  rows / slot0 as rjbin_steps."""
    torch = _torch()
    lib = _hip.load()
    if state.dtype != torch.float64 or state.dim() != 2 or state.shape[1] != _hip.LR_TRAIT_STATE_W or not state.is_contiguous() \
            or state.device != data.device:
        raise ValueError("state must be trait_init's [C, LR_TRAIT_STATE_W] float64 tensor on the data's device")
    C = int(state.shape[0])
    n = rows_due(it0, n_iters, s_freq) if int(s_freq) >= 1 and int(n_iters) >= 0 and int(it0) >= 0 else 0
    if rows is None:
        (rows,) = _ade_out(out, ((max(n, 0), C, _hip.LR_TRAIT_ROW_W),), (torch.float64,), data.device, "(rows,)")
    elif rows.dtype != torch.float64 or rows.dim() != 3 or not rows.is_contiguous() or rows.device != data.device \
            or tuple(rows.shape[1:]) != (C, _hip.LR_TRAIT_ROW_W):
        raise ValueError("rows must be a [cap, C, LR_TRAIT_ROW_W] float64 tensor on the data's device")
    ws = _trait_ws(data, C)
    rc = _hip.launch_problem(lib.lr_trait_steps, data.device, trait_problem(data, state, ws, C, seed, settings, chain0), int(it0),
                             int(n_iters), int(s_freq), _hip.ptr(rows) if rows.numel() else None, int(rows.shape[0]), int(slot0))
    _hip.check(rc, "lr_trait_steps")
    return rows


class TraitEngine:
    """C chains of the trait-dependent RJ sampler on one data set, in the style of replicates.ReplicateEngine: the trace
    [n_trace_slots, C, LR_TRAIT_ROW_W] is resident; its first LR_TRACE_W columns have the engines' row layout."""

    def __init__(self, ts, te, x, n_chains, t0=None, n_bins=None, seed=1, settings=TraitSettings(), s_freq=1000, n_trace_slots=0,
                 chain_offset=0, device=None):
        torch = _torch()
        ts_h, te_h = _host_f64(ts), _host_f64(te)
        self.t0 = float(np.floor(ts_h.min())) if t0 is None else float(t0)
        self.n_bins = int(np.ceil(te_h.max()) - self.t0) if n_bins is None else int(n_bins)
        self.data = TraitData(ts, te, x, self.t0, self.n_bins, float(ts_h.min()), float(te_h.max()), device)
        self.device = self.data.device
        self.settings, self.seed, self.chain_offset = settings, int(seed), int(chain_offset)
        self.n_chains, self.s_freq, self.n_trace_slots = int(n_chains), int(s_freq), int(n_trace_slots)
        self.start_time, self.end_time = self.data.start_time, self.data.end_time
        self.trace = alloc_output((self.n_trace_slots, self.n_chains, _hip.LR_TRAIT_ROW_W), torch.float64, self.device, zero=True)
        self.state = None
        self.iterations = 0

    def init(self, params0=None):
        self.data.warn.zero_()
        self.state = trait_init(self.data, self.n_chains, self.seed, self.settings, self.chain_offset, params0)
        self.iterations = 0

    def samples_done(self):
        return min(self.n_trace_slots, (self.iterations + self.s_freq - 1) // self.s_freq)

    def steps(self, n):
        if self.state is None:
            raise _hip.HipLibraryError("TraitEngine.steps before init")
        n = int(n)
        due = rows_due(self.iterations, n, self.s_freq) if n > 0 else 0
        slot0 = (self.iterations + self.s_freq - 1) // self.s_freq
        if slot0 + due > self.n_trace_slots:
            raise ValueError("the trace holds %d samples; %d iterations from %d on sample up to row %d" %
                             (self.n_trace_slots, n, self.iterations, slot0 + due))
        trait_steps(self.data, self.state, self.iterations, n, self.s_freq, self.seed, self.settings, self.chain_offset,
                    rows=self.trace, slot0=slot0)
        self.iterations += n

    def set_windows(self, win_x0, win_kappa):
        """the sliding windows of the trait move, per side (tuned on the host between blocks during the burn-in)"""
        self.settings = self.settings._replace(win_x0=tuple(win_x0), win_kappa=tuple(win_kappa))

    def trait_counts(self):
        """(proposed [C, 2], accepted [C, 2]) trait moves so far, per side (a device read-back)"""
        sc = self.state[:, _hip.LR_TRAIT_ROW_SCALARS:_hip.LR_TRAIT_ROW_SCALARS + 10].cpu().numpy()
        return sc[:, [6, 8]], sc[:, [7, 9]]

    def check_status(self):
        import torch
        torch.cuda.synchronize(self.device)

    def warnings(self):
        return self.data.warnings()

    def trace_rows(self):
        """the rows written so far, on the host: [samples, C, LR_TRAIT_ROW_W]"""
        return self.trace[:self.samples_done()].cpu().numpy()

    def close(self):
        self.state = None


def ess_summary(rows, n_samples, columns, burnin=0.1, max_lag=2000):
    """Convergence summary of rows [>= n_samples, C, width] (lr_ess_summary): per chain and column Tracer's ESS, ACT,
    SE of the mean and the lag its sum stopped at, and per column the pooled mean, the pooled ESS and the split R-hat.
    Every chain drops its first int(burnin * n_samples) rows.  columns: the column indices to diagnose."""
    torch = _torch()
    lib = _hip.load()
    rows = _dev(rows, torch.float64)
    if rows.dim() != 3 or rows.shape[0] < int(n_samples):
        raise ValueError("rows must be [>= n_samples, chains, width]")
    S, C, W = int(n_samples), int(rows.shape[1]), int(rows.shape[2])
    cols = np.ascontiguousarray(np.asarray(columns, dtype=np.int32).ravel())
    K = int(cols.size)
    cptr = cols.ctypes.data_as(_hip.c_vp) if K else None
    nbytes = lib.lr_ess_summary_workspace_bytes(S, C, W, cptr, K, float(burnin), int(max_lag))
    if nbytes < 0:
        _hip.check(int(nbytes), "lr_ess_summary_workspace_bytes")
    dev = rows.device
    cs = alloc_output((K, C, 4), torch.float64, dev)
    stop = alloc_output((K, C), torch.int32, dev)
    col = alloc_output((K, 3), torch.float64, dev)
    ws = alloc_workspace(int(nbytes), dev)
    rc = _hip.launch(lib.lr_ess_summary, dev, _hip.ptr(rows), S, C, W, cptr, K, float(burnin), int(max_lag), _hip.ptr(cs),
                     _hip.ptr(stop), _hip.ptr(col), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_ess_summary")
    per = cs.permute(2, 1, 0)                                  # [4, C, K]
    return EssSummary(per[0].contiguous(), per[1].contiguous(), per[2].contiguous(), per[3].contiguous(),
                      stop.t().contiguous(), col[:, 0].contiguous(), col[:, 1].contiguous(), col[:, 2].contiguous(),
                      S - int(burnin * S))


ColSummary = namedtuple("ColSummary", "mean lo hi n")
ColSummary.__doc__ = """lr_col_summary's results.  mean, lo, hi [G, K]: the mean and the ends of the 95 % HPD of each chosen column (NaN
where the column holds a NaN); n: samples per group.  G = 1 pooled, one per chain otherwise.  Device tensors."""

CurveSummary = namedtuple("CurveSummary", "kinds values n")
CurveSummary.__doc__ = """lr_curve_summary's results.  kinds: the names of values' second axis (CURVE_KINDS[sampler]); values [G, kinds,
3 (mean, HPD low, HPD high), n_bins] (device); n: samples per group.  G = 1 pooled, one per chain otherwise."""

CURVE_KINDS = {1: ("birth", "death", "net", "niche", "nicheFrac"), 2: ("birth", "death", "net")}


def summary_geometry(n_samples, n_chains, burnin, pooled):
    """(rows dropped per chain, samples per group n, samples inside the HPD window) of lr_col_summary /
    lr_curve_summary: int(burnin * S) rows dropped, n_in = round-half-even(0.95 n).  Host arithmetic only."""
    S = int(n_samples)
    burn = int(burnin * S)
    n = (S - burn) * (int(n_chains) if pooled else 1)
    return burn, n, int(round(0.95 * n))


def _summary_cap(workspace_bytes, dev, torch):
    # by default at most a quarter of the free device memory (and never less than 1 GiB), as ops.rtt_summary
    if workspace_bytes is not None:
        return int(workspace_bytes)
    return max(1 << 30, torch.cuda.mem_get_info(dev)[0] // 4)


def col_summary(rows, n_samples, columns, burnin=0.2, pooled=True, workspace_bytes=None):
    """Mean and 95 % HPD (calcHPD) of chosen columns of rows [>= n_samples, C, width] (lr_col_summary: what plotDD.py /
    logAverager.py take of a log's parameter columns) -> ColSummary.  Every chain drops its first int(burnin * n_samples)
    rows; pooled: the kept rows of all chains as one sample, chain after chain; else one summary per chain.
    workspace_bytes: cap the workspace (the call then works through the columns in chunks; the same results)."""
    torch = _torch()
    lib = _hip.load()
    rows = _dev(rows, torch.float64)
    if rows.dim() != 3 or rows.shape[0] < int(n_samples):
        raise ValueError("rows must be [>= n_samples, chains, width]")
    S, C, W = int(n_samples), int(rows.shape[1]), int(rows.shape[2])
    cols = np.ascontiguousarray(np.asarray(columns, dtype=np.int32).ravel())
    K = int(cols.size)
    cptr = cols.ctypes.data_as(_hip.c_vp) if K else None
    full = lib.lr_col_summary_workspace_bytes(S, C, W, cptr, K, float(burnin), int(bool(pooled)), 0)
    if full < 0:
        _hip.check(int(full), "lr_col_summary_workspace_bytes")
    dev = rows.device
    G = 1 if pooled else C
    out = alloc_output((G, K, 3), torch.float64, dev)
    ws = alloc_workspace(max(1, min(int(full), _summary_cap(workspace_bytes, dev, torch))), dev)
    rc = _hip.launch(lib.lr_col_summary, dev, _hip.ptr(rows), S, C, W, cptr, K, float(burnin), int(bool(pooled)),
                     _hip.ptr(out), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_col_summary")
    return ColSummary(out[:, :, 0].contiguous(), out[:, :, 1].contiguous(), out[:, :, 2].contiguous(),
                      summary_geometry(S, C, burnin, pooled)[1])


def curve_summary(rows, n_samples, sampler, aux, m_birth, m_death, arg_col=4, burnin=0.2, pooled=True,
                  workspace_bytes=None):
    """Mean and 95 % HPD per time bin of the curves the parameter vectors rows[..., arg_col:arg_col + npar] imply
    (lr_curve_summary: what plotDD.py takes of a log's l_i, m_i and niche_i columns, derived on the device instead of read
    from the log) -> CurveSummary.  sampler 1: DDRate (aux = DT, m_birth / m_death as dd_rates; birth, death, net, niche,
    nicheFrac); sampler 2: trend_rate (aux = TREND, m_birth / m_death = const_birth / const_death; birth, death, net).
    Burn-in, pooling and workspace_bytes as col_summary (chunks of bins)."""
    torch = _torch()
    lib = _hip.load()
    rows = _dev(rows, torch.float64)
    if rows.dim() != 3 or rows.shape[0] < int(n_samples):
        raise ValueError("rows must be [>= n_samples, chains, width]")
    aux = _dev(aux, torch.float64, rows.device).reshape(-1)
    S, C, W, nb = int(n_samples), int(rows.shape[1]), int(rows.shape[2]), int(aux.numel())
    sampler = int(sampler)
    full = lib.lr_curve_summary_workspace_bytes(S, C, W, int(arg_col), sampler, nb, float(burnin), int(bool(pooled)), 0)
    if full < 0:
        _hip.check(int(full), "lr_curve_summary_workspace_bytes")
    dev = rows.device
    G = 1 if pooled else C
    kinds = CURVE_KINDS[sampler]
    out = alloc_output((G, len(kinds), 3, nb), torch.float64, dev)
    ws = alloc_workspace(max(1, min(int(full), _summary_cap(workspace_bytes, dev, torch))), dev)
    rc = _hip.launch(lib.lr_curve_summary, dev, _hip.ptr(rows), S, C, W, int(arg_col), sampler, int(m_birth), int(m_death),
                     _hip.ptr(aux), nb, float(burnin), int(bool(pooled)), _hip.ptr(out), _hip.ptr(ws), ws.numel())
    _hip.check(rc, "lr_curve_summary")
    return CurveSummary(kinds, out, summary_geometry(S, C, burnin, pooled)[1])


def debug_draws(seed, chain, it, purpose, idx, kind, shape):
    """Device RNG probe: kind 0 u_a, 1 u_b, 2 normal, 3 gamma(shape) at (it, purpose, idx)."""
    torch = _torch()
    lib = _hip.load()
    it = _dev(it, torch.int64)
    purpose, idx, kind = _dev(purpose, torch.int32), _dev(idx, torch.int32), _dev(kind, torch.int32)
    shape = _dev(shape, torch.float64)
    out = alloc_output(it.numel(), torch.float64, it.device)
    rc = _hip.launch(lib.lr_debug_draws, it.device, int(seed), int(chain), _hip.ptr(it), _hip.ptr(purpose), _hip.ptr(idx), _hip.ptr(kind),
                            _hip.ptr(shape), it.numel(), _hip.ptr(out))
    _hip.check(rc, "lr_debug_draws")
    return out
