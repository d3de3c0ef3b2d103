"""Numpy restatement of lr_shift_prior (include/literate_hip.h): the Monte Carlo prior on the times of rate shifts of
plotRJforward.v3.py get_prior_shift (:58-89), replicate by replicate on the draws the device uses - Philox4x32-10
(oracle/philox.py) with key (seed's low word, seed's high word) and counter (replicate, P_SHIFT_PRIOR, idx).  Every
numpy operation rounds on its own, which is what the kernel's __dmul_rn / __dadd_rn / __ddiv_rn restate; lambda is taken
with libm's log here and with lr_log there (a last-place difference moves a K only where a uniform lies within an ulp of
a step of the CDF).  The accept rule and the histogram are the script's own expressions."""
from collections import namedtuple

import numpy as np

from oracle.philox import MASK, philox4x32_10_np

P_SHIFT_PRIOR = 40      # (must match literate_amd/csrc/lr_prior.hip)
KCAP = 64               # LR_SHIFT_PRIOR_KCAP

ShiftPriorRef = namedtuple("ShiftPriorRef", "totals shift_hist k_drawn k_accepted K accept")


def _to_double(hi, lo):
    return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def pair(it, idx, seed):
    """(u_a, u_b) of the replicates `it` (uint64 array) at index idx"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10_np(it & np.uint64(MASK), it >> np.uint64(32), P_SHIFT_PRIOR, idx, seed & MASK, seed >> 32)
    return _to_double(w[0], w[1]), _to_double(w[2], w[3])


def replicates(rep0, n_reps):
    return np.uint64(rep0) + np.arange(n_reps, dtype=np.uint64)


def draw_k(it, seed, poi_lambda=None):
    """(K, capped) of the replicates `it`: zero-truncated Poisson(lambda) by inversion, lambda ~ Gamma(2, 1) as the sum of
    two exponentials unless a fixed rate is given"""
    n = len(it)
    if poi_lambda is not None and poi_lambda > 0:
        lam = np.full(n, float(poi_lambda))
        p0 = np.full(n, np.exp(-float(poi_lambda)))
    else:
        ua, ub = pair(it, 0, seed)
        p0 = (1.0 - ua) * (1.0 - ub)
        with np.errstate(divide="ignore"):
            lam = -np.log(p0)
    u = pair(it, 1, seed)[0]
    t = p0 + u * (1.0 - p0)
    k = np.zeros(n, dtype=np.int64)
    p, cum = p0.copy(), p0.copy()
    live = np.ones(n, dtype=bool)
    while live.any():
        k[live] += 1
        p[live] = (p[live] * lam[live]) / k[live].astype(np.float64)
        cum[live] = cum[live] + p[live]
        live &= (cum <= t) & (k < KCAP)
    return k, cum <= t


def shift_times(it, K, seed, a, b):
    """[n, max(K) - 1] shift times, NaN beyond a replicate's K - 1"""
    lo, w = a - 1.0, (b + 1.0) - (a - 1.0)
    m = int(K.max()) - 1
    X = np.full((len(it), max(m, 0)), np.nan)
    for q in range((m + 1) // 2):
        rows = np.nonzero(K - 1 > 2 * q)[0]
        ua, ub = pair(it[rows], 2 + q, seed)
        X[rows, 2 * q] = lo + w * ua
        if 2 * q + 1 < m:
            both = K[rows] - 1 > 2 * q + 1
            X[rows[both], 2 * q + 1] = lo + w * ub[both]
    return X


def shift_prior_ref(a, b, rep0, n_reps, seed, poi_lambda=None):
    """lr_shift_prior(a, b, rep0, n_reps, seed, poi_lambda) -> ShiftPriorRef: the four outputs, and K and the accept flag
    per replicate"""
    a, b = float(a), float(b)
    it = replicates(rep0, n_reps)
    K, capped = draw_k(it, seed, poi_lambda)
    X = shift_times(it, K, seed, a, b)
    # time_frames = np.sort([t_start, t_end] + shift_times); rejected if min(np.diff(time_frames)) < 1 (NaN sorts last)
    frames = np.sort(np.concatenate([np.full((n_reps, 1), a), np.full((n_reps, 1), b), X], axis=1), axis=1)
    d = np.diff(frames, axis=1)
    accept = ~(np.where(np.isnan(d), np.inf, d).min(axis=1) < 1.0)
    edges = np.arange(a, b)
    kept = X[accept]
    kept = kept[~np.isnan(kept)]
    hist = np.histogram(kept, bins=edges)[0].astype(np.int64)
    totals = np.array([accept.sum(), hist.sum(), capped.sum(), (K[accept] - 1).sum()], dtype=np.int64)
    k_drawn = np.bincount(K - 1, minlength=KCAP).astype(np.int64)
    k_accepted = np.bincount(K[accept] - 1, minlength=KCAP).astype(np.int64)
    return ShiftPriorRef(totals, hist, k_drawn, k_accepted, K, accept)
