"""Numpy restatement of lr_ade_classes and lr_ade_profile, written from their definition (include/literate_hip_ade.h): the
lineages per (birth bin, age at death) class, and per (draw, shape) the multiplier c that maximises

    l(c) = sum_{dead[jb][a] > 0} dead[jb][a] (-c H[jb][a] + log(-expm1(-c (H[jb][a + 1] - H[jb][a])))) - c sum_jb cens[jb] H[jb][A - jb]

with H[jb][m] = sum_{j < m} mu[jb + j] w_k[j], w_k[0] = 1, w_k[j] = j^k expm1(k log1p(1 / j)).  H is formed as the header writes
it, one cumulative sum per birth bin; c^ by BISECTION on the sign of the score in log c, to 1e-13 (a search on the value
would locate it to 1e-8 only).  profile_loop is the definition once more, class by class in Python floats, and `Restated`
is the three methods literate_amd.ade.fit_rates takes in place of the device."""
import math

import numpy as np

BISECT_TOL = 1e-13


def classes(ts, te, t0, n_bins):
    """-> (dead [A, A], cens [A], totals [2] = used, unused), int64"""
    ts, te = np.asarray(ts, dtype=np.float64), np.asarray(te, dtype=np.float64)
    A = int(n_bins)
    t_end = np.float64(t0) + np.float64(A)
    with np.errstate(invalid="ignore"):
        x = ts - np.float64(t0)
        used = (x >= 0.0) & (x < float(A)) & (te > ts)
        jb = np.floor(np.where(used, x, 0.0)).astype(np.int64)
        is_dead = used & (te <= t_end)
        je = np.minimum(np.floor(np.where(is_dead, te - np.float64(t0), 0.0)).astype(np.int64), A - 1)
    dead = np.zeros((A, A), dtype=np.int64)
    cens = np.zeros(A, dtype=np.int64)
    np.add.at(dead, (jb[is_dead], je[is_dead] - jb[is_dead]), 1)
    np.add.at(cens, jb[used & ~is_dead], 1)
    return dead, cens, np.array([used.sum(), len(ts) - used.sum()], dtype=np.int64)


def weights(k, A):
    """w_k[0 .. A)"""
    j = np.arange(1, A, dtype=np.float64)
    return np.concatenate([[1.0], j ** np.float64(k) * np.expm1(np.float64(k) * np.log1p(1.0 / j))])


def class_list(dead):
    """(jb, a, n) of the cells with jb + a < A and a count > 0"""
    dead = np.asarray(dead)
    A = dead.shape[0]
    jb, a = np.nonzero((dead > 0) & (np.add.outer(np.arange(A), np.arange(A)) < A))
    return jb, a, dead[jb, a].astype(np.float64)


def flags(dead, mu_bins):
    """draws with a rate that is not finite or < 0, or zero in a bin that holds an observed death"""
    mu = np.asarray(mu_bins, dtype=np.float64)
    jb, a, _ = class_list(dead)
    death_bin = np.zeros(mu.shape[1], dtype=bool)
    death_bin[jb + a] = True
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(mu).all(axis=1) | (np.nan_to_num(mu, nan=-1.0) < 0).any(axis=1) | ((mu == 0.0) & death_bin[None, :]).any(axis=1)


def tables(dead, cens, mu, k):
    """one draw, one shape -> (n, H at the class, its step to the next age, the censored's sum of cens H[jb][A - jb])"""
    A = len(mu)
    w = weights(k, A)
    H = np.zeros((A, A + 1))
    for jb in range(A):
        H[jb, 1:A - jb + 1] = np.cumsum(mu[jb:] * w[:A - jb])
    jb, a, n = class_list(dead)
    h_end = H[np.arange(A), A - np.arange(A)]
    return n, H[jb, a], H[jb, a + 1] - H[jb, a], float(np.sum(np.asarray(cens, dtype=np.float64) * h_end))


def loglik(c, n, h, d, ce):
    """l(c) and sum n |class term|"""
    with np.errstate(divide="ignore"):
        term = -c * h + np.log(-np.expm1(-c * d))
    return float(np.sum(n * term) - c * ce), float(np.sum(n * np.abs(term)))


def score(c, n, h, d, ce):
    """dl/dc"""
    with np.errstate(over="ignore"):
        return float(np.sum(n * (d / np.expm1(c * d) - h)) - ce)


def profile_one(dead, cens, mu, k):
    """-> (l(c^), c^, sum n |class term| at c^)"""
    n, h, d, ce = tables(dead, cens, np.asarray(mu, dtype=np.float64), k)
    if len(n) == 0:
        return 0.0, 0.0, 0.0
    coef = float(np.sum(n * h) + ce)
    if coef == 0.0:
        return 0.0, math.inf, 0.0
    u = math.log(np.sum(n) / (coef + 0.5 * np.sum(n * d)))
    lo = hi = u
    while score(math.exp(lo), n, h, d, ce) <= 0.0:
        lo -= 1.0
    while score(math.exp(hi), n, h, d, ce) >= 0.0:
        hi += 1.0
    while hi - lo > BISECT_TOL:
        mid = 0.5 * (lo + hi)
        if score(math.exp(mid), n, h, d, ce) > 0.0:
            lo = mid
        else:
            hi = mid
    c = math.exp(0.5 * (lo + hi))
    ll, mag = loglik(c, n, h, d, ce)
    return ll, c, mag


def profile(dead, cens, mu_bins, shapes, with_scale=False):
    """-> (ll [S, G], c [S, G], flag [S] int32) - and with_scale the sums of n |class term| [S, G] the tolerance is taken of"""
    mu = np.asarray(mu_bins, dtype=np.float64)
    shapes = np.asarray(shapes, dtype=np.float64).reshape(-1)
    S, G = mu.shape[0], len(shapes)
    bad = flags(dead, mu)
    ll, c, mag = (np.full((S, G), np.nan) for _ in range(3))
    for s in range(S):
        if bad[s]:
            continue
        for g in range(G):
            if np.isfinite(shapes[g]) and shapes[g] > 0.0:
                ll[s, g], c[s, g], mag[s, g] = profile_one(dead, cens, mu[s], shapes[g])
    out = (ll, c, bad.astype(np.int32))
    return out + (mag,) if with_scale else out


def profile_loop(dead, cens, mu, k):
    """one draw, one shape, the definition class by class in Python floats -> (l(c^), c^)"""
    A = len(mu)
    mu = [float(v) for v in mu]
    k = float(k)
    w = [1.0] + [j ** k * math.expm1(k * math.log1p(1.0 / j)) for j in range(1, A)]
    H = []
    for jb in range(A):
        row = [0.0]
        for j in range(A - jb):
            row.append(row[-1] + mu[jb + j] * w[j])
        H.append(row)
    cls = [(int(dead[jb][a]), H[jb][a], H[jb][a + 1] - H[jb][a]) for jb in range(A) for a in range(A - jb) if dead[jb][a] > 0]
    ce = sum(int(cens[jb]) * H[jb][A - jb] for jb in range(A))
    if not cls:
        return 0.0, 0.0
    if sum(n * h for n, h, _ in cls) + ce == 0.0:
        return 0.0, math.inf

    def sc(c):
        tot = -ce
        for n, h, d in cls:
            x = c * d
            tot += n * ((d / math.expm1(x) if x < 700.0 else 0.0) - h)
        return tot
    lo, hi = -1.0, 1.0
    while sc(math.exp(lo)) <= 0.0:
        lo -= 1.0
    while sc(math.exp(hi)) >= 0.0:
        hi += 1.0
    while hi - lo > BISECT_TOL:
        mid = 0.5 * (lo + hi)
        if sc(math.exp(mid)) > 0.0:
            lo = mid
        else:
            hi = mid
    c = math.exp(0.5 * (lo + hi))
    return sum(n * (-c * h + math.log(-math.expm1(-c * d))) for n, h, d in cls) - c * ce, c


class Restated:
    """literate_amd.ade.fit_rates' `profile`: the restatement in the device's place (the column summary by
    tests/helpers/summary_ref.py)"""

    def classes(self, ts, te, t0, n_bins):
        return classes(ts, te, t0, n_bins)

    def profile(self, dead, cens, mu_bins, shapes):
        return profile(dead, cens, mu_bins, shapes)

    def summary(self, vals):
        from helpers import summary_ref
        return summary_ref.triples(vals)


def simulate(rng, n_bins, births_per_bin, mu, k, c):
    """the model itself at year resolution: births_per_bin lineages born at the start of every bin, a lineage of age a (in
    bins) survives bin b with probability exp(-c mu[b] w_k[a]); -> (ts, te) with te = death bin + 0.5, or far beyond the
    window for a survivor (t0 = 0)"""
    w = weights(k, n_bins)
    ts, te = [], []
    for jb in range(n_bins):
        p = -np.expm1(-c * np.asarray(mu[jb:]) * w[:n_bins - jb])             # dies in bin jb + a, given alive at its start
        u = rng.random((births_per_bin, n_bins - jb))
        dies = u < p[None, :]
        first = np.where(dies.any(axis=1), dies.argmax(axis=1), -1)
        ts.extend([float(jb)] * births_per_bin)
        te.extend([jb + a + 0.5 if a >= 0 else n_bins + 100.0 for a in first])
    return np.array(ts), np.array(te)
