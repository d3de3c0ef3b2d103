"""Numpy restatement of lr_ppc_age, written from its definition (include/literate_hip_age.h): posterior predictive deaths by
age.  Every product, sum, difference and quotient is one numpy float64 operation, so the doubles are the device's - up to
the logarithm: the device's lr_log is within 1.2 ulp of log (tests/helpers/math_edges.py), so E = -log(1 - u) may differ by
about 2 ulp, and with it the target.  Only a pair whose target lies within a few ulp of a table step, or whose lifespan
lies within a few ulp of a class edge, can then land elsewhere: `fragile` lists the pairs whose outcome changes when E is
multiplied by 1 +- 2^-50 (4.5 ulp), and the case table holds none.

    ppc_age      vectorised over the lineages, per draw: np.cumsum and np.searchsorted(C[1:], target, side="right")
    ppc_age_loop the same definition as a scalar Python loop that walks the bins one by one (an independent cross-check)
    summary      the tables of literate_amd.ppc_age from (obs, rep): per-class deaths and hazard, the overall statistics,
                 the means summed in lr_col_summary's own order (device_mean)"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import philox  # noqa: E402

P_PPC_AGE = 41
MASK = 0xFFFFFFFF


def lineage_terms(ts, te, t0, n_bins):
    """the data's side: used [n], x, jb, fs, dead, observed class, censor class"""
    ts, te = np.asarray(ts, dtype=np.float64), np.asarray(te, dtype=np.float64)
    A = int(n_bins)
    t_end = np.float64(t0) + np.float64(A)
    with np.errstate(invalid="ignore"):
        x = ts - np.float64(t0)
        used = (x >= 0.0) & (x < float(A)) & (te > ts)
        xs = np.where(used, x, 0.0)
        jb = np.floor(xs).astype(np.int64)
        fs = xs - np.floor(xs)
        dead = used & (te <= t_end)
        life = np.where(used, np.floor(np.where(dead, te, t_end) - ts), 0.0)
        cens = np.where(used, np.floor(t_end - ts), 0.0)
    oc = np.minimum(life, A - 1).astype(np.int64)
    cc = np.minimum(cens, A - 1).astype(np.int64)
    return used, xs, jb, fs, dead, oc, cc


def flagged(mu):
    """draws with a rate that is not finite or negative, or a total that is not finite"""
    mu = np.asarray(mu, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        total = np.cumsum(mu, axis=1)[:, -1]
    return ~np.isfinite(mu).all(axis=1) | (np.nan_to_num(mu, nan=-1.0) < 0).any(axis=1) | ~np.isfinite(total)


def uniforms(n, s, seed):
    """u_a of the pairs (i, s), i = 0 .. n - 1"""
    return philox.uniform_a_np(np.arange(n, dtype=np.uint64), P_PPC_AGE, s, seed & MASK, (seed >> 32) & MASK)


def ppc_age(ts, te, t0, mu_bins, seed, e_scale=1.0):
    """-> dict(obs [2, A], rep [S, 2, A], totals [4], dead [n, S] bool, cls [n, S] - both -1 / False where the lineage is
    unused or the draw flagged).  e_scale multiplies E (for `fragile`)."""
    mu = np.asarray(mu_bins, dtype=np.float64)
    S, A = mu.shape
    n = len(ts)
    used, x, jb, fs, dead_obs, oc, cc = lineage_terms(ts, te, t0, A)
    obs = np.zeros((2, A), dtype=np.int64)
    np.add.at(obs[0], oc[used & dead_obs], 1)
    np.add.at(obs[1], oc[used & ~dead_obs], 1)
    bad = flagged(mu)
    rep = np.zeros((S, 2, A), dtype=np.int64)
    dead = np.zeros((n, S), dtype=bool)
    cls = np.full((n, S), -1, dtype=np.int64)
    for s in range(S):
        if bad[s]:
            rep[s] = -1
            continue
        m = mu[s]
        C = np.concatenate([[0.0], np.cumsum(m)])
        E = -np.log(1.0 - uniforms(n, s, seed)) * np.float64(e_scale)
        target = (C[jb] + m[jb] * fs) + E
        b = np.maximum(np.searchsorted(C[1:], target, side="right"), jb)
        dies = b < A
        bb = np.minimum(b, A - 1)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t_in = (target - C[bb]) / m[bb]
            life = (bb.astype(np.float64) + t_in) - x
        k = np.where(dies, np.minimum(np.maximum(np.floor(np.where(dies, life, 0.0)), 0.0), A - 1).astype(np.int64), cc)
        np.add.at(rep[s, 0], k[used & dies], 1)
        np.add.at(rep[s, 1], k[used & ~dies], 1)
        dead[:, s] = used & dies
        cls[:, s] = np.where(used, k, -1)
    totals = np.array([used.sum(), n - used.sum(), S - bad.sum(), bad.sum()], dtype=np.int64)
    return dict(obs=obs, rep=rep, totals=totals, dead=dead, cls=cls)


def ppc_age_loop(ts, te, t0, mu_bins, seed):
    """the definition once more, pair by pair and bin by bin in Python floats -> (obs, rep, totals)"""
    mu = np.asarray(mu_bins, dtype=np.float64)
    S, A = mu.shape
    n = len(ts)
    t0 = float(t0)
    t_end = t0 + float(A)
    stream = philox.Stream(seed & MASK, (seed >> 32) & MASK)
    obs = np.zeros((2, A), dtype=np.int64)
    rep = np.zeros((S, 2, A), dtype=np.int64)
    lin = []
    unused = 0
    for i in range(n):
        s_, e_ = float(ts[i]), float(te[i])
        x = s_ - t0
        if not (0.0 <= x < A and e_ > s_):
            unused += 1
            continue
        jb = int(math.floor(x))
        dead = e_ <= t_end
        obs[0 if dead else 1][min(int(math.floor((e_ if dead else t_end) - s_)), A - 1)] += 1
        lin.append((i, x, jb, x - jb, min(int(math.floor(t_end - s_)), A - 1)))
    n_bad = 0
    for s in range(S):
        m = [float(v) for v in mu[s]]
        C = [0.0]
        for v in m:
            C.append(C[-1] + v)
        if any(not math.isfinite(v) or v < 0.0 for v in m) or not math.isfinite(C[-1]):
            rep[s] = -1
            n_bad += 1
            continue
        for i, x, jb, fs, cc in lin:
            u = stream.pair(i, P_PPC_AGE, s)[0]
            target = (C[jb] + m[jb] * fs) + -math.log(1.0 - u)
            b = jb
            while b < A and not (C[b + 1] > target):
                b += 1
            if b == A:
                rep[s, 1, cc] += 1
            else:
                life = (float(b) + (target - C[b]) / m[b]) - x
                rep[s, 0, min(max(int(math.floor(life)), 0), A - 1)] += 1
    return obs, rep, np.array([len(lin), unused, S - n_bad, n_bad], dtype=np.int64)


def fragile(ts, te, t0, mu_bins, seed, base=None):
    """the pairs (i, s) whose outcome (dead, class) changes when E is multiplied by 1 - 2^-50 or 1 + 2^-50"""
    base = base or ppc_age(ts, te, t0, mu_bins, seed)
    out = np.zeros(base["dead"].shape, dtype=bool)
    for f in (1.0 - 2.0 ** -50, 1.0 + 2.0 ** -50):
        other = ppc_age(ts, te, t0, mu_bins, seed, e_scale=f)
        out |= (other["dead"] != base["dead"]) | (other["cls"] != base["cls"])
    return np.argwhere(out)


# ------------------------------------------------------------------------------------------------
# the summary tables, from their definition
# ------------------------------------------------------------------------------------------------
def _values(c):
    """c [2, A] integers -> (deaths [A], at_risk [A], hazard [A], [total deaths, mean class at death, median survival class])"""
    A = c.shape[1]
    d = [int(v) for v in c[0]]
    tot = [int(c[0, a] + c[1, a]) for a in range(A)]
    risk = [sum(tot[a:]) for a in range(A)]
    haz = [np.float64(d[a]) / np.float64(risk[a]) if risk[a] > 0 else np.nan for a in range(A)]
    nd = sum(d)
    mean_class = np.float64(sum(a * d[a] for a in range(A))) / np.float64(nd) if nd > 0 else np.nan
    surv, median = np.float64(1.0), float(A)
    for a in range(A):
        surv = surv * (np.float64(1.0) - haz[a])
        if surv <= 0.5:
            median = float(a)
            break
    return np.array(d, float), np.array(risk, np.int64), np.array(haz, float), np.array([float(nd), mean_class, median])


def device_mean(col):
    """The mean of a column as lr_col_summary forms it (csrc/lr_curves.hip, lr_cv_hpd_kernel): on the SORTED values thread t of
    256 adds d[t], d[t + 256], ... in that order, the 256 partial sums are then added pairwise (s[t] += s[t + w] for
    w = 128, 64, ..., 1), and the sum is divided by n.  A sum of non-integers depends on its order in the last bits; in this
    order the restatement's mean is the device's, so the files compare with ==."""
    d = np.sort(np.asarray(col, dtype=np.float64))
    part = np.zeros(256)
    for e in range(0, len(d), 256):
        c = d[e:e + 256]
        part[:len(c)] = part[:len(c)] + c
    w = 128
    while w > 0:
        part[:w] = part[:w] + part[w:2 * w]
        w //= 2
    return part[0] / np.float64(len(d))


def col_stats(vals, o):
    """vals [n, K], o [K] -> [K, 5] = (obs, mean, hpd_low, hpd_high, p_ge): the HPD by tests/helpers/summary_ref.py, the mean by
    device_mean; a column that holds a NaN is NaN in mean and HPD"""
    from helpers import summary_ref
    vals, o = np.asarray(vals, dtype=np.float64), np.asarray(o, dtype=np.float64)
    bad = np.isnan(vals).any(axis=0)
    clean = np.where(np.isnan(vals), 0.0, vals)
    st = np.empty((len(o), 5))
    st[:, 0] = o
    st[:, 1:4] = summary_ref.triples(clean)
    st[:, 1] = [device_mean(clean[:, k]) for k in range(vals.shape[1])]
    st[bad, 1:4] = np.nan
    with np.errstate(invalid="ignore"):
        st[:, 4] = (vals >= o[None, :]).sum(axis=0) / float(len(vals))
    return st


def summary(obs, rep):
    """(obs [2, A], rep [S, 2, A]) -> dict(kept, at_risk_obs [A], deaths [A, 5], hazard [A, 5], overall [3, 5], coverage_deaths,
    coverage_hazard, hazard_classes_extreme): every statistic as (obs, mean, hpd_low, hpd_high, p_ge) over the unflagged
    draws (col_stats); mean, HPD and p_ge NaN where the statistic is undefined in the data or in a kept draw"""
    obs, rep = np.asarray(obs, dtype=np.int64), np.asarray(rep, dtype=np.int64)
    A = obs.shape[1]
    kept = rep[:, 0, 0] >= 0
    o = np.concatenate([_values(obs)[k] for k in (0, 2, 3)])
    rows = np.array([np.concatenate([v[k] for k in (0, 2, 3)]) for v in (_values(r) for r in rep[kept])])
    undefined = np.isnan(o) | np.isnan(rows).any(axis=0)
    st = col_stats(rows, o)
    st[undefined, 1:] = np.nan

    def coverage(t):
        r = np.isfinite(t[:, 1])
        return float(np.mean((t[r, 0] >= t[r, 2]) & (t[r, 0] <= t[r, 3]))) if r.any() else float("nan")

    deaths, hazard, overall = st[:A], st[A:2 * A], st[2 * A:]
    with np.errstate(invalid="ignore"):
        extreme = int(np.sum((hazard[:, 4] < 0.025) | (hazard[:, 4] > 0.975)))
    return dict(kept=kept, at_risk_obs=_values(obs)[1], deaths=deaths, hazard=hazard, overall=overall,
                coverage_deaths=coverage(deaths), coverage_hazard=coverage(hazard), hazard_classes_extreme=extreme)
