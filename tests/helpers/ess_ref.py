"""Numpy restatement of lr_ess_summary (include/literate_hip.h): per chain and column Tracer's effective sample size (BEAST
TraceCorrelation), per column the pooled mean and ESS and the split R-hat (Gelman et al., BDA3 11.4).

Written straight from the definitions, one series at a time.  The arithmetic is generic: given arrays of
fractions.Fraction (dtype=object) every quantity but the square roots comes out exact."""
import math

import numpy as np

NAN = float("nan")


def seq_mean(x):
    """A sequence of equal values has that value as its mean; otherwise sum / n."""
    return x[0] if np.all(x == x[0]) else x.sum() / len(x)


def autocov(d, t):
    n = len(d)
    return (d[:n - t] * d[t:]).sum() / (n - t)


def pair_bound(d, t):
    """How far from zero the rounding of g_{t-1} + g_t can reach: n 2^-52 (sum|d_j d_{j+t-1}| / (n-t+1) + sum|d_j d_{j+t}| / (n-t))"""
    n = len(d)
    a = np.abs(d)
    return n * 2.0 ** -52 * ((a[:n - t + 1] * a[t - 1:]).sum() / (n - t + 1) + (a[:n - t] * a[t:]).sum() / (n - t))


def series(x, max_lag=2000, stop_at=None):
    """One kept series -> dict(mean, ess, act, se_mean, stop_lag, V, g0, d).  stop_at: end the sum at this lag instead
    of where the pair rule ends it (an even lag below L, or L)."""
    n = len(x)
    m = seq_mean(x)
    d = x - m
    L = min(n - 1, max_lag)
    g0 = autocov(d, 0)
    if g0 == 0:
        return dict(mean=m, ess=NAN, act=NAN, se_mean=0.0, se2=0, stop_lag=0, V=g0, g0=g0, d=d)
    V, stop, t = g0, L, 2
    while t < L:
        p = autocov(d, t - 1) + autocov(d, t)
        go = (t < stop_at) if stop_at is not None else p > 0
        if not go:
            stop = t
            break
        V += 2 * p
        t += 2
    act = V / g0
    return dict(mean=m, ess=n / act, act=act, se_mean=math.sqrt(V / n), se2=V / n, stop_lag=stop, V=V, g0=g0, d=d)


def halves(x):
    """The two R-hat sequences of one chain: (mean, variance with divisor h - 1) of rows [0, h) and [n - h, n)."""
    n = len(x)
    h = n // 2
    out = []
    for q in (x[:h], x[n - h:]):
        mu = seq_mean(q)
        out.append((mu, ((q - mu) * (q - mu)).sum() / (h - 1)))
    return out, h


def rhat_of(chains):
    """split R-hat of kept series [C][n] -> (rhat, rhat^2 (exact for fractions), W)"""
    seqs = []
    h = None
    for x in chains:
        hs, h = halves(x)
        seqs += hs
    M = len(seqs)
    mu = sum(s[0] for s in seqs) / M
    B = h * sum((s[0] - mu) * (s[0] - mu) for s in seqs) / (M - 1)
    W = sum(s[1] for s in seqs) / M
    if W == 0:
        return NAN, NAN, W
    r2 = ((h - 1) * W / h + B / h) / W
    return math.sqrt(r2), r2, W


def kept(rows, n_samples, columns, burnin):
    """rows [>= n_samples, C, width] -> kept series [C, K, n] (float64) and the burn-in"""
    rows = np.asarray(rows, dtype=np.float64)
    burn = int(burnin * n_samples)
    return np.ascontiguousarray(rows[burn:n_samples][:, :, list(columns)].transpose(1, 2, 0)), burn


def summary(rows, n_samples, columns, burnin=0.1, max_lag=2000, stop_at=None, chains=None):
    """The whole call -> dict of [C, K] arrays (mean, ess, act, se_mean, stop_lag) and [K] arrays (pooled_mean, pooled_ess,
    rhat), n.  stop_at: {(c, k): lag} forced stop lags; chains: only these chains' per-chain values (the pooled values
    and R-hat always use every chain)."""
    X, _ = kept(rows, n_samples, columns, burnin)
    C, K, n = X.shape
    out = {key: np.full((C, K), NAN) for key in ("mean", "ess", "act", "se_mean")}
    out["stop_lag"] = np.full((C, K), -1, dtype=np.int64)
    want = range(C) if chains is None else chains
    for c in want:
        for k in range(K):
            r = series(X[c, k], max_lag, None if stop_at is None else stop_at.get((c, k)))
            for key in ("mean", "ess", "act", "se_mean", "stop_lag"):
                out[key][c, k] = r[key]
    means = np.array([[seq_mean(X[c, k]) for k in range(K)] for c in range(C)])
    out["pooled_mean"] = means.sum(0) / C
    if chains is None:
        e = out["ess"]
        out["pooled_ess"] = np.array([e[:, k][np.isfinite(e[:, k])].sum() if np.isfinite(e[:, k]).any() else NAN
                                      for k in range(K)])
    out["rhat"] = np.array([rhat_of(X[:, k])[0] for k in range(K)])
    out["n"] = n
    return out


def _host(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)


def check(dev, rows, n_samples, columns, burnin=0.1, max_lag=2000, chains=None, pooled=True):
    """Device results (ops.ess_summary) against the restatement, to the tolerances of the feature:
    ESS, ACT, SE and R-hat to relative 1e-9 where the stop lags agree; means within 4 n 2^-53 mean|x|; a stop lag may differ
    only at a near-tie (the pair sum within pair_bound of zero), and is then compared at the device's stop lag.
    chains: check the per-chain values of these chains only.  Returns the number of near-ties met."""
    X, _ = kept(rows, n_samples, columns, burnin)
    C, K, n = X.shape
    assert dev.n == n
    got = {key: _host(getattr(dev, key)) for key in ("mean", "ess", "act", "se_mean", "stop_lag")}
    assert got["mean"].shape == (C, K)
    ties = 0
    for c in (range(C) if chains is None else chains):
        for k in range(K):
            x = X[c, k]
            ref = series(x, max_lag)
            s_dev = int(got["stop_lag"][c, k])
            if s_dev != ref["stop_lag"]:
                t = min(s_dev, ref["stop_lag"])
                d = ref["d"]
                p = autocov(d, t - 1) + autocov(d, t)
                assert t >= 2 and abs(p) <= pair_bound(d, t), (c, k, s_dev, ref["stop_lag"], p, pair_bound(d, t))
                ties += 1
                ref = series(x, max_lag, stop_at=s_dev)
                assert ref["stop_lag"] == s_dev
            tol_m = 4 * n * 2.0 ** -53 * np.abs(x).mean()
            assert abs(got["mean"][c, k] - ref["mean"]) <= tol_m, (c, k, got["mean"][c, k], ref["mean"])
            if ref["stop_lag"] == 0:
                assert np.isnan(got["ess"][c, k]) and np.isnan(got["act"][c, k]) and got["se_mean"][c, k] == 0, (c, k)
                continue
            for key in ("ess", "act", "se_mean"):
                assert np.isclose(got[key][c, k], ref[key], rtol=1e-9, atol=0), (c, k, key, got[key][c, k], ref[key])
    if not pooled:
        return ties
    pm, pe, rh = (_host(getattr(dev, key)) for key in ("pooled_mean", "pooled_ess", "rhat"))
    for k in range(K):
        means = np.array([seq_mean(X[c, k]) for c in range(C)])
        tol = 4 * (n + C) * 2.0 ** -53 * np.abs(X[:, k]).mean()
        assert abs(pm[k] - means.sum() / C) <= tol, (k, pm[k], means.sum() / C)
        r = rhat_of(X[:, k])[0]
        assert (np.isnan(r) and np.isnan(rh[k])) or np.isclose(rh[k], r, rtol=1e-9, atol=0), (k, rh[k], r)
        e = got["ess"][:, k]
        fin = np.isfinite(e)
        want = e[fin].sum() if fin.any() else NAN              # (the device's own per-chain values, checked above)
        assert (np.isnan(want) and np.isnan(pe[k])) or np.isclose(pe[k], want, rtol=1e-12, atol=0), (k, pe[k], want)
    return ties
