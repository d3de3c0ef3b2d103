"""numpy restatement of PSIS-LOO (literate_amd/loo.py, csrc/lr_loo.hip), written straight from the published algorithm
(Vehtari, Simpson, Gelman, Yao & Gabry, "Pareto smoothed importance sampling"; Vehtari, Gelman & Gabry 2017; the fit of
Zhang & Stephens 2009 as loo::gpdfit does it), in float64 or np.longdouble, one row at a time and with no online forms.

Per row of S terms l, r = -l, rmax = max r:
    M = min(floor(0.2 S), ceil(3 sqrt S))          (relative efficiency 1)
    the draws sorted ascending by (r, draw index); the last M are the tail t_1 <= ... <= t_M, the one below them the cutoff c
    M < 5 or t_M == t_1: unsmoothed, k = +inf
    x_j = exp(t_j - rmax) - exp(c - rmax); gpdfit(x) -> k, sigma; a k or sigma that is not finite: unsmoothed, k = +inf
    lw(tail j) = min(log(qgpd((j - 1/2) / M; k, sigma) + exp(c - rmax)), 0), lw(others) = r - rmax
    elpd_loo = logsumexp(l + lw) - logsumexp(lw) = (max(l + lw) - max lw) + log(sum exp(l + lw - max) / sum exp(lw - max))
    lppd = max l + log(1/S sum exp(l - max l));  n_eff = 1 / sum (normalised weights)^2;  reported k = (M k + 5) / (M + 10)
A row with a term that is not finite is flagged: four NaN, left out of the totals."""
import math

import numpy as np

from helpers import waic_ref

EPS = waic_ref.EPS
TOTALS = ("lineages_used", "lineages_flagged", "elpd_loo", "se_elpd", "p_loo", "lppd", "n_k_gt_0.5", "n_k_gt_0.7",
          "n_unsmoothed", "max_k")


def tail_length(S):
    """min(floor(0.2 S), ceil(3 sqrt S)) in integers"""
    return min(S // 5, math.isqrt(9 * S - 1) + 1)


def grid_points(M):
    return 30 + math.isqrt(M) if M >= 5 else 0


def qgpd(p, k, sigma):
    """the quantile function of the generalized Pareto distribution (location 0)"""
    p = np.asarray(p, dtype=np.result_type(k, sigma, np.float64))
    if k == 0:
        return -sigma * np.log1p(-p)
    return sigma * np.expm1(-k * np.log1p(-p)) / k


def gpdfit(x):
    """Zhang & Stephens (2009) as loo::gpdfit: x sorted ascending -> (k before the prior step, sigma)"""
    x = np.asarray(x)
    dt = x.dtype.type
    M = len(x)
    m = 30 + math.isqrt(M)
    q = int(math.floor(M / 4 + 0.5))
    j = np.arange(1, m + 1).astype(x.dtype)
    with np.errstate(all="ignore"):
        theta = dt(1) / x[-1] + (dt(1) - np.sqrt(dt(m) / (j - dt(0.5)))) / (dt(3) * x[q - 1])
        kj = np.array([np.sum(np.log1p(-t * x)) / dt(M) for t in theta], dtype=x.dtype)
        ell = dt(M) * (np.log(-theta / kj) - kj - dt(1))
        w = np.array([dt(1) / np.sum(np.exp(ell - e)) for e in ell], dtype=x.dtype)
        theta_hat = np.sum(theta * w)
        k = np.sum(np.log1p(-theta_hat * x)) / dt(M)
        sigma = -k / theta_hat
    return k, sigma


def psis_row(l):
    """one row of finite terms -> dict(M, tail, cutoff, k_fit, sigma, k, out [4], lw, cond, gap)"""
    l = np.asarray(l)
    dt = l.dtype.type
    S = len(l)
    M = tail_length(S)
    r = -l
    order = np.argsort(r, kind="stable")                  # ascending by (r, draw index)
    tail = order[S - M:]
    rmax = r[order[-1]]
    c = r[order[S - M - 1]] if M > 0 else rmax
    lw = r - rmax
    k_fit, sigma, k, cond, gap = dt(np.inf), dt(np.nan), dt(np.inf), 1.0, float("inf")
    if M >= 1:
        gap = float(r[tail[0]] - c)
    if M >= 5 and r[tail[-1]] != r[tail[0]]:
        ec = np.exp(c - rmax)
        x = np.exp(r[tail] - rmax) - ec
        with np.errstate(all="ignore"):
            cond = float(min(x[-1] / x[0], 1e6)) if x[0] > 0 else 1e6
        kf, sg = gpdfit(x)
        if np.isfinite(kf) and np.isfinite(sg):
            k_fit, sigma = kf, sg
            p = (np.arange(1, M + 1).astype(l.dtype) - dt(0.5)) / dt(M)
            with np.errstate(all="ignore"):
                lw = lw.copy()
                lw[tail] = np.minimum(np.log(qgpd(p, kf, sg) + ec), dt(0))
            k = (dt(M) * kf + dt(5)) / (dt(M) + dt(10))
    a = l + lw
    mA, mB = a.max(), lw.max()
    sA, sB = np.sum(np.exp(a - mA)), np.sum(np.exp(lw - mB))
    elpd = (mA - mB) + np.log(sA / sB)
    ml = l.max()
    lppd = ml + np.log(np.sum(np.exp(l - ml)) / dt(S))
    wn = np.exp(lw - mB) / sB
    n_eff = dt(1) / np.sum(wn * wn)
    return dict(M=M, tail=tail, cutoff=c, k_fit=k_fit, sigma=sigma, k=k, out=np.array([elpd, k, lppd, n_eff], dtype=l.dtype),
                lw=lw, cond=cond, gap=gap)


def totals(pw, bad):
    pw = np.asarray(pw)
    use = ~np.asarray(bad)
    n = int(use.sum())
    elpd, k, lppd = pw[use, 0], pw[use, 1], pw[use, 2]
    fin = np.isfinite(k)
    nan = np.nan
    se = np.sqrt(n * np.var(elpd, ddof=1)) if n >= 2 else nan
    return np.array([n, int((~use).sum()), elpd.sum() if n else nan, se, (lppd - elpd).sum() if n else nan,
                     lppd.sum() if n else nan, int((k[fin] > 0.5).sum()), int((k[fin] > 0.7).sum()), int((~fin).sum()),
                     k[fin].max() if fin.any() else nan], dtype=pw.dtype)


def psis(L, dtype=np.float64):
    """L [n, S] -> dict: M, tails (a list: the tail's draw indices per row in its sorted order, None where flagged), cutoff
    [n], k_fit [n] (before the prior step), sigma [n], pointwise [n, 4] = (elpd_loo, pareto_k, lppd, n_eff), flagged [n],
    totals [10], cond [n] (x_M / x_1 capped at 1e6; 1 where nothing is fitted), gap [n] (t_1 - c)"""
    L = np.asarray(L).astype(dtype)
    n, S = L.shape
    bad = ~np.isfinite(L).all(axis=1)
    pw = np.full((n, 4), np.nan, dtype=dtype)
    tails, cutoff, k_fit, sigma = [None] * n, np.full(n, np.nan, dtype=dtype), np.full(n, np.nan, dtype=dtype), np.full(n, np.nan, dtype=dtype)
    cond, gap = np.ones(n), np.full(n, np.inf)
    for i in np.nonzero(~bad)[0]:
        row = psis_row(L[i])
        pw[i], tails[i], cutoff[i], k_fit[i], sigma[i], cond[i], gap[i] = (row["out"], row["tail"], row["cutoff"], row["k_fit"],
                                                                          row["sigma"], row["cond"], row["gap"])
    return dict(M=tail_length(S), tails=tails, cutoff=cutoff, k_fit=k_fit, sigma=sigma, pointwise=pw, flagged=bad,
                totals=totals(pw, bad), cond=cond, gap=gap)


def loo(ts, te, t0, lam_bins, mu_bins, model=2, br_length=None, end_time=0.0, dtype=np.float64):
    """the terms by waic_ref.matrix, then psis; also A [n] (the error scale of a lineage's term) and L"""
    L, A = waic_ref.matrix(ts, te, t0, lam_bins, mu_bins, model, br_length, end_time, dtype)
    out = psis(L, dtype)
    out["A"], out["L"] = A, L
    return out


def value_units(ref, u_term=None):
    """[n, 4]: the error unit of each output of a longdouble restatement `ref`: eps max(1, |value|) times the row's tail
    condition x_M / x_1 (capped at 1e6), plus the term's own unit u_i (eps A_i) where the rows were computed from rates"""
    pw = ref["pointwise"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        mag = np.fmax(1.0, np.where(np.isfinite(pw), np.abs(pw), 1.0))
    U = EPS * mag * ref["cond"][:, None]
    if u_term is not None:
        U = U + np.asarray(u_term)[:, None] * ref["cond"][:, None]
    return U


def error_counts(got, ref, u_term=None):
    """worst |got - ref| per output column in value_units; +inf and NaN must sit in the same places"""
    got = np.asarray(got)
    want = ref["pointwise"]
    assert np.array_equal(np.isnan(got), np.isnan(want.astype(np.float64))), "NaN in different places"
    assert np.array_equal(np.isposinf(got), np.isposinf(want.astype(np.float64))), "+inf in different places"
    fin = np.isfinite(want.astype(np.float64))
    U = value_units(ref, u_term)
    with np.errstate(invalid="ignore"):
        d = np.abs(np.where(fin, got, 0.0).astype(np.longdouble) - np.where(fin, want, 0.0)).astype(np.float64)
    c = np.where(d == 0.0, 0.0, d / U)
    return c.max(axis=0) if len(c) else np.zeros(4)
