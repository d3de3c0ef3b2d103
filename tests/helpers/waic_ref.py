"""numpy restatement of the pointwise WAIC (literate_amd/waic.py, csrc/lr_waic.hip): the FULL [lineages, draws] matrix of
per-lineage terms from the oracle's per-bin terms (oracle.literate_oracle.per_lineage_tables) and index rule
(lineage_bins), in float64 or np.longdouble, then the four formulas, the flag rule, the totals and the compare arithmetic,
each as written in the definition (no online forms).

    l[i, s] = (logB + cum)[js] + fs R[js] + (logD - cum)[je] - fe R[je],   cum_b = sum_{b' < b} R_b'
    model 3, te >= end_time: the birth process alone (logB, R = lam; no logD)

The error scale of a lineage is A_i = max_s(|logB[js]| + |logD[je]| + sum_b R[s, b]): the table's cumulative sums set the
size of the rounding errors, not |l| (which may cancel to nothing)."""
import numpy as np

from oracle import literate_oracle as lo

EPS = float(np.finfo(np.float64).eps)
TOTALS = ("lineages_used", "lineages_flagged", "lppd", "p_waic", "elpd_waic", "se_elpd", "n_var_gt_0.4", "max_var")


def bin_terms(lam, mu, model, br_length, dtype):
    """(logB, logD, R) of one draw: float64 from the oracle itself, longdouble by the same rules in longdouble"""
    m = 2 if model == 3 else model
    if dtype == np.float64:
        logB, logD, R, const = lo.per_lineage_tables(lam, mu, m, br_length)
        assert const == 0.0 or m == 1      # (model 1's constant belongs to no lineage: tests/helpers/loglik_ref.py adds it)
        return logB, logD, R
    lam, mu = np.asarray(lam, dtype=dtype), np.asarray(mu, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        if m >= 2:
            return np.log(lam), np.log(mu), lam + mu
        assert m in (0, 1)
        k = np.asarray(br_length, dtype=dtype)
        ok = k > 0
        logB, logD, R = np.zeros_like(lam), np.zeros_like(lam), np.zeros_like(lam)
        if m == 0:
            logB[ok], logD[ok], R[ok] = np.log(k[ok] * lam[ok]), np.log(mu[ok] * k[ok]), lam[ok] + mu[ok]
        else:
            logB[ok], logD[ok], R[ok] = np.log(lam[ok]), np.log(mu[ok] * k[ok]), mu[ok]
        return logB, logD, R


def matrix(ts, te, t0, lam_bins, mu_bins, model=2, br_length=None, end_time=0.0, dtype=np.float64):
    """(L [n, S], A [n]): the terms and the error scale of every lineage"""
    ts, te = np.asarray(ts, dtype=np.float64), np.asarray(te, dtype=np.float64)
    lam_bins, mu_bins = np.atleast_2d(np.asarray(lam_bins, dtype=np.float64)), np.atleast_2d(np.asarray(mu_bins, dtype=np.float64))
    S, n_bins = lam_bins.shape
    js, fs, je, fe = lo.lineage_bins(ts, te, float(t0), n_bins)
    fs, fe = fs.astype(dtype), fe.astype(dtype)
    extant = (te >= end_time) if model == 3 else np.zeros(len(ts), dtype=bool)
    L = np.empty((len(ts), S), dtype=dtype)
    A = np.zeros(len(ts), dtype=np.float64)
    zero = np.zeros(1, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for s in range(S):
            logB, logD, R = bin_terms(lam_bins[s], mu_bins[s], model, br_length, dtype)
            logB, logD, R = logB.astype(dtype), logD.astype(dtype), R.astype(dtype)
            for cls in ((0, 1) if model == 3 else (0,)):
                if cls == 1:
                    R, logD = np.asarray(lam_bins[s], dtype=dtype), np.zeros(n_bins, dtype=dtype)
                sel = extant if cls == 1 else ~extant
                if not sel.any():
                    continue
                cum = np.concatenate((zero, np.cumsum(R)))
                SA = np.concatenate((zero, logB + cum[:-1], cum[-1:]))
                SR = np.concatenate((zero, R, zero))
                EA = np.concatenate((zero, logD - cum[:-1], -cum[-1:]))
                a, b = js[sel], je[sel]
                L[sel, s] = SA[a] + fs[sel] * SR[a] + EA[b] - fe[sel] * SR[b]
                aB = np.concatenate((zero, np.abs(logB), zero))
                aD = np.concatenate((zero, np.abs(logD), zero))
                scale = (aB[a] + aD[b] + cum[-1]).astype(np.float64)
                A[sel] = np.fmax(A[sel], np.where(np.isfinite(scale), scale, 0.0))
    return L, A


def pointwise(L):
    """[n, 3] = (lppd_i, mean_i, var_i) by the defining formulas, NaN where any term of the lineage is not finite; and the
    flags"""
    L = np.asarray(L)
    n, S = L.shape
    bad = ~np.isfinite(L).all(axis=1)
    out = np.full((n, 3), np.nan, dtype=L.dtype)
    G = L[~bad]
    if len(G):
        m = G.max(axis=1)
        lppd = m + np.log(np.sum(np.exp(G - m[:, None]), axis=1) / S)
        mean = np.sum(G, axis=1) / S
        var = np.sum((G - mean[:, None]) ** 2, axis=1) / (S - 1)
        out[~bad] = np.stack([lppd, mean, var], axis=1)
    return out, bad


def totals(pw, bad):
    pw = np.asarray(pw)
    use = ~np.asarray(bad)
    lppd, var = pw[use, 0], pw[use, 2]
    elpd = lppd - var
    n = int(use.sum())
    se = np.sqrt(n * np.var(elpd, ddof=1)) if n >= 2 else np.nan
    return np.array([n, int((~use).sum()), lppd.sum(), var.sum(), elpd.sum(), se, int((var > 0.4).sum()),
                     var.max() if n else np.nan], dtype=pw.dtype)


def waic(ts, te, t0, lam_bins, mu_bins, model=2, br_length=None, end_time=0.0, dtype=np.float64):
    """dict: pointwise [n, 3], flagged [n], totals [8], A [n], spread [n], L"""
    L, A = matrix(ts, te, t0, lam_bins, mu_bins, model, br_length, end_time, dtype)
    pw, bad = pointwise(L)
    with np.errstate(invalid="ignore"):
        spread = np.where(bad, np.nan, (L.max(axis=1) - L.min(axis=1)).astype(np.float64))
    return dict(pointwise=pw, flagged=bad, totals=totals(pw, bad), A=A, spread=spread, L=L)


def units(ref):
    """[n, 3]: the error unit of each output of a restatement `ref` (waic(...)): u_i = eps A_i for lppd_i and mean_i,
    u_i max(spread_i, u_i) for var_i"""
    u = EPS * ref["A"]
    return np.stack([u, u, u * np.fmax(ref["spread"], u)], axis=1)


def error_counts(got, ref):
    """worst |got - ref| per output column, in the units of `ref` (a longdouble restatement); flagged rows must be NaN in
    both and are left out"""
    got = np.asarray(got)
    want = ref["pointwise"]
    bad = ref["flagged"]
    assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
    if bad.all():
        return np.zeros(3)
    U = units(ref)[~bad]
    d = np.abs(got[~bad].astype(np.longdouble) - want[~bad].astype(np.longdouble)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(d == 0.0, 0.0, d / U)
    return c.max(axis=0)


def draw_indices(n_rows, n_draws):
    M, R = int(n_rows), min(int(n_draws), int(n_rows))
    return np.array([(i * M) // R for i in range(R)], dtype=np.int64)


def compare_rows(names, elpds):
    """the compare arithmetic: models sorted by the sum of their finite elpd_i, best first; against the best model, over the
    lineages finite in both: elpd_diff = sum of the differences, se_diff = sqrt(n var(differences, ddof 1))"""
    E = [np.asarray(e, dtype=np.float64) for e in elpds]
    tot = [float(np.nansum(e)) for e in E]
    order = sorted(range(len(E)), key=lambda k: -tot[k])
    best = E[order[0]]
    rows = []
    for k in order:
        both = np.isfinite(E[k]) & np.isfinite(best)
        d = E[k][both] - best[both]
        n = int(both.sum())
        first = k == order[0]
        rows.append(dict(model=names[k], elpd_waic=tot[k], elpd_diff=0.0 if first else float(d.sum()),
                         se_diff=0.0 if first else (float(np.sqrt(n * np.var(d, ddof=1))) if n >= 2 else float("nan"))))
    return rows
