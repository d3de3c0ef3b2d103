"""Numpy restatement of lr_col_summary / lr_curve_summary (include/literate_hip.h): "np.mean and calcHPD of a column" with
the grouping rules - what plotDD.py make_vec_dict and logAverager.py take of a log's columns.

Written from the definitions: every chain drops its first int(burnin * S) rows; per chain, or the kept rows pooled chain
after chain; a triple is (mean, HPD low, HPD high) with the HPD the first window of n_in = round-half-even(0.95 n) sorted
values of minimum width (the reference scans with a strict `<`), its ends sample values.  A column that holds a NaN is
NaN three times."""
import numpy as np


def n_in_of(n):
    return int(round(0.95 * n))          # Python rounds half to even


def triple(x):
    """(mean, HPD low, HPD high) of one column"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    n_in = n_in_of(n)
    if n_in < 2:
        raise RuntimeError("not enough data")
    if np.isnan(x).any():
        return np.array([np.nan, np.nan, np.nan])
    d = np.sort(x)
    w = d[n_in - 1:] - d[:n - n_in + 1]
    i = 0
    for k in range(len(w)):              # the reference's scan: the first window of minimum width
        if w[k] < w[i]:
            i = k
    return np.array([np.mean(x), d[i], d[i + n_in - 1]])


def triples(X):
    """X [n, K] -> [K, 3]; the scan vectorised (np.argmin returns the first minimum: the strict `<` scan)"""
    X = np.asarray(X, dtype=np.float64)
    n, K = X.shape
    n_in = n_in_of(n)
    if n_in < 2:
        raise RuntimeError("not enough data")
    d = np.sort(X, axis=0)
    w = d[n_in - 1:] - d[:n - n_in + 1]
    out = np.empty((K, 3))
    bad = np.isnan(X).any(axis=0)
    # a NaN width (inf - inf) in the reference's scan: as the first width it is never replaced (window 0), as a later one
    # it never compares below the minimum
    i = np.where(np.isnan(w[0]), 0, np.argmin(np.where(np.isnan(w), np.inf, w), axis=0))
    out[:, 0] = np.ascontiguousarray(X.T).mean(axis=1)      # (pairwise summation along the contiguous axis)
    out[:, 1] = d[i, np.arange(K)]
    out[:, 2] = d[i + n_in - 1, np.arange(K)]
    out[bad] = np.nan
    return out


def groups(T, n_samples, burnin, pooled):
    """T [>= S, C, K] -> list of [n, K] groups: per chain, or one of the kept rows chain after chain"""
    T = np.asarray(T, dtype=np.float64)
    S = int(n_samples)
    burn = int(burnin * S)
    kept = T[burn:S]
    if pooled:
        return [np.concatenate([kept[:, c] for c in range(T.shape[1])], axis=0)]
    return [kept[:, c] for c in range(T.shape[1])]


def col_summary(T, n_samples, cols, burnin, pooled):
    """-> [G, len(cols), 3]"""
    return np.stack([triples(g[:, list(cols)]) for g in groups(T, n_samples, burnin, pooled)])


def curve_summary(kind_tables, n_samples, burnin, pooled):
    """kind_tables: per kind the per-bin columns [>= S, C, n_bins] (as the logs hold them) -> [G, kinds, 3, n_bins]"""
    per_kind = [np.stack([triples(g).T for g in groups(t, n_samples, burnin, pooled)]) for t in kind_tables]   # [G, 3, nb]
    return np.stack(per_kind, axis=1)


def check(got, want, what=""):
    """got, want [..., 3] (triples on the last axis): HPD ends bit-identical (NaN where NaN), means within rtol 1e-12"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for e in (1, 2):
        assert np.array_equal(got[..., e], want[..., e], equal_nan=True), (what, "HPD end", e)
    assert np.allclose(got[..., 0], want[..., 0], rtol=1e-12, atol=0, equal_nan=True), (what, "mean")
