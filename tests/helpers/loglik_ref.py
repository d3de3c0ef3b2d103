"""References and the error bound for the value tests of lr_bd_loglik_batch (tests/helpers/loglik_cases.py).

terms / loglik   the gather form, term by term, in np.longdouble: tests/helpers/waic_ref.matrix, which restates the
                 per-lineage term from oracle.literate_oracle.per_lineage_tables / lineage_bins, has model 3's second table
                 class (te >= end_time: the birth process alone) and returns the error scale A_i of every lineage; model 1
                 (R = mu, logB = log lam on bins with k > 0) adds the per-chain constant -sum lam[k > 0].
binned           a second reference that shares no index rule with the first: oracle.literate_oracle.calc_likelihood on the
                 precompute_events / get_br statistics of the unit windows (model 3: ex_dead / br_dead from the te < end_time
                 subset, as bin_events_dead forms them).
plain            the same terms in plain float64 numpy with hooks for the mutations of tests/test_loglik_matrix_host.py.

The bound (tolerance), per chain c:

    tol_c = eps (c_term sum_i A_i + depth sum_i |l_ic|) [+ eps c_const |const_c|, model 1],    eps = 2^-52 = 2 u

A_i = max_c(|logB[js]| + |logD[je]| + sum_b R_cb) (+ 1 in models 0 / 1, below) bounds every intermediate of lineage i's term.

c_term - the rounding of ONE term  t = fma(fe, E.y, fma(fs, S.y, S.x + E.x)),  S.x = logB + cum_js, E.x = logD - cum_je:

  * cum_b is a chain of K additions of R's, each R = lam + mu itself rounded once: |d cum| <= (K + 1) u sum R.  The kernel
    (lr_build_tables_wave, P = ceil(n_bins / 64) bins per lane) adds an R at most P - 1 times into its lane's sum, 7 times
    in the wave's prefix scan and P - 1 times in the lane's walk over its bins: 2 P + 5 (for n_bins >= 9 no more than the
    next count; the in-lane walk is what a count of P + 6 leaves out).  numpy's cumsum in the float64 restatement adds
    n_bins times.  K = max(n_bins, 2 P + 5) covers both.  Two cum values enter a term: 2 (K + 1) u A = (K + 1) eps A.
  * lr_log is within 1.2 ulp, and ulp(x) <= eps |x|: 1.2 eps (|logB| + |logD|) <= 1.2 eps A.  Models 0 / 1 round the
    argument (k lam, mu k) first, a relative u there = an absolute u in the logarithm whatever its size: A_i + 1 covers it.
  * storing S.x and E.x: u (|logB| + cum) + u (|logD| + cum) <= 2 u A = 1 eps A; the add S.x + E.x: u A = 0.5 eps A.
  * the two fma round once each, |result| <= 2 A: 2 u 2 A = 2 eps A.
  * the in-bin fractions: fs = s - floor s is the same float64 operation in kernel and reference; fe is (e - ceil e) + 1
    in the fast kernels, e - (ceil e - 1) in the others and te - (t0 + bin) in the oracle - each within u of the exact
    fraction, times |R| <= A: u A = 0.5 eps A.

  c_term = (K + 1) + 1.2 + 1 + 0.5 + 2 + 0.5 = K + 6.2, taken as K + 7.

depth - the additions on the longest path from a term to out[c] (loglik_cases.depth computes it from the restated plan): a
sum whose every partial sum is bounded by sum |l| is off by at most depth u sum |l| to first order; eps = 2 u leaves the
higher orders room.

c_const (model 1) - the constant -sum lam[k > 0] is summed per lane (P additions), by the wave (7) and added to the result
(1): P + 8.

Non-finite results are compared by class: where the reference is -inf / +inf / nan the kernel must give the same."""
import numpy as np

from oracle import literate_oracle as lo

from . import waic_ref as W

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


def terms(ts, te, t0, lam, mu, model, br_length=None, end_time=0.0, dtype=LD):
    """(L [n, C], A [n])"""
    L, A = W.matrix(ts, te, t0, lam, mu, model, br_length, end_time, dtype)
    return L, (A + 1.0 if model < 2 else A)


def constant(lam, model, br_length, dtype=LD):
    """[C]: what belongs to no lineage"""
    lam = np.atleast_2d(np.asarray(lam, dtype=np.float64))
    if model != 1:
        return np.zeros(lam.shape[0], dtype=dtype)
    ok = np.asarray(br_length, dtype=np.float64) > 0
    return -np.sum(lam[:, ok].astype(dtype), axis=1)


def loglik(ts, te, t0, lam, mu, model, br_length=None, end_time=0.0, dtype=LD):
    """(out [C] in `dtype`, L, A)"""
    L, A = terms(ts, te, t0, lam, mu, model, br_length, end_time, dtype)
    with np.errstate(invalid="ignore"):
        return np.sum(L, axis=0, dtype=dtype) + constant(lam, model, br_length, dtype), L, A


def c_term(n_bins):
    P = -(-int(n_bins) // 64)
    return max(int(n_bins), 2 * P + 5) + 7


def c_const(n_bins):
    return -(-int(n_bins) // 64) + 8


def tolerance(L, A, depth, n_bins, const=None):
    """[C] (inf where the chain's terms are not all finite: those chains are compared by class)"""
    with np.errstate(invalid="ignore"):
        absl = np.sum(np.abs(np.asarray(L, dtype=LD)), axis=0).astype(np.float64)
    tol = EPS * (c_term(n_bins) * float(np.sum(A)) + depth * absl)
    if const is not None:
        tol = tol + EPS * c_const(n_bins) * np.abs(np.asarray(const, dtype=np.float64))
    return np.where(np.isfinite(tol), tol, np.inf)


def ratios(got, want, tol):
    """[C] |got - want| / tol; a chain whose reference is not finite gives 0 when the classes agree and inf otherwise"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    out = np.zeros(len(got))
    for c in range(len(got)):
        w = float(want[c])
        if np.isfinite(w):
            d = float(abs(LD(got[c]) - want[c])) if np.isfinite(got[c]) else np.inf
            out[c] = 0.0 if d == 0.0 else d / tol[c]
        else:
            same = (np.isnan(w) and np.isnan(got[c])) or (not np.isnan(w) and got[c] == w)
            out[c] = 0.0 if same else np.inf
    return out


# ------------------------------------------------------------------------------------------------
# the binned form
# ------------------------------------------------------------------------------------------------
def unit_stats(ts, te, t0, n_bins):
    sp, ex, br = np.zeros(n_bins), np.zeros(n_bins), np.zeros(n_bins)
    for b in range(n_bins):
        sp[b], ex[b], br[b] = lo.precompute_events(ts, te, t0 + b, t0 + b + 1)
    return sp, ex, br


def binned(ts, te, t0, lam, mu, model, br_length=None, end_time=0.0):
    """(out [C] float64, scale [C]) or None where the form is not defined: models 0 / 1 with a br_length that is not the
    lineage-time of the data (there k and the exposure are one vector).  A chain with a rate that is not positive and finite
    comes out nan (log(0) * 0).  scale_c = sum_b |logB| sp + |logD| ex + R br: with numpy's pairwise sums and get_br's, each
    statistic and the sum over bins are within (log2(n) + log2(n_bins) + 8) u of exact, relative to that scale."""
    ts, te = np.asarray(ts, dtype=np.float64), np.asarray(te, dtype=np.float64)
    lam, mu = np.atleast_2d(np.asarray(lam, dtype=np.float64)), np.atleast_2d(np.asarray(mu, dtype=np.float64))
    n_bins = lam.shape[1]
    sp, ex, br = unit_stats(ts, te, float(t0), n_bins)
    stats = dict(sp=sp, ex=ex, br=br)
    if model < 2:
        k = np.asarray(br_length, dtype=np.float64)
        if not np.allclose(k, br, rtol=1e-13, atol=0.0):
            return None
        stats["br"] = k
    if model == 3:
        dead = te < end_time
        _, stats["ex_dead"], stats["br_dead"] = unit_stats(ts[dead], te[dead], float(t0), n_bins)
    out, scale = np.empty(lam.shape[0]), np.empty(lam.shape[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        for c in range(lam.shape[0]):
            out[c] = lo.calc_likelihood(model, lam[c], mu[c], stats)
            exd, brd = (stats["ex_dead"], stats["br_dead"]) if model == 3 else (ex, stats["br"])
            scale[c] = np.sum(np.abs(np.log(lam[c])) * sp + lam[c] * stats["br"] + np.abs(np.log(mu[c])) * exd + mu[c] * brd)
            if model < 2:
                kk = np.where(stats["br"] > 0, stats["br"], 1.0)
                scale[c] += np.sum(np.abs(np.log(kk)) * (sp + ex)) + np.sum(lam[c])
    return out, scale


def binned_tolerance(scale, n, n_bins):
    return EPS * (np.log2(max(n, 2)) + np.log2(max(n_bins, 2)) + 8.0) * scale


# ------------------------------------------------------------------------------------------------
# plain float64, with the mutations the host test applies
# ------------------------------------------------------------------------------------------------
MUTATIONS = ("birth_bin", "death_bin", "drop_last", "class_gt", "extant_full", "swap_chains", "ignore_br_mask", "no_const")


def plain(ts, te, t0, lam, mu, model, br_length=None, end_time=0.0, mutate=None, lineage=None, swap=None):
    """(L [n, C] float64, const [C]) of the gather form in plain numpy, or None where `mutate` does not apply.
    lineage: the one birth_bin / death_bin move; swap: the two chains swap_chains exchanges."""
    ts, te = np.asarray(ts, dtype=np.float64), np.asarray(te, dtype=np.float64)
    lam, mu = np.atleast_2d(np.asarray(lam, dtype=np.float64)), np.atleast_2d(np.asarray(mu, dtype=np.float64))
    C, n_bins = lam.shape
    n = len(ts)
    js, fs, je, fe = lo.lineage_bins(ts, te, float(t0), n_bins)
    if model == 3:
        extant = (te > end_time) if mutate == "class_gt" else (te >= end_time)
        # (a lineage wholly outside the window scores 0 in either class)
        if mutate == "class_gt" and not np.any((te == end_time) & (te > t0) & (ts < t0 + n_bins)):
            return None
    else:
        extant = np.zeros(n, dtype=bool)
    if mutate in ("class_gt", "extant_full") and (model != 3 or not np.any(te >= end_time)):
        return None
    if mutate == "extant_full":
        extant = np.zeros(n, dtype=bool)
    if mutate in ("birth_bin", "death_bin"):
        if lineage is None:
            return None
        js, je = js.copy(), je.copy()
        (js if mutate == "birth_bin" else je)[lineage] += 1
    k = None if br_length is None else np.asarray(br_length, dtype=np.float64)
    if mutate == "ignore_br_mask":
        if model >= 2 or not np.any((k == 0) & (np.bincount(js, minlength=n_bins + 2)[1:-1] + np.bincount(je, minlength=n_bins + 2)[1:-1] > 0)):
            return None
    if mutate == "no_const" and model != 1:
        return None
    if mutate == "swap_chains" and swap is None:
        return None
    L = np.empty((n, C))
    const = np.zeros(C)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for c in range(C):
            if model >= 2:
                logB, logD, R = np.log(lam[c]), np.log(mu[c]), lam[c] + mu[c]
            else:
                ok = np.ones(n_bins, dtype=bool) if mutate == "ignore_br_mask" else k > 0
                kk = np.where(k > 0, k, 1.0)
                logB = np.where(ok, np.log(kk * lam[c]) if model == 0 else np.log(lam[c]), 0.0)
                logD = np.where(ok, np.log(mu[c] * kk), 0.0)
                R = np.where(ok, lam[c] + mu[c] if model == 0 else mu[c], 0.0)
                if model == 1 and mutate != "no_const":
                    const[c] = -np.sum(lam[c][ok])
            for cls in (0, 1):
                sel = extant if cls else ~extant
                if not sel.any():
                    continue
                Rc, logDc = (lam[c], np.zeros(n_bins)) if cls else (R, logD)
                cum = np.concatenate(([0.0], np.cumsum(Rc)))
                SA = np.concatenate(([0.0], logB + cum[:-1], cum[-1:]))
                SR = np.concatenate(([0.0], Rc, [0.0]))
                EA = np.concatenate(([0.0], logDc - cum[:-1], -cum[-1:]))
                a, b = js[sel], je[sel]
                L[sel, c] = SA[a] + fs[sel] * SR[a] + EA[b] - fe[sel] * SR[b]
    if mutate == "drop_last":
        L = L[:-1]
    if mutate == "swap_chains":
        i, j = swap
        L[:, [i, j]] = L[:, [j, i]]
        const[[i, j]] = const[[j, i]]
    return L, const


def seq_sum(L, const, reverse=False):
    """[C]: one float64 accumulator per chain, the lineages in order (or reversed)"""
    L = L[::-1] if reverse else L
    with np.errstate(invalid="ignore"):
        return np.cumsum(L, axis=0)[-1] + const if len(L) else const.copy()
