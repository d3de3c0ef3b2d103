"""Numpy restatement of the joint sampler of (death-rate skyline, Weibull shape) - include/literate_hip_adej.h,
literate_amd/csrc/lr_adej.hip - and its specification: statement by statement, with the addressed draws of
oracle/philox.py (the device's stream) and the reversible-jump moves and priors of oracle/literate_oracle.py.

The model is include/literate_hip_ade.h's with c = 1 (the multiplier is absorbed into the rates):

    l(mu, k) = sum_classes n (-H[jb][a] + log(-expm1(-(H[jb][a + 1] - H[jb][a])))) - sum_jb cens[jb] H[jb][A - jb]      (loglik_cum)
             = -sum_j w_k[j] M[j] + sum_classes n log(-expm1(-mu[je] w_k[a])),  M[j] = sum_{jb < A - j} R[jb][j] mu[jb + j]   (loglik)
    R[jb][j] = cens[jb] + sum_{a > j, jb + a < A} dead[jb][a]

State of a chain: K rates m, K + 1 times (t0 .. t0 + A), g = log shape, rate_hp, poi_hp.  Priors: Gamma(2, rate rate_hp) on
every rate, -log(A) (K - 1) on the shift times, Poisson_prior(K, poi_hp), g flat on [-log 8, log 8] (its constant density is
left out of the prior column).  One iteration `it`:

    (r0, r1) = pair(it, P_MOVE, 0); the acceptance uniform is pair(it, P_ACCEPT, 0)[0]
    r0 < 0.30                 multiplier on the rates (d = 1.1, f = 0.75; the pairs (it, P_MULT, j))
    r0 < 0.60                 g' = g + (pair(it, P_SHAPE, 0)[0] - 0.5) win; outside the bounds: rejected
    r0 < 0.999 and not const  r1 > 0.5: add a shift (position and offset pair(it, P_RJ, 1), Beta(10, 10) from the Gamma
                              variates (it, P_BETA_A / P_BETA_B)), forced reject at K = KMAX; else remove the shift
                              1 + int(pair(it, P_RJ, 1)[0] (K - 1)) if K > 1, and at K = 1 the unchanged state is scored
    else                      Gibbs: poi_hp = Gamma(2 + K) / 2 (it, P_GIBBS_POI) unless fixed, rate_hp = Gamma(1.2 + 2 K) /
                              (0.1 + sum m) (it, P_GIBBS_RATE) if use_rate_hp; always accepted, and the prior is recomputed
                              under the new hyper-parameters
    min |t[j + 1] - t[j]| <= 1 rejects; otherwise accepted iff lik - likA + prior - priorA + hastings >= log(u)

The initial state (K = 1) comes from the stream at it = 0 under P_INIT: m = 0.2 Gamma(2) (attempts from index 0), g uniform
on [-log 4, log 4] from pair(0, P_INIT, 64)[0]; rate_hp = 1, poi_hp = 1 or the fixed value.

run() returns, beside the rows, for every iteration the move kind, whether it was accepted, and the margin
|log ratio - log u| of its Metropolis-Hastings decision (inf where nothing was decided by a comparison)."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import literate_oracle as lo  # noqa: E402
from oracle import philox as px  # noqa: E402
from helpers import ade_ref  # noqa: E402

KMAX = 32
MAX_BINS = 128
LOG_SHAPE_MAX = math.log(8.0)
INIT_RATE_SCALE = 0.2
INIT_LOG_SHAPE_SPAN = 2.0 * math.log(4.0)
UPDATE_FRACTION = 0.75
P_SHAPE, P_INIT, P_GIBBS_POI, P_GIBBS_RATE = 48, 49, 50, 51
MOVES = ("mult", "shape", "add", "remove", "gibbs")
MULT, SHAPE, ADD, REMOVE, GIBBS = range(5)
ROW_HEAD = ("it", "posterior", "lik", "prior", "shape", "log_shape", "K", "mean_rate", "rate_hp", "poi_hp")
ROW_W = len(ROW_HEAD) + KMAX + KMAX - 1
COL = {k: i for i, k in enumerate(ROW_HEAD)}


class Settings:
    def __init__(self, const=0, use_rate_hp=1, poisson_prior=0.0, win=0.4):
        self.const, self.use_rate_hp, self.poisson_prior, self.win = int(const), int(use_rate_hp), float(poisson_prior), float(win)


# ------------------------------------------------------------------------------------------------
# the likelihood
# ------------------------------------------------------------------------------------------------
def risk(dead, cens):
    """R[jb][j], int64 [A, A] (0 where jb + j >= A): the lineages of birth bin jb that live past age j"""
    dead, cens = np.asarray(dead, dtype=np.int64), np.asarray(cens, dtype=np.int64)
    A = len(cens)
    R = np.zeros((A, A), dtype=np.int64)
    for jb in range(A):
        run = int(cens[jb])
        for j in range(A - jb - 1, -1, -1):
            R[jb, j] = run
            run += max(int(dead[jb, j]), 0)
    return R


class Data:
    """what the likelihood takes of the data: R, and the classes (je, a, n) in the table's own order"""

    def __init__(self, dead, cens):
        self.dead, self.cens = np.asarray(dead, dtype=np.int64), np.asarray(cens, dtype=np.int64)
        self.A = A = len(self.cens)
        self.R = risk(dead, cens)
        jb, a, n = ade_ref.class_list(self.dead)
        self.je, self.a, self.n = jb + a, a, n
        # M = T mu:  T[j][b] = R[b - j][j], b >= j
        self.T = np.zeros((A, A))
        for j in range(A):
            self.T[j, j:] = self.R[:A - j, j]


def risk_sums(data, mu):
    return data.T @ np.asarray(mu, dtype=np.float64)


def loglik(data, mu, k, M=None, w=None):
    """l(mu, k) in the form without a cumulative sum"""
    mu = np.asarray(mu, dtype=np.float64)
    if w is None:
        w = ade_ref.weights(k, data.A)
    if M is None:
        M = risk_sums(data, mu)
    with np.errstate(divide="ignore"):
        return float(-np.dot(w, M) + np.sum(data.n * np.log(-np.expm1(-mu[data.je] * w[data.a]))))


def loglik_cum(data, mu, k):
    """l(mu, k) as include/literate_hip_ade.h writes it: one cumulative hazard per birth bin, class by class"""
    A = data.A
    mu = [float(v) for v in mu]
    k = float(k)
    w = [1.0] + [j ** k * math.expm1(k * math.log1p(1.0 / j)) for j in range(1, A)]
    tot = 0.0
    for jb in range(A):
        H = [0.0]
        for j in range(A - jb):
            H.append(H[-1] + mu[jb + j] * w[j])
        for a in range(A - jb):
            if data.dead[jb][a] > 0:
                tot += int(data.dead[jb][a]) * (-H[a] + math.log(-math.expm1(-(H[a + 1] - H[a]))))
        tot -= int(data.cens[jb]) * H[A - jb]
    return tot


def loglik_rows(dead, cens, mu_bins, shapes):
    """lr_adej_loglik: (ll [S], flag [S] int32, mag [S]); flag bit 0: a rate that is not finite or negative, or zero in a bin
    with an observed death; bit 1: a shape that is not finite or <= 0; a flagged row is NaN.  mag = sum n |class term| of
    ade_ref.loglik at c = 1, the scale of the tolerance."""
    mu_bins = np.asarray(mu_bins, dtype=np.float64)
    shapes = np.asarray(shapes, dtype=np.float64).reshape(-1)
    data = Data(dead, cens)
    flag = ade_ref.flags(dead, mu_bins).astype(np.int32)
    with np.errstate(invalid="ignore"):
        flag |= 2 * (~(np.isfinite(shapes) & (shapes > 0.0))).astype(np.int32)
    ll, mag = np.full(len(shapes), np.nan), np.full(len(shapes), np.nan)
    for s in range(len(shapes)):
        if flag[s]:
            continue
        ll[s] = loglik(data, mu_bins[s], shapes[s])
        mag[s] = ade_ref.loglik(1.0, *ade_ref.tables(dead, cens, mu_bins[s], shapes[s]))[1]
    return ll, flag, mag


# ------------------------------------------------------------------------------------------------
# the sampler
# ------------------------------------------------------------------------------------------------
class PhiloxDraws:
    """the device's addressed stream for one chain (key = (seed, global chain index))"""

    def __init__(self, seed, chain):
        self.s = px.Stream(seed, chain)

    def init(self):
        return self.s.gamma(0, P_INIT, 0, 2.0) * INIT_RATE_SCALE, (self.s.pair(0, P_INIT, 64)[0] - 0.5) * INIT_LOG_SHAPE_SPAN

    def move(self, it):
        return self.s.pair(it, px.P_MOVE, 0)

    def multiplier(self, it, K, f):
        ff, u = np.zeros(K, dtype=int), np.zeros(K)
        for j in range(K):
            ub, uu = self.s.pair(it, px.P_MULT, j)
            ff[j], u[j] = (1 if ub < f else 0), uu
        return ff, u

    def shape(self, it):
        return self.s.pair(it, P_SHAPE, 0)[0]

    def rj_add(self, it, times):
        K = len(times) - 1
        uc, ud = self.s.pair(it, px.P_RJ, 1)
        ind = min(int(uc * K), K - 1)
        ga = self.s.gamma(it, px.P_BETA_A, 0, lo.SHAPE_BETA_RJ)
        gb = self.s.gamma(it, px.P_BETA_B, 0, lo.SHAPE_BETA_RJ)
        return ind, ud * (times[ind + 1] - times[ind]), ga / (ga + gb)

    def rj_remove(self, it, K):
        return 1 + min(int(self.s.pair(it, px.P_RJ, 1)[0] * (K - 1)), K - 2)

    def gibbs_poi(self, it, shape):
        return self.s.gamma(it, P_GIBBS_POI, 0, shape)

    def gibbs_rate(self, it, shape):
        return self.s.gamma(it, P_GIBBS_RATE, 0, shape)

    def accept(self, it):
        return self.s.pair(it, px.P_ACCEPT, 0)[0]


class NumpyDraws:
    """the same draws from a numpy Generator (the statistical tests of the restatement: any stream will do, and this one
    is much faster than Philox in Python)"""

    def __init__(self, rng):
        self.r = rng

    def init(self):
        return self.r.gamma(2.0) * INIT_RATE_SCALE, (self.r.random() - 0.5) * INIT_LOG_SHAPE_SPAN

    def move(self, it):
        return tuple(self.r.random(2))

    def multiplier(self, it, K, f):
        return (self.r.random(K) < f).astype(int), self.r.random(K)

    def shape(self, it):
        return self.r.random()

    def rj_add(self, it, times):
        K = len(times) - 1
        ind = min(int(self.r.random() * K), K - 1)
        return ind, self.r.random() * (times[ind + 1] - times[ind]), self.r.beta(lo.SHAPE_BETA_RJ, lo.SHAPE_BETA_RJ)

    def rj_remove(self, it, K):
        return 1 + min(int(self.r.random() * (K - 1)), K - 2)

    def gibbs_poi(self, it, shape):
        return self.r.gamma(shape)

    def gibbs_rate(self, it, shape):
        return self.r.gamma(shape)

    def accept(self, it):
        return self.r.random()


def log_prior(m, A, rate_hp, poi_hp):
    K = len(m)
    return float(lo.prior_gamma(m, lo.GAMMA_SHAPE, rate_hp) - math.log(A) * (K - 1) + lo.Poisson_prior(K, poi_hp))


def bins_of(m, times, A):
    return np.asarray(m)[lo.get_rate_index(np.floor(times), A)]


class State:
    def __init__(self, m, times, g, rate_hp, poi_hp, lik, prior):
        self.m, self.times, self.g = np.array(m, dtype=float), np.array(times, dtype=float), float(g)
        self.rate_hp, self.poi_hp, self.lik, self.prior = float(rate_hp), float(poi_hp), float(lik), float(prior)
        self.proposed, self.accepted = np.zeros(len(MOVES), dtype=np.int64), np.zeros(len(MOVES), dtype=np.int64)

    def row(self, it):
        K = len(self.m)
        r = np.full(ROW_W, np.nan)
        r[:len(ROW_HEAD)] = [it, self.lik + self.prior, self.lik, self.prior, math.exp(self.g), self.g, K, np.mean(self.m),
                             self.rate_hp, self.poi_hp]
        r[len(ROW_HEAD):len(ROW_HEAD) + K] = self.m
        r[len(ROW_HEAD) + KMAX:len(ROW_HEAD) + KMAX + K - 1] = self.times[1:K]
        return r


def init_state(data, t0, st, draws):
    A = data.A
    m0, g0 = draws.init()
    m, times = np.array([m0]), np.array([float(t0), float(t0) + A])
    poi_hp = st.poisson_prior if st.poisson_prior > 0 else 1.0
    return State(m, times, g0, 1.0, poi_hp, loglik(data, bins_of(m, times, A), math.exp(g0)), log_prior(m, A, 1.0, poi_hp))


def run(data, t0, st, draws, n_iters, s_freq=1, it0=0, state=None, k_max=KMAX):
    """n_iters iterations from it0 (from `state`, or from the initial state) -> dict(rows [n, ROW_W], kind, accepted,
    margin [n_iters], K [n_iters] after each iteration, state, forced: add proposals refused at k_max)"""
    A = data.A
    s = init_state(data, t0, st, draws) if state is None else state
    rows, kinds, acc, margins, Ks = [], [], [], [], []
    forced = 0
    for it in range(it0, it0 + n_iters):
        r0, r1 = draws.move(it)
        m, times, g = s.m, s.times, s.g
        hasting, invalid, gibbs = 0.0, False, False
        rate_hp, poi_hp = s.rate_hp, s.poi_hp
        if r0 < 0.30:
            kind = MULT
            m, hasting = lo.update_multiplier_freq(s.m, *draws.multiplier(it, len(s.m), UPDATE_FRACTION))
        elif r0 < 0.60:
            kind = SHAPE
            g = s.g + (draws.shape(it) - 0.5) * st.win
            invalid = not (-LOG_SHAPE_MAX <= g <= LOG_SHAPE_MAX)
        elif r0 < 0.999 and not st.const:
            if r1 > 0.5:
                kind = ADD
                if len(s.m) >= k_max:
                    invalid, forced = True, forced + 1
                else:
                    m, times, hasting = lo.add_shift_RJ_weighted_mean(s.m, s.times, *draws.rj_add(it, s.times))
            else:
                kind = REMOVE
                if len(s.m) > 1:
                    m, times, hasting = lo.remove_shift_RJ_weighted_mean(s.m, s.times, draws.rj_remove(it, len(s.m)))
        else:
            kind, gibbs = GIBBS, True
            if st.poisson_prior == 0:
                poi_hp = draws.gibbs_poi(it, lo.RJHP_GAMMA_SHAPE + len(s.m)) * (1.0 / (lo.RJHP_GAMMA_RATE + 1.0))
            if st.use_rate_hp:
                rate_hp = draws.gibbs_rate(it, lo.HP_GAMMA_SHAPE + lo.GAMMA_SHAPE * len(s.m)) * (1.0 / (lo.HP_GAMMA_RATE + np.sum(s.m)))
        s.proposed[kind] += 1
        u = draws.accept(it)
        margin, ok = math.inf, False
        if gibbs:
            ok = True
            lik, prior = s.lik, log_prior(s.m, A, rate_hp, poi_hp)
        elif not invalid and not np.min(np.abs(np.diff(times))) <= lo.MIN_ALLOWED_T:
            prior = log_prior(m, A, rate_hp, poi_hp)
            lik = loglik(data, bins_of(m, times, A), math.exp(g))
            ratio = lik - s.lik + prior - s.prior + hasting
            log_u = math.log(u) if u > 0 else -math.inf
            ok = bool(ratio >= log_u)
            margin = abs(ratio - log_u)
        if ok:
            s.m, s.times, s.g, s.rate_hp, s.poi_hp, s.lik, s.prior = np.array(m, dtype=float), np.array(times, dtype=float), g, rate_hp, poi_hp, lik, prior
            s.accepted[kind] += 1
        kinds.append(kind), acc.append(ok), margins.append(margin), Ks.append(len(s.m))
        if it % s_freq == 0:
            rows.append(s.row(it))
    return dict(rows=np.array(rows).reshape(-1, ROW_W), kind=np.array(kinds), accepted=np.array(acc), margin=np.array(margins),
                K=np.array(Ks), state=s, forced=forced)


# ------------------------------------------------------------------------------------------------
# exact answers the statistical tests compare with
# ------------------------------------------------------------------------------------------------
def k_prior_pmf(A, poi, kmax=KMAX):
    """p(K) of the prior-only sampler: Poisson_prior(K, poi) x Gamma priors (integrate to 1) x A^-(K - 1) x the volume of the
    ordered K - 1 shift times with every segment longer than 1, (A - K)^(K - 1) / (K - 1)!"""
    K = np.arange(1, kmax + 1)
    lp = np.array([k * math.log(poi) - math.lgamma(k + 1) - math.lgamma(k) + (k - 1) * (math.log(max(A - k, 1e-300) / A)) for k in K])
    lp[K >= A] = -np.inf
    lp[0] = math.log(poi)
    p = np.exp(lp - lp.max())
    return p / p.sum()


def grid_posterior(data, n_g=601, n_lm=801, lm_lo=math.log(1e-3), lm_hi=math.log(3.0), rate_hp=1.0):
    """K = 1, use_rate_hp = 0: the posterior of (log m, g) on a grid (trapezoid weights) -> dict of E and sd of g, g^2, log m"""
    A = data.A
    gs = np.linspace(-LOG_SHAPE_MAX, LOG_SHAPE_MAX, n_g)
    lms = np.linspace(lm_lo, lm_hi, n_lm)
    ms = np.exp(lms)
    lp = np.empty((n_g, n_lm))
    ones = np.ones(A)
    for i, g in enumerate(gs):
        w = ade_ref.weights(math.exp(g), A)
        E = float(np.dot(w, data.T @ ones))
        x = np.outer(ms, w[data.a])                                        # [n_lm, classes]
        with np.errstate(divide="ignore"):
            lp[i] = -ms * E + np.log(-np.expm1(-x)) @ data.n
    # Gamma(2, rate_hp) on m, and the Jacobian of log m
    lp += (np.log(ms) - rate_hp * ms + lms)[None, :]
    wg, wl = np.ones(n_g), np.ones(n_lm)
    wg[[0, -1]] = 0.5
    wl[[0, -1]] = 0.5
    p = np.exp(lp - lp.max()) * wg[:, None] * wl[None, :]
    p /= p.sum()
    G, L = np.meshgrid(gs, lms, indexing="ij")
    out = {}
    for name, f in (("g", G), ("g2", G * G), ("logm", L)):
        e = float((p * f).sum())
        out[name] = (e, math.sqrt(max(float((p * f * f).sum()) - e * e, 0.0)))
    return out
