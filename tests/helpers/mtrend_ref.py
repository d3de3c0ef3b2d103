"""Numpy restatement of the joint covariate sampler (include/literate_hip_mtrend.h): the specification the device is held to
(tests/test_hip_mtrend.py) and that tests/test_mtrend_host.py checks without a GPU.

Chain c runs the header's iteration on the one data set with the draws of oracle/philox.py's Stream(seed, chain0 + c),
addressed as the header lists them: the grouped likelihood per side with the accepted E kept in the chain, the prior on every
free coefficient whether included or not, the thresholds, the target (side, covariate), `>` in the acceptance test, the
unconditional acceptance of iteration 0, a NaN likelihood counted as -inf, the six counters.  Every accept decision's margin
|lhs - log u| is recorded (iteration 0 and non-finite sides apart): where none is within TIE of zero, a device that agrees to
1e-9 takes the same decisions.

loglik_bins is the likelihood as trend_rate.py:82 computes it - sum_b log(rate_b) n_b - rate_b DT_b - and the reference of
the grouped form here and on the device.

The cases of tests/test_hip_mtrend.py stand here too (CASES), so the host test can hold every one of them to the tie
condition without a GPU.
"""
import functools
import math

import numpy as np

from oracle.philox import Stream

STATE_W, ROW_W, MOVES = 96, 72, 6
S_L0, S_M0, S_LIK_B, S_LIK_D, S_PRIOR, S_E_B, S_E_D, S_PROPOSED, S_ACCEPTED, S_IL, S_A, S_IM, S_B = 0, 1, 2, 3, 4, 5, 6, 8, 16, 32, 48, 64, 80
P_MOVE, P_NORM, P_ACCEPT, P_INIT = 72, 73, 74, 75
TIE = 1e-6
MAX_BINS, MAX_COVS = 512, 16


class Settings:
    """m_birth / m_death: 1 = the side is constant; win: (birth, death)"""

    def __init__(self, m_birth=0, m_death=0, no_death=0, bvs=1, bvs_from=0, pI=0.1, slab_sd=1.0, win=(0.1, 0.1)):
        self.m_birth, self.m_death, self.no_death, self.bvs, self.bvs_from = m_birth, m_death, no_death, bvs, bvs_from
        self.pI, self.slab_sd, self.win = pI, slab_sd, tuple(win)

    def astuple(self):
        return (self.m_birth, self.m_death, self.no_death, self.bvs, self.bvs_from, self.pI, self.slab_sd, self.win)

    def free(self):
        """the free sides, in the order birth, death"""
        return [s for s, const in ((0, self.m_birth), (1, self.m_death or self.no_death)) if not const]


class Data:
    """n_spec, n_exti, DT [n_bins]; X [P, n_bins]"""

    def __init__(self, n_spec, n_exti, DT, X):
        self.n = [np.asarray(n_spec, dtype=float), np.asarray(n_exti, dtype=float)]
        self.DT, self.X = np.asarray(DT, dtype=float), np.atleast_2d(np.asarray(X, dtype=float))
        self.P, self.n_bins = self.X.shape
        self.N = [float(np.sum(v)) for v in self.n]
        self.SX = [self.X @ v for v in self.n]


# ---- the likelihood and the prior ----------------------------------------------------------------------------------------
def eta_of(D, coef, I):
    eta = np.zeros(D.n_bins)
    for j in range(D.P):
        if I[j]:
            eta = eta + coef[j] * D.X[j]
    return eta


def E_of(D, coef, I):
    with np.errstate(all="ignore"):
        return float(np.sum(D.DT * np.exp(eta_of(D, coef, I))))


def side_lik(D, side, base, coef, I, E):
    """N log(base) + sum_j I_j coef_j SX_j - base E"""
    d = 0.0
    for j in range(D.P):
        if I[j]:
            d += coef[j] * D.SX[side][j]
    with np.errstate(all="ignore"):
        return float(D.N[side] * np.log(base) + d - base * E)


def total(lik_b, lik_d):
    with np.errstate(all="ignore"):
        t = lik_b + lik_d
    return -np.inf if np.isnan(t) else float(t)


def loglik_bins(D, side, base, coef, I):
    """trend_rate.py:82 for one side: sum_b log(rate_b) n_b - rate_b DT_b, a plain loop over the bins"""
    out = 0.0
    for b in range(D.n_bins):
        eta = 0.0
        for j in range(D.P):
            if I[j]:
                eta += coef[j] * D.X[j, b]
        rate = base * math.exp(eta)
        out += math.log(rate) * D.n[side][b] - rate * D.DT[b]
    return out


def prior_base(x):
    return -np.inf if x < .001 else -(x - .001) / 10.0 - math.log(10.0)


def log_prior(D, st, l0, m0, a, I_l, b, I_m):
    """Gamma(1, scale 10, loc .001) on l0 and m0; Normal(0, slab_sd) on every coefficient of a free side; log(pI) or log(1 - pI)
    per free indicator"""
    p = prior_base(l0) + prior_base(m0)
    for side in st.free():
        c, I = (a, I_l) if side == 0 else (b, I_m)
        z = np.asarray(c, dtype=float) / st.slab_sd
        p += float(np.sum(-0.5 * math.log(2.0 * math.pi) - math.log(st.slab_sd) - 0.5 * z * z))
        on = int(np.sum(I))
        p += math.log(st.pI) * on + math.log1p(-st.pI) * (D.P - on)
    return p


# ---- the chain -----------------------------------------------------------------------------------------------------------
class Chain:
    def __init__(self, D, st, stream, given=None):
        self.D, self.st, self.u = D, st, stream
        P, free = D.P, st.free()
        if given is None:
            sdt = float(np.sum(D.DT))
            with np.errstate(all="ignore"):
                base = [D.N[0] / sdt if sdt != 0 else np.nan, D.N[1] / sdt if sdt != 0 else np.nan]
            self.base = [float(x) if (np.isfinite(x) and x > 0) else 0.1 for x in base]
            self.coef = [np.zeros(P), np.zeros(P)]
            self.I = [np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)]
            for side in free:
                for j in range(P):
                    self.coef[side][j] = 0.1 * stream.normal(0, P_INIT, side * P + j)
                if not st.bvs:
                    self.I[side][:] = 1
        else:
            l0, m0, a, I_l, b, I_m = given
            self.base = [float(l0), float(m0)]
            self.coef = [np.array(a, dtype=float), np.array(b, dtype=float)]
            self.I = [(np.array(I_l) != 0).astype(np.int64), (np.array(I_m) != 0).astype(np.int64)]
            for side in (0, 1):
                if side not in free:
                    self.coef[side][:], self.I[side][:] = 0.0, 0
        self.E, self.lik = [0.0, 0.0], [0.0, 0.0]
        for side in (0, 1):
            if side == 1 and st.no_death:
                continue
            self.E[side] = E_of(D, self.coef[side], self.I[side])
            self.lik[side] = side_lik(D, side, self.base[side], self.coef[side], self.I[side], self.E[side])
        self.prior = self.log_prior(self.base, self.coef, self.I)
        self.proposed, self.accepted = [0] * MOVES, [0] * MOVES
        self.margin = np.inf

    def log_prior(self, base, coef, I):
        return log_prior(self.D, self.st, base[0], base[1], coef[0], I[0], coef[1], I[1])

    def full(self):
        """the chain that starts from this one's parameters with every free indicator 1: how MultiTrendRate.py starts a run"""
        ones = np.ones(self.D.P, dtype=np.int64)
        return Chain(self.D, self.st, self.u, given=(self.base[0], self.base[1], self.coef[0], ones, self.coef[1], ones))

    def step(self, it):
        D, st, P = self.D, self.st, self.D.P
        free = st.free()
        F = len(free) * P
        ua, _ = self.u.pair(it, P_ACCEPT, 0)
        r, pick = self.u.pair(it, P_MOVE, 0)
        coin, um = self.u.pair(it, P_MOVE, 1)
        flips = bool(st.bvs) and it >= st.bvs_from
        th1, th2 = (1.0, 1.0) if F == 0 else ((0.10, 0.60) if flips else (0.10, 1.0))
        base, coef, I = list(self.base), [self.coef[0], self.coef[1]], [self.I[0], self.I[1]]
        lik, E, hasting, kinds = list(self.lik), list(self.E), 0.0, []
        if r < th1:
            kinds = [0]
            side = 0 if (st.no_death or coin < 0.5) else 1
            hasting = 2.0 * math.log(1.1) * (um - .5)
            base[side] = self.base[side] * math.exp(hasting)
            if not (side == 1 and st.no_death):
                lik[side] = side_lik(D, side, base[side], coef[side], I[side], E[side])
        else:
            k = min(int(pick * F), F - 1)
            side, j = free[k // P], k % P
            recompute = True
            if r < th2:
                kinds = [1 + side]
                coef[side] = coef[side].copy()
                coef[side][j] += st.win[side] * self.u.normal(it, P_NORM, 0)
                recompute = bool(I[side][j])
                if recompute:
                    kinds.append(4 + side)
            else:
                kinds = [3]
                I[side] = I[side].copy()
                I[side][j] = 1 - I[side][j]
            if recompute:
                E[side] = E_of(D, coef[side], I[side])
                lik[side] = side_lik(D, side, base[side], coef[side], I[side], E[side])
        prior = self.log_prior(base, coef, I)
        with np.errstate(all="ignore"):
            lhs = (total(*lik) - total(*self.lik)) + (prior - self.prior) + hasting
            log_u = math.log(ua) if ua > 0 else -np.inf
        ok = it == 0 or bool(lhs > log_u)
        if it != 0 and np.isfinite(lhs) and np.isfinite(log_u):
            self.margin = min(self.margin, abs(lhs - log_u))
        for k in kinds:
            self.proposed[k] += 1
        if ok:
            self.base, self.coef, self.I, self.lik, self.E, self.prior = base, coef, I, lik, E, prior
            for k in kinds:
                self.accepted[k] += 1

    def state(self):
        P, s = self.D.P, np.zeros(STATE_W)
        s[S_L0], s[S_M0], s[S_LIK_B], s[S_LIK_D], s[S_PRIOR], s[S_E_B], s[S_E_D] = (self.base[0], self.base[1], self.lik[0], self.lik[1],
                                                                                 self.prior, self.E[0], self.E[1])
        s[S_PROPOSED:S_PROPOSED + MOVES], s[S_ACCEPTED:S_ACCEPTED + MOVES] = self.proposed, self.accepted
        s[S_IL:S_IL + P], s[S_A:S_A + P], s[S_IM:S_IM + P], s[S_B:S_B + P] = self.I[0], self.coef[0], self.I[1], self.coef[1]
        return s

    def row(self, it):
        P, row = self.D.P, np.zeros(ROW_W)
        tot = total(*self.lik)
        row[:8] = it, tot + self.prior, tot, self.lik[0], self.lik[1], self.prior, self.base[0], self.base[1]
        row[8:8 + P], row[8 + P:8 + 2 * P], row[8 + 2 * P:8 + 3 * P], row[8 + 3 * P:8 + 4 * P] = self.I[0], self.coef[0], self.I[1], self.coef[1]
        return row


def run(D, st, C, n_iter, s_freq, seed, chain0=0, win_at=None, full_start=False):
    """every chain -> (rows [ceil(n_iter / s_freq), C, ROW_W], state [C, STATE_W], the smallest margin).  win_at = (it, win): the
    windows change to `win` from iteration `it` on; full_start: from the initial state with every free indicator set to 1"""
    n = (n_iter + s_freq - 1) // s_freq
    rows, state, margin = np.zeros((n, C, ROW_W)), np.zeros((C, STATE_W)), np.inf
    for c in range(C):
        s = Settings(*st.astuple())
        ch, k = Chain(D, s, Stream(seed, chain0 + c)), 0
        if full_start:
            ch = ch.full()
        for it in range(n_iter):
            if win_at is not None and it == win_at[0]:
                s.win = tuple(win_at[1])
            ch.step(it)
            if it % s_freq == 0:
                rows[k, c] = ch.row(it)
                k += 1
        state[c], margin = ch.state(), min(margin, ch.margin)
    return rows, state, margin


# ---- data ----------------------------------------------------------------------------------------------------------------
def standardise(x):
    """mean 0, population sd 1"""
    x = np.asarray(x, dtype=float)
    return (x - np.mean(x)) / np.std(x)


@functools.lru_cache(maxsize=None)
def synthetic(n_bins, P, seed):
    """DT uniform on (5, 50), births and deaths Poisson at rates 0.15 and 0.1, P covariates: a shared random walk plus noise of
    their own, standardised (one bin: plain normals, the library takes X as it is)"""
    g = np.random.default_rng(seed)
    DT = g.uniform(5.0, 50.0, n_bins)
    n_spec, n_exti = g.poisson(0.15 * DT).astype(float), g.poisson(0.1 * DT).astype(float)
    if n_bins == 1:
        X = g.normal(0.0, 0.5, (P, 1))
    else:
        walk = np.cumsum(g.normal(size=n_bins))
        X = np.stack([standardise(0.5 * walk / max(np.std(walk), 1e-9) + g.normal(size=n_bins)) for _ in range(P)])
    return Data(n_spec, n_exti, DT, X)


def random_params(D, C, seed, I="mixed"):
    """l0, m0 [C]; a, b [C, P]; I_l, I_m [C, P]"""
    g = np.random.default_rng(seed)
    a, b = g.normal(0.0, 0.4, (C, D.P)), g.normal(0.0, 0.4, (C, D.P))
    if I == "zeros":
        I_l, I_m = np.zeros((C, D.P), dtype=np.int64), np.zeros((C, D.P), dtype=np.int64)
    elif I == "ones":
        I_l, I_m = np.ones((C, D.P), dtype=np.int64), np.ones((C, D.P), dtype=np.int64)
    else:
        I_l, I_m = g.integers(0, 2, (C, D.P)), g.integers(0, 2, (C, D.P))
    return g.uniform(0.05, 0.5, C), g.uniform(0.05, 0.5, C), a, I_l, b, I_m


# ---- the cases of tests/test_hip_mtrend.py -------------------------------------------------------------------------------
BIN_EDGES = [1, 63, 64, 65, 128, 129, 512]          # every instantiation (1, 2, 4, 8 bins a lane) and its edges
P_EDGES = [1, 2, 16]
N_ITER, N_CHAINS = 400, 3          # three chains: a workgroup of four waves with one idle
# name -> Settings' arguments; pI = 0.5 keeps both values of an indicator visited within 400 iterations
MODES = [("bvs", dict(bvs=1, bvs_from=50)), ("bvs_late", dict(bvs=1, bvs_from=10 ** 6)), ("nobvs", dict(bvs=0)),
         ("constB", dict(bvs=1, bvs_from=50, m_birth=1)), ("constD", dict(bvs=1, bvs_from=50, m_death=1)),
         ("nodeath", dict(bvs=1, bvs_from=50, no_death=1)), ("constBD", dict(bvs=1, bvs_from=50, m_birth=1, m_death=1))]
RESEED = {}          # case name -> a seed that keeps every decision clear of a tie (tests/test_mtrend_host.py)


def settings(mode):
    return Settings(pI=0.5, win=(0.1, 0.07), **dict(MODES)[mode])


def _cases():
    """(name, (n_bins, P, data seed), mode, n_iter, s_freq, seed, chain0).  Every n_bins edge with every P, the mode and s_freq
    cycling through them so that each mode meets every P and several instantiations; then the full cross of mode and s_freq at
    65 bins (two bins a lane, the second nearly empty) with two covariates."""
    out, i = [], 0
    for P in P_EDGES:
        for nb in BIN_EDGES:
            mode, sf = MODES[(i + i // 7) % 7][0], (1, 7)[i % 2]
            name = "b%d_P%d_%s_s%d" % (nb, P, mode, sf)
            out.append((name, (nb, P, 100 + i), mode, N_ITER, sf, RESEED.get(name, 7000 + i), i % 4))
            i += 1
    for mode, _ in MODES:
        for sf in (1, 7):
            name = "b65_P2_%s_s%d_x" % (mode, sf)
            out.append((name, (65, 2, 200 + i), mode, N_ITER, sf, RESEED.get(name, 7000 + i), 2))
            i += 1
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def run_case(case):
    """(data, settings, rows, state, margin) of a case; computed once per process and shared - leave the arrays unchanged"""
    name, key, mode, n_iter, s_freq, seed, chain0 = case
    D, st = synthetic(*key), settings(mode)
    return (D, st) + run(D, st, N_CHAINS, n_iter, s_freq, seed, chain0)


# ---- the laws of the statistical checks ----------------------------------------------------------------------------------
def constant_posterior(N_spec, sum_DT):
    """Both sides constant: the birth likelihood of l0 is l0^N exp(-l0 sum DT), the prior Gamma(1, scale 10, loc .001) adds
    exp(-l0 / 10) on l0 > .001, nothing else of the posterior involves l0 and the multiplier move with its Hastings term leaves it
    invariant.  Hence l0 | data ~ Gamma(N + 1, rate sum DT + 0.1), truncated at .001 -> (mean, variance) of the untruncated law"""
    a, b = N_spec + 1.0, sum_DT + 0.1
    return a / b, a / b ** 2


SELECTION_SEED = 4
SELECTION_SETTINGS = dict(bvs=1, bvs_from=0, pI=0.1, slab_sd=1.0, win=(0.05, 0.05), m_death=0)


@functools.lru_cache(maxsize=None)
def selection_data(seed=SELECTION_SEED):
    """40 bins, DT uniform on (80, 160); six standardised columns x_0 .. x_5 of independent normals but x_3 = 0.8 x_2 + 0.6 noise
    (correlation about 0.8); births Poisson(0.2 exp(0.6 x_2) DT_b), deaths Poisson(0.1 DT_b)"""
    g = np.random.default_rng(seed)
    nb = 40
    DT = g.uniform(80.0, 160.0, nb)
    Z = g.normal(size=(6, nb))
    Z[3] = 0.8 * standardise(Z[2]) + 0.6 * standardise(Z[3])
    X = np.stack([standardise(z) for z in Z])
    n_spec = g.poisson(0.2 * np.exp(0.6 * X[2]) * DT).astype(float)
    n_exti = g.poisson(0.1 * DT).astype(float)
    return Data(n_spec, n_exti, DT, X)


def hpd(x, level=0.95):
    """calcHPD: the shortest interval holding `level` of the sample"""
    d = np.sort(np.asarray(x, dtype=float))
    n_in = int(round(level * len(d)))
    i = int(np.argmin(d[n_in - 1:] - d[:len(d) - n_in + 1]))
    return d[i], d[i + n_in - 1]


def selection_outcome(rows, P=6):
    """rows [n, width] pooled after the burn-in -> (P(I = 1) [2, P], the 95 % HPD of a_2 given inclusion)"""
    pl, pm = rows[:, 8:8 + P].mean(axis=0), rows[:, 8 + 2 * P:8 + 3 * P].mean(axis=0)
    a2 = rows[rows[:, 8 + 2] != 0, 8 + P + 2]
    return np.stack([pl, pm]), (hpd(a2) if len(a2) >= 2 else (np.nan, np.nan))
