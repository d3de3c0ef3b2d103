"""Numpy restatement of the parametric samplers on replicate data sets (include/literate_hip_parbin.h): the specification the
device is held to (tests/test_hip_parbin.py) and that tests/test_parbin_host.py pins to the oracle exactly.

Chain c runs oracle/dd_mcmc_oracle.run_dd_mcmc's (sampler 1) or oracle/trend_mcmc_oracle.run_trend_mcmc's (sampler 2) loop on
the statistics of replicate c // chains_per_rep with PhiloxDraws(seed, chain0 + c): the same likelihood and prior functions,
moves, masks, `>` rule and unconditional acceptance of iteration 0, a NaN likelihood counted as -inf.  Every accept decision's
margin |lhs - log u| is recorded (iteration 0 and non-finite sides apart): where none is within TIE of zero, a device that
agrees to 1e-9 takes the same decisions.  Rows have the engines' trace layout: [it, posterior, likelihood, prior, args], then
zeros up to TRACE_W.

The cases of tests/test_hip_parbin.py stand here too (CASES_*), so the host test can hold every one of them to the tie
condition without a GPU.
"""
import functools

import numpy as np

from oracle import dd_mcmc_oracle as ddo
from oracle import literate_oracle as lo
from oracle import trend_mcmc_oracle as tro

TRACE_W, STATE_W = 13 + 2 * 63, 16
S_LIK, S_PRIOR, S_PROPOSED, S_ACCEPTED = 8, 9, 10, 12
NPAR = {1: 8, 2: 6}
TIE = 1e-6
DD_MODELS = [(mb, md) for mb in (0, 1, 2) for md in (-2, -1, 0, 1, 2)]
TREND_MODELS = [(0, 0), (1, 0), (0, 1), (1, 1)]


class Data:
    """per-replicate statistics n_spec, n_exti, DT [R, n_bins], origin, present [R] and the shared covariate trend [n_bins]"""

    def __init__(self, n_spec, n_exti, DT, origin, present, trend=None):
        self.n_spec, self.n_exti, self.DT = [np.atleast_2d(np.asarray(x, dtype=float)) for x in (n_spec, n_exti, DT)]
        self.origin, self.present = np.atleast_1d(np.asarray(origin, dtype=float)), np.atleast_1d(np.asarray(present, dtype=float))
        self.trend = None if trend is None else np.asarray(trend, dtype=float)
        self.R, self.n_bins = self.DT.shape

    def take(self, reps):
        reps = list(reps)
        return Data(self.n_spec[reps], self.n_exti[reps], self.DT[reps], self.origin[reps], self.present[reps], self.trend)


def synthetic(R, n_bins, seed):
    """uniform DT in (50, 400) with Poisson counts, origin / present differing per replicate, a covariate in (0, 1]"""
    g = np.random.default_rng(seed)
    DT = g.uniform(50.0, 400.0, (R, n_bins))
    n_spec = g.poisson(0.12 * DT).astype(float)
    n_exti = g.poisson(0.07 * DT).astype(float)
    origin = 3.0 + 1.5 * np.arange(R) + g.uniform(0.0, 1.0, R)
    present = origin + n_bins
    trend = g.uniform(0.05, 1.0, n_bins)
    trend[g.integers(n_bins)] = lo.SMALL_NUMBER if n_bins > 1 else trend[0]
    return Data(n_spec, n_exti, DT, origin, present, trend)


def _nan_to_ninf(v):
    return -np.inf if np.isnan(v) else v


class Chain:
    def __init__(self, D, r, sampler, m_birth, m_death, init_death=0.1):
        self.sampler, self.mb, self.md = int(sampler), int(m_birth), int(m_death)
        self.ns, self.ne, self.dt = D.n_spec[r], D.n_exti[r], D.DT[r]
        self.origin, self.present, self.trend = float(D.origin[r]), float(D.present[r]), D.trend
        self.x = np.arange(D.n_bins).astype(float)          # bin b at x = b
        self.k0 = np.max(self.dt)
        if self.sampler == 1:
            self.um = ddo.update_multiplier_mask(self.mb, self.md)
            self.args = ddo.initial_args(self.origin, self.present, init_death)
        else:
            self.um, self.un = tro.update_masks(bool(self.mb), bool(self.md))
            self.args = np.array([.1, .1, 0, 0, 1, 1], dtype=float)
        self.lik, self.prior = self.lik_of(self.args), self.prior_of(self.args)
        self.proposed, self.accepted = [0, 0], [0, 0]
        self.margin = np.inf

    def lik_of(self, a):
        with np.errstate(all="ignore"):
            if self.sampler == 1:
                v = np.sum(lo.dd_likelihood_function(a, self.ns, self.ne, self.dt, self.x, self.mb, self.md)[0])
            else:
                v = np.sum(lo.trend_likelihood_function(a, self.ns, self.ne, self.dt, self.trend, bool(self.mb), bool(self.md))[0])
        return _nan_to_ninf(v)

    def prior_of(self, a):
        with np.errstate(all="ignore"):
            return lo.dd_calc_prior(a, self.k0, self.origin, self.present) if self.sampler == 1 else lo.trend_calc_prior(a)

    def state(self):
        s = np.zeros(STATE_W)
        s[:len(self.args)] = self.args
        s[S_LIK], s[S_PRIOR] = self.lik, self.prior
        s[S_PROPOSED:S_PROPOSED + 2], s[S_ACCEPTED:S_ACCEPTED + 2] = self.proposed, self.accepted
        return s

    def row(self, it):
        row = np.zeros(TRACE_W)
        row[:4] = it, self.lik + self.prior, self.lik, self.prior
        row[4:4 + len(self.args)] = self.args
        return row


def step(ch, it, draws):
    """one iteration: DD:195-217 (sampler 1) or trend_rate.py:163-181 (sampler 2), as the oracles state them"""
    args = ch.args + 0.
    counted = True
    if ch.sampler == 1:
        hastings = 0
        rr0, rr1 = draws.move(it)
        if rr1 < 0.1 and (ch.mb == 2 or ch.md == 2):
            res = ch.args + 0
            ii = res[2] + (draws.slide(it) - .5) * 1.5
            if ii > ch.present:
                ii = ch.present - (ii - ch.present)
            res[2] = abs(ii)
            if ch.md == -1:
                res[1] = res[1] + draws.normal(it, 0.2)
            args, hastings, move = res, 0, 1
        else:
            ff, u = draws.multiplier(it, ch.um)
            m = np.exp(2 * np.log(1.1) * (u - .5))
            m[ff == 0] = 1.
            args, hastings, move = args * m, np.sum(np.log(m)), 0
    else:
        rr = draws.move(it)
        if rr < .33:
            ff, m = draws.normal_vec(it, ch.un, .001)
            m = np.array(m, dtype=float)
            m[ff == 0] = 0.
            args, hastings, move = args + m, 0, 1
            counted = bool(np.any(ff != 0))          # an empty mask proposes the state itself: not counted
        else:
            ff, u = draws.multiplier(it, ch.um)
            m = np.exp(2 * np.log(1.1) * (u - .5))
            m[ff == 0] = 1.
            args, hastings, move = args * m, np.sum(np.log(m)), 0
    with np.errstate(all="ignore"):
        lik, prior = ch.lik_of(args), ch.prior_of(args)
        lhs, log_u = (lik - ch.lik) + (prior - ch.prior) + hastings, np.log(draws.accept(it))
        ok = (lhs > log_u) or it == 0
    if it != 0 and np.isfinite(lhs) and np.isfinite(log_u):
        ch.margin = min(ch.margin, abs(lhs - log_u))
    ch.proposed[move] += counted
    if ok:
        ch.args, ch.lik, ch.prior = args, lik, prior
        ch.accepted[move] += counted


def draws_of(sampler, seed, key):
    return (ddo if sampler == 1 else tro).PhiloxDraws(seed, key)


def run(D, sampler, m_birth, m_death, chains_per_rep, n_iter, s_freq, seed, chain0=0, init_death=0.1):
    """every chain -> (rows [ceil(n_iter / s_freq), C, TRACE_W], state [C, STATE_W], the smallest margin)"""
    C = D.R * chains_per_rep
    n = (n_iter + s_freq - 1) // s_freq
    rows, state, margin = np.zeros((n, C, TRACE_W)), np.zeros((C, STATE_W)), np.inf
    for c in range(C):
        ch = Chain(D, c // chains_per_rep, sampler, m_birth, m_death, init_death)
        draws, k = draws_of(sampler, seed, chain0 + c), 0
        for it in range(n_iter):
            step(ch, it, draws)
            if it % s_freq == 0:
                rows[k, c] = ch.row(it)
                k += 1
        state[c], margin = ch.state(), min(margin, ch.margin)
    return rows, state, margin


# ---- the cases of tests/test_hip_parbin.py ------------------------------------------------------------------------------
# (name, data (R, n_bins, data seed), sampler, m_birth, m_death, chains_per_rep, n_iter, s_freq, seed, chain0)
def _models():
    return [(1, mb, md) for mb, md in DD_MODELS] + [(2, cb, cd) for cb, cd in TREND_MODELS]


CASES_MODELS = [("model_s%d_%d_%d" % (s, a, b), (3, 12, 11), s, a, b, 2, 600, 7, 4100 + i, 5) for i, (s, a, b) in enumerate(_models())]
BIN_EDGES = [1, 2, 63, 64, 65, 128, 129, 256, 257, 511, 512]
CASES_BINS = [("bins%d_s%d_cpr%d" % (nb, s, cpr), (2, nb, 20 + nb), s, 2 if s == 1 else 0, 2 if s == 1 else 0, cpr, 200, 7,
               5200 + 3 * i + 2 * s + cpr, 1)
              for i, nb in enumerate(BIN_EDGES) for s in (1, 2) for cpr in (1, 3)]
CHAIN_EDGES = [1, 3, 4, 5, 8, 9]
CASES_CHAINS = [("chains_R%d_cpr%d_s%d" % (R, C // R, s), (R, 9, 70 + C), s, 2 if s == 1 else 0, 2 if s == 1 else 0, C // R, 150, 5,
                 6300 + 10 * C + s + R, 0)
                for C in CHAIN_EDGES for R in sorted({C, 1}) for s in (1, 2)]
CASES = CASES_MODELS + CASES_BINS + CASES_CHAINS


@functools.lru_cache(maxsize=None)
def case_data(key):
    return synthetic(*key)


@functools.lru_cache(maxsize=None)
def run_case(case):
    """(data, rows, state, margin) of a case; computed once per process and shared - leave the arrays unchanged"""
    name, key, sampler, mb, md, cpr, n_iter, s_freq, seed, chain0 = case
    D = case_data(key)
    return (D,) + run(D, sampler, mb, md, cpr, n_iter, s_freq, seed, chain0)


# ---- lineages: the data of the comparison with the lineage engines ------------------------------------------------------
LINEAGE_SEEDS = {1: 7301, 2: 7302}          # sampler -> the seed of that comparison (held to the tie condition by the host test)
LINEAGE_ITERS, LINEAGE_CPR = 400, 2


def lineage_replicates(n=300, span=13, seed=3, R=2):
    """[(ts, te, PRESENT, ORIGIN)] per replicate, as parse_ts_te returns them: one set of birth years (sorted), the death
    years resampled per replicate, te with the jitter 0.5; 12 time bins"""
    g = np.random.default_rng(seed)
    ts = np.sort(g.integers(0, span - 1, n)).astype(float)
    ts[0] = 0.0
    out = []
    for r in range(R):
        te = np.minimum(ts + g.integers(0, 8, n), span - 1).astype(float)
        te[-1] = span - 1
        te = te + 0.5
        out.append((ts, te, float(te.max()), float(ts.min())))
    return out


@functools.lru_cache(maxsize=None)
def lineage_data():
    """the replicates of lineage_replicates() binned by the oracle's create_bins, with a covariate -> Data"""
    rows = [lo.create_bins(origin, present, ts, te, 0) for ts, te, present, origin in lineage_replicates()]
    nb = rows[0][5]
    trend = np.random.default_rng(17).uniform(0.05, 1.0, nb)
    return Data([r[2] for r in rows], [r[3] for r in rows], [r[4] for r in rows], [r[0] for r in rows], [r[1] for r in rows], trend)


@functools.lru_cache(maxsize=None)
def run_lineage_case(sampler):
    D = lineage_data()
    mb, md = (2, 2) if sampler == 1 else (0, 0)
    return (D,) + run(D, sampler, mb, md, LINEAGE_CPR, LINEAGE_ITERS, 1, LINEAGE_SEEDS[sampler], 0)


# ---- the closed form of the statistical check ---------------------------------------------------------------------------
def constant_rate_posterior_mean(n_events, total_time):
    """DDRate model (0, 0): lam_b = l_max in every bin, so the likelihood of l_max is l^N exp(-l T), N = sum n_spec, T = sum DT;
    dd_calc_prior puts Gamma(shape 1, scale 10) on l_max (and on m_max), density ~ exp(-l / 10), independent of the other
    parameters, whose terms do not involve l_max; the multiplier move with its Hastings ratio leaves that posterior
    invariant on l > 0.  The posterior of l_max is therefore ~ l^N exp(-l (T + 1 / 10)): Gamma(N + 1, rate T + 0.1), with
    mean (N + 1) / (T + 0.1)."""
    return (n_events + 1.0) / (total_time + 0.1)
