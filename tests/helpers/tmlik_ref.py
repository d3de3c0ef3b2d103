"""Numpy restatement of the power-posterior sampler of include/literate_hip_tmlik.h and of the window schedule of
literate_amd/trend_mlik.py: the specification the device is held to (tests/test_hip_tmlik.py) and that tests/test_tmlik_host.py
pins to what can be known exactly.

The model is trend_rate.py's as oracle/trend_mcmc_oracle.run_trend_mcmc restates it - the same likelihood and prior functions,
moves, masks, `>` rule and unconditional acceptance of iteration 0 - with three additions: chain (model m, replicate r,
temperature j) targets L^beta_j p, i.e. accepts iff beta_j (lik' - lik) + (prior' - prior) + hastings > log u (the likelihood
term left out at beta_j == 0, a NaN likelihood counted as -inf); the multiplier's log d is scaled by s_j; and the additive step's
sd is win[m, j] instead of 0.001; an additive step whose mask fires for no slope is carried out (it changes nothing) but not
counted as a proposal.  With beta = 1, s = 1 and win = 0.001 `step` is the oracle's loop body.

Two sources of randomness: oracle.trend_mcmc_oracle.PhiloxDraws (the device's addressed stream, chain key (key0[m] + r) T + j)
through `run`, one chain at a time; and a numpy Generator through `run_vec`, all chains at once and with the burn-in's window
tuning, for the long statistical runs.  The closed forms and the quadrature of the shared problem's marginal likelihoods stand at
the end.
"""
import math

import numpy as np

from oracle import literate_oracle as lo
from oracle.trend_mcmc_oracle import PhiloxDraws, update_masks

ROW_W, STATE_W = 12, 16
R_IT, R_BETA, R_LIK, R_PRIOR, R_ARGS, R_WIN, R_MODEL = 0, 1, 2, 3, 4, 10, 11
S_LIK, S_PRIOR, S_PROPOSED, S_ACCEPTED, S_BETA, S_SCALE, S_WIN, S_MODEL = 6, 7, 8, 10, 12, 13, 14, 15
WIN0, WIN_MIN, WIN_MAX, TUNE_BLOCKS = 0.001, 0.001, 20.0, 20


class Problem:
    """the statistics (create_bins' N_SPEC, N_EXTI, DT) and the normalised covariates trends [n_cols, n_bins]"""

    def __init__(self, n_spec, n_exti, DT, trends):
        self.n_spec, self.n_exti = np.asarray(n_spec, dtype=float), np.asarray(n_exti, dtype=float)
        self.DT = np.asarray(DT, dtype=float)
        self.trends = np.atleast_2d(np.asarray(trends, dtype=float))
        assert self.trends.shape[1] == len(self.DT) and (self.trends > 0).all() and (self.trends <= 1).all()

    def lik(self, args, col, const_b, const_d):
        with np.errstate(all="ignore"):
            v = np.sum(lo.trend_likelihood_function(args, self.n_spec, self.n_exti, self.DT, self.trends[col], const_b, const_d)[0])
        return -np.inf if np.isnan(v) else v


def normalise(x):
    """trendrate.normalise_trend without the dropped last bin"""
    x = np.asarray(x, dtype=float)
    t = (x - x.min()) / (x.max() - x.min())
    t[t == 0] = lo.SMALL_NUMBER
    return t


class Chain:
    def __init__(self, P, col, flags, beta, scale, win, m=0):
        self.P, self.col, self.cb, self.cd = P, int(col), bool(flags & 1), bool(flags & 2)
        self.beta, self.scale, self.win, self.m = float(beta), float(scale), float(win), int(m)
        self.um, self.un = update_masks(self.cb, self.cd)
        self.args = np.array([.1, .1, 0, 0, 1, 1], dtype=float)
        self.lik, self.prior = P.lik(self.args, self.col, self.cb, self.cd), lo.trend_calc_prior(self.args)
        self.proposed, self.accepted = [0, 0], [0, 0]
        self.margin = np.inf          # the smallest |lhs - log u| of the accept decisions made so far

    def state(self):
        return np.array(list(self.args) + [self.lik, self.prior] + self.proposed + self.accepted + [self.beta, self.scale, self.win, self.m],
                        dtype=float)

    def row(self, it):
        return np.array([it, self.beta, self.lik, self.prior] + list(self.args) + [self.win, self.m], dtype=float)


def step(ch, it, draws):
    """one iteration of one chain (trend_rate.py:163-181 with the power posterior's acceptance rule and the scaled windows)"""
    args = ch.args + 0.
    rr = draws.move(it)
    if rr < .33:
        ff, m = draws.normal_vec(it, ch.un, ch.win)
        m = np.array(m, dtype=float)
        m[ff == 0] = 0.
        args, hastings, move = args + m, 0, 1
        counted = bool(np.any(ff != 0))          # a step that fires for no slope proposes the state itself: not counted
    else:
        ff, u = draws.multiplier(it, ch.um)
        m = np.exp((ch.scale * (2 * np.log(1.1))) * (u - .5))
        m[ff == 0] = 1.
        args, hastings, move, counted = args * m, np.sum(np.log(m)), 0, True
    with np.errstate(all="ignore"):
        lik, prior = ch.P.lik(args, ch.col, ch.cb, ch.cd), lo.trend_calc_prior(args)
        dl = 0.0 if ch.beta == 0.0 else ch.beta * (lik - ch.lik)
        lhs, log_u = dl + (prior - ch.prior) + hastings, np.log(draws.accept(it))
        ok = (lhs > log_u) or it == 0
    if it != 0 and np.isfinite(lhs) and np.isfinite(log_u):
        ch.margin = min(ch.margin, abs(lhs - log_u))
    ch.proposed[move] += counted
    if ok:
        ch.args, ch.lik, ch.prior = args, lik, prior
        ch.accepted[move] += counted


def run_chain(ch, draws, n_iter, s_freq, it0=0):
    """iterations it0 .. it0 + n_iter - 1 of one chain -> rows [n, ROW_W]"""
    rows = []
    for it in range(it0, it0 + n_iter):
        step(ch, it, draws)
        if it % s_freq == 0:
            rows.append(ch.row(it))
    return np.array(rows).reshape(-1, ROW_W)


def run(P, col, flags, key0, betas, scales, wins, n_reps, n_iter, s_freq, seed):
    """every chain of the grid on the device's draws -> (rows [M, n, n_reps, T, ROW_W], state [M, n_reps, T, STATE_W], the
    smallest margin of an accept decision).  wins: [M, T] or a number."""
    M, T = len(col), len(betas)
    wins = np.broadcast_to(np.asarray(wins, dtype=float), (M, T))
    n = (n_iter + s_freq - 1) // s_freq
    rows, state, margin = np.zeros((M, n, n_reps, T, ROW_W)), np.zeros((M, n_reps, T, STATE_W)), np.inf
    for m in range(M):
        for r in range(n_reps):
            for j in range(T):
                ch = Chain(P, col[m], flags[m], betas[j], scales[j], wins[m, j], m)
                rows[m, :, r, j] = run_chain(ch, PhiloxDraws(seed, (int(key0[m]) + r) * T + j), n_iter, s_freq)
                state[m, r, j] = ch.state()
                margin = min(margin, ch.margin)
    return rows, state, margin


# ---- all chains at once on a numpy Generator, with the window schedule ---------------------------------------------------
def lik_vec(P, args, t, cb, cd):
    """the likelihood for args [C, 6], covariates t [C, n_bins], flags cb, cd [C] -> [C]"""
    l_min, m_min, alpha, beta, delta, gamma = [args[:, i, None] for i in range(6)]
    with np.errstate(all="ignore"):
        birth = l_min + alpha * t ** delta
        birth = np.where(birth <= 0, lo.SMALL_NUMBER, birth)
        birth = np.where(cb[:, None], l_min + 0 * t, birth)
        death = m_min + beta * t ** gamma
        death = np.where(death <= 0, lo.SMALL_NUMBER, death)
        death = np.where(cd[:, None], m_min + 0 * t, death)
        v = np.sum(np.log(birth) * P.n_spec - birth * P.DT, axis=1) + np.sum(np.log(death) * P.n_exti - death * P.DT, axis=1)
    return np.where(np.isnan(v), -np.inf, v)


def prior_vec(args):
    with np.errstate(all="ignore"):
        def g1(x):
            y = (x - .001) / 10.0
            return np.where(y < 0, -np.inf, -y - np.log(10.0))

        def nrm(x):
            return -0.5 * (x / 5.0) ** 2 - 0.5 * np.log(2 * np.pi) - np.log(5.0)

        def g3(x):
            y = x / .5
            return np.where(y <= 0, -np.inf, 2.0 * np.log(np.where(y > 0, y, 1.0)) - y - math.lgamma(3) - np.log(.5))

        return g1(args[:, 0]) + g1(args[:, 1]) + nrm(args[:, 2]) + nrm(args[:, 3]) + g3(args[:, 4]) + g3(args[:, 5])


def tune_blocks(burn_iters):
    return [(int(burn_iters) * b) // TUNE_BLOCKS for b in range(TUNE_BLOCKS + 1)]


def run_vec(P, col, flags, betas, scales, n_reps, n_iter, s_freq, burnin, rng):
    """the same sampler, every chain of [M, n_reps, T] advanced together on rng's draws, the additive window tuned during the
    burn-in by trend_mlik's rule: after block b = 1 .. 20 of the burn-in iterations, per (model, temperature),
    win <- clip(win exp(4 (rate - 0.3) / sqrt(b)), 0.001, 20) with rate = accepted / proposed of the additive move in that block
    over the replicates; a model with both flags is never tuned -> (rows [M, n, n_reps, T, ROW_W], wins [M, T], accepted /
    proposed after the burn-in per move kind [M, T, 2], row0: the first row after the burn-in)"""
    M, T, R = len(col), len(betas), n_reps
    C = M * R * T
    shape = (M, R, T)
    grid = lambda x, axis: np.broadcast_to(np.asarray(x).reshape([-1 if a == axis else 1 for a in range(3)]), shape).reshape(C)
    beta, s = grid(np.asarray(betas, dtype=float), 2), grid(np.asarray(scales, dtype=float), 2)
    flags = np.asarray(flags)
    cb, cd = grid((flags & 1) > 0, 0), grid((flags & 2) > 0, 0)
    t = P.trends[np.asarray(col)][:, None, None, :] + np.zeros(shape + (1,))
    t = t.reshape(C, -1)
    masks = [update_masks(bool(f & 1), bool(f & 2)) for f in flags]
    um = np.array([k[0] for k in masks])[:, None, None, :] + np.zeros(shape + (1,))
    un = np.array([k[1] for k in masks])[:, None, None, :] + np.zeros(shape + (1,))
    um, un = um.reshape(C, 6), un.reshape(C, 6)
    tunable = flags != 3
    wins = np.full((M, T), WIN0)
    args = np.tile(np.array([.1, .1, 0, 0, 1, 1], dtype=float), (C, 1))
    lik, prior = lik_vec(P, args, t, cb, cd), prior_vec(args)
    prop, acc = np.zeros((C, 2)), np.zeros((C, 2))
    n = (n_iter + s_freq - 1) // s_freq
    burn = int(burnin * n)
    ends = tune_blocks(burn * s_freq)
    rows = np.zeros((n, C, ROW_W))
    block = 1
    model = grid(np.arange(M), 0).astype(float)

    def pooled(x):
        return x.reshape(M, R, T, 2).sum(axis=1)
    for it in range(n_iter):
        while block <= TUNE_BLOCKS and it == ends[block]:
            if ends[block] > ends[block - 1]:
                a, p = pooled(acc)[:, :, 1], pooled(prop)[:, :, 1]
                with np.errstate(all="ignore"):
                    new = np.clip(wins * np.exp(4.0 * (a / p - 0.3) / math.sqrt(block)), WIN_MIN, WIN_MAX)
                wins = np.where((p > 0) & tunable[:, None], new, wins)
                prop[:], acc[:] = 0, 0
            block += 1
        w = (wins[:, None, :] + np.zeros(shape)).reshape(C)
        add = rng.random(C) < .33
        u_acc, ub, u, z = rng.random(C), rng.random((C, 6)), rng.random((C, 6)), rng.standard_normal((C, 6))
        with np.errstate(all="ignore"):
            m = np.where(ub < um, np.exp((s[:, None] * (2 * np.log(1.1))) * (u - .5)), 1.0)
            step_add = np.where(ub < un, z * w[:, None], 0.0)
        new = np.where(add[:, None], args + step_add, args * m)
        hastings = np.where(add, 0.0, np.sum(np.log(m), axis=1))
        lik_n, prior_n = lik_vec(P, new, t, cb, cd), prior_vec(new)
        with np.errstate(all="ignore"):
            dl = np.where(beta == 0.0, 0.0, beta * (lik_n - lik))
            ok = (dl + (prior_n - prior) + hastings > np.log(u_acc)) | (it == 0)
        k = add.astype(int)
        with np.errstate(all="ignore"):
            counted = ~add | np.any(ub < un, axis=1)          # (an additive step that fires for no slope is not counted)
        prop[np.arange(C), k] += counted
        acc[np.arange(C), k] += ok & counted
        args, lik, prior = np.where(ok[:, None], new, args), np.where(ok, lik_n, lik), np.where(ok, prior_n, prior)
        if it % s_freq == 0:
            q = rows[it // s_freq]
            q[:, R_IT], q[:, R_BETA], q[:, R_LIK], q[:, R_PRIOR], q[:, R_ARGS:R_ARGS + 6], q[:, R_WIN], q[:, R_MODEL] = \
                it, beta, lik, prior, args, w, model
    with np.errstate(all="ignore"):
        rate = pooled(acc) / pooled(prop)
    return rows.reshape(n, M, R, T, ROW_W).transpose(1, 0, 2, 3, 4), wins, rate, burn


# ---- the shared problem of tests/test_tmlik_host.py (b) and tests/test_hip_tmlik.py (6), (7) ---------------------------------
DT = [40., 50., 60., 70., 80.]
BIRTHS, DEATHS = [4, 8, 12, 20, 28], [5, 5, 5, 5, 5]
COVARIATE = [0, .25, .5, .8, 1]
MODELS = [(0, True, True), (0, False, True), (0, False, False)]          # CONB_COND, EXPB_COND, EXPB_EXPD: (column, const_B, const_D)
T, R, N_IT, S_FREQ, BURN, ALPHA, WIDEN, SEED = 16, 16, 20000, 10, 0.3, 0.3, 8.0, 20261020
# sd of the per-replicate stepping-stone values over the 16 replicates of run_vec on these settings, per model of MODELS
# (tests/test_tmlik_host.py (b) measures them again and holds them to these)
REF_SD = (0.2027, 0.3515, 0.3779)


def shared_problem():
    return Problem(BIRTHS, DEATHS, DT, normalise(COVARIATE))


def temperatures(T, alpha):
    return (np.arange(T) / (T - 1.0)) ** (1.0 / alpha)


def window_scales(betas, widen):
    with np.errstate(divide="ignore"):
        return np.minimum(np.asarray(betas, dtype=float) ** -0.5, float(widen))


# ---- the marginal likelihoods: log Z = (birth half) + (death half) ----------------------------------------------------------
def const_half(N, S):
    """log int_{.001}^inf r^N exp(-r S) Gamma(1, scale 10, loc .001)(r) dr: a constant rate with N events in lineage-time S"""
    from scipy.special import gammaincc
    a = S + .1
    return math.log(.1) + 1e-4 + math.lgamma(N + 1) + math.log(gammaincc(N + 1, .001 * a)) - (N + 1) * math.log(a)


def exp_half(N, DT, t, n=121):
    """log int lik x prior over (floor in [.001, 1.2], slope in [-1.5, 2.5], exponent in (0, 12]) of the half whose rate is
    floor + slope t ** exponent (floored to 1e-15 where <= 0): trapezoid rule on an n^3 grid, a slice of the floor at a time"""
    N, DT, t = [np.asarray(x, dtype=float) for x in (N, DT, t)]
    lm, sl, ex = np.linspace(.001, 1.2, n), np.linspace(-1.5, 2.5, n), np.linspace(0.0, 12.0, n)

    def weights(x):
        w = np.full(len(x), x[1] - x[0])
        w[0] = w[-1] = (x[1] - x[0]) / 2
        return w
    with np.errstate(all="ignore"):
        p_sl = -0.5 * (sl / 5.0) ** 2 - 0.5 * math.log(2 * math.pi) - math.log(5.0)
        y = ex / .5
        p_ex = np.where(y > 0, 2.0 * np.log(np.where(y > 0, y, 1.0)) - y - math.lgamma(3) - math.log(.5), -np.inf)
        te = t[None, :] ** ex[:, None]                                   # [exponent, bin]
        curve = sl[:, None, None] * te[None]                             # [slope, exponent, bin]
        lw = np.log(weights(sl))[:, None] + np.log(weights(ex))[None] + p_sl[:, None] + p_ex[None]
        parts = []
        for a, wa in zip(lm, weights(lm)):
            rate = a + curve
            rate = np.where(rate <= 0, lo.SMALL_NUMBER, rate)
            ll = np.sum(np.log(rate) * N - rate * DT, axis=2)
            parts.append(np.logaddexp.reduce((ll + lw).ravel()) + math.log(wa) - (a - .001) / 10.0 - math.log(10.0))
        return float(np.logaddexp.reduce(np.array(parts)))


def shared_truth(n=121):
    """log Z of MODELS on the shared problem"""
    P = shared_problem()
    S = float(np.sum(P.DT))
    bc, dc = const_half(int(np.sum(P.n_spec)), S), const_half(int(np.sum(P.n_exti)), S)
    be = exp_half(P.n_spec, P.DT, P.trends[0], n)
    de = exp_half(P.n_exti, P.DT, P.trends[0], n)
    halves = dict(birth_const=bc, death_const=dc, birth_exp=be, death_exp=de)
    return [(bc if b else be) + (dc if d else de) for _, b, d in MODELS], halves
