"""Numpy restatement of the power-posterior sampler and the marginal-likelihood estimators of include/literate_hip_mlik.h: the
specification the device is held to (tests/test_hip_mlik.py) and that tests/test_mlik_host.py pins to what can be known exactly.

The model is DDRate.py's as oracle/dd_mcmc_oracle.run_dd_mcmc restates it - the same likelihood and prior functions, the same
moves, masks, `>` rule and unconditional acceptance of iteration 0 - with two additions: chain (replicate r, temperature j)
targets L^beta_j p, i.e. accepts iff beta_j (lik' - lik) + (prior' - prior) + hastings > log u (the likelihood term left out at
beta_j == 0, a NaN likelihood counted as -inf), and its windows are scaled by s_j: the multiplier's log d, the 1.5 of the
midpoint's sliding window and the 0.2 of the normal step on k.  With beta = 1 and s = 1 `step` is the oracle's loop body.

Two sources of randomness: oracle.dd_mcmc_oracle.PhiloxDraws (the device's addressed stream, chain key (rep0 + r) T + j) through
`run`, one chain at a time; and a numpy Generator through `run_vec`, all chains at once, for the long statistical runs.
"""
import numpy as np

from oracle import literate_oracle as lo
from oracle.dd_mcmc_oracle import PhiloxDraws, initial_args, update_multiplier_mask

ROW_W, STATE_W = 12, 16
R_IT, R_BETA, R_LIK, R_PRIOR, R_ARGS = 0, 1, 2, 3, 4
MODELS = [(mb, md) for mb in (0, 1, 2) for md in (-2, -1, 0, 1, 2)]


class Model:
    """the statistics (create_bins' N_SPEC, N_EXTI, DT), the window and the model flags of one run"""

    def __init__(self, n_spec, n_exti, DT, origin, present, m_birth=2, m_death=2, init_death=0.1):
        self.n_spec, self.n_exti = np.asarray(n_spec, dtype=float), np.asarray(n_exti, dtype=float)
        self.DT = np.asarray(DT, dtype=float)
        self.time_range = np.arange(len(self.DT)).astype(float)
        self.origin, self.present, self.init_death = float(origin), float(present), float(init_death)
        self.m_birth, self.m_death = int(m_birth), int(m_death)
        self.k0 = np.max(self.DT)
        self.um = update_multiplier_mask(self.m_birth, self.m_death)

    def lik(self, args):
        with np.errstate(all="ignore"):
            v = np.sum(lo.dd_likelihood_function(args, self.n_spec, self.n_exti, self.DT, self.time_range, self.m_birth,
                                                 self.m_death)[0])
        return -np.inf if np.isnan(v) else v

    def prior(self, args):
        return lo.dd_calc_prior(args, self.k0, self.origin, self.present)


def temperatures(T, alpha):
    """beta_j = (j / (T - 1)) ** (1 / alpha)"""
    return (np.arange(T) / (T - 1.0)) ** (1.0 / alpha)


def window_scales(betas, widen):
    """s_j = min(beta_j ** -1/2, widen)"""
    with np.errstate(divide="ignore"):
        return np.minimum(np.asarray(betas, dtype=float) ** -0.5, float(widen))


class Chain:
    def __init__(self, M, beta, scale):
        self.M, self.beta, self.scale = M, float(beta), float(scale)
        self.args = initial_args(M.origin, M.present, M.init_death)
        self.lik, self.prior = M.lik(self.args), M.prior(self.args)
        self.proposed, self.accepted = [0, 0], [0, 0]

    def state(self):
        return np.array(list(self.args) + [self.lik, self.prior] + self.proposed + self.accepted + [self.beta, self.scale], dtype=float)

    def row(self, it):
        return np.array([it, self.beta, self.lik, self.prior] + list(self.args), dtype=float)


def step(ch, it, draws):
    """one iteration of one chain (DD:195-217 with the power posterior's acceptance rule and the scaled windows)"""
    M, s = ch.M, ch.scale
    args = ch.args + 0.
    hastings = 0
    rr0, rr1 = draws.move(it)
    if rr1 < 0.1 and (M.m_birth == 2 or M.m_death == 2):
        res = ch.args + 0
        ii = res[2] + (draws.slide(it) - .5) * (1.5 * s)
        if ii > M.present:
            ii = M.present - (ii - M.present)
        res[2] = abs(ii)
        if M.m_death == -1:
            res[1] = res[1] + draws.normal(it, 0.2 * s)
        args, hastings, move = res, 0, 1
    else:
        ff, u = draws.multiplier(it, M.um)
        m = np.exp((s * (2 * np.log(1.1))) * (u - .5))
        m[ff == 0] = 1.
        args = args * m
        hastings = np.sum(np.log(m))
        move = 0
    with np.errstate(all="ignore"):
        lik, prior = M.lik(args), M.prior(args)
        dl = 0.0 if ch.beta == 0.0 else ch.beta * (lik - ch.lik)
        ok = (dl + (prior - ch.prior) + hastings > np.log(draws.accept(it))) or it == 0
    ch.proposed[move] += 1
    if ok:
        ch.args, ch.lik, ch.prior = args, lik, prior
        ch.accepted[move] += 1


def run_chain(M, beta, scale, draws, n_iter, s_freq, it0=0, chain=None):
    """iterations it0 .. it0 + n_iter - 1 of one chain -> (rows [n, ROW_W], the chain)"""
    ch = Chain(M, beta, scale) if chain is None else chain
    rows = []
    for it in range(it0, it0 + n_iter):
        step(ch, it, draws)
        if it % s_freq == 0:
            rows.append(ch.row(it))
    return np.array(rows).reshape(-1, ROW_W), ch


def run(M, betas, scales, n_reps, n_iter, s_freq, seed, rep0=0):
    """every chain on the device's draws -> (rows [n, n_reps, T, ROW_W], state [n_reps, T, STATE_W])"""
    T = len(betas)
    n = (n_iter + s_freq - 1) // s_freq
    rows, state = np.zeros((n, n_reps, T, ROW_W)), np.zeros((n_reps, T, STATE_W))
    for r in range(n_reps):
        for j in range(T):
            rows[:, r, j], ch = run_chain(M, betas[j], scales[j], PhiloxDraws(seed, (rep0 + r) * T + j), n_iter, s_freq)
            state[r, j] = ch.state()
    return rows, state


# ---- all chains at once on a numpy Generator ---------------------------------------------------------------------------
def lik_vec(M, args):
    """Model.lik for args [C, 8] -> [C]"""
    a = [args[:, i, None] for i in range(8)]
    l_max, k, x0, div_0, L, m_max, nuB, nuD = a
    DT, x = M.DT[None], M.time_range[None]
    ones = np.ones((len(args), len(M.DT)))

    def niche_of(m):
        return ones * (L + div_0) if m == 1 else div_0 + L / ((1 + np.exp(-k * (x - x0))) ** (1 / 1))

    def floor_rates(r):
        r = r.copy()
        r[r <= 0] = lo.SMALL_NUMBER
        return r

    with np.errstate(all="ignore"):
        birth = ones * l_max if M.m_birth == 0 else floor_rates(l_max - l_max * ((DT / niche_of(M.m_birth)) ** nuB))
        death = ones * m_max if M.m_death <= 0 else floor_rates(m_max + m_max * ((DT / niche_of(M.m_death)) ** nuD))
        v = np.sum(np.log(birth) * M.n_spec - birth * DT, axis=1) + np.sum(np.log(death) * M.n_exti - death * DT, axis=1)
    return np.where(np.isnan(v), -np.inf, v)


def prior_vec(M, args):
    def g1(x, scale):
        with np.errstate(all="ignore"):
            return np.where(x < 0, -np.inf, -x / scale - np.log(scale))

    def nrm(x):
        return -0.5 * x * x - 0.5 * np.log(2 * np.pi)

    p = g1(args[:, 0], 10) + nrm(args[:, 1]) + g1(args[:, 5], 10) + g1(args[:, 3], M.k0) + g1(args[:, 4], M.k0) + nrm(args[:, 6]) \
        + nrm(args[:, 7])
    return np.where(M.origin + args[:, 2] >= M.present, -np.inf, p)


def run_vec(M, betas, scales, n_reps, n_iter, s_freq, rng):
    """the same sampler, every chain of [n_reps, T] advanced together on rng's draws -> (rows [n, n_reps, T, ROW_W],
    accepted / proposed per move kind [n_reps, T, 2])"""
    T = len(betas)
    C = n_reps * T
    beta, s = np.tile(np.asarray(betas, dtype=float), n_reps), np.tile(np.asarray(scales, dtype=float), n_reps)
    args = np.tile(initial_args(M.origin, M.present, M.init_death), (C, 1))
    lik, prior = lik_vec(M, args), prior_vec(M, args)
    niche = M.m_birth == 2 or M.m_death == 2
    prop, acc = np.zeros((C, 2)), np.zeros((C, 2))
    n = (n_iter + s_freq - 1) // s_freq
    rows = np.zeros((n, C, ROW_W))
    for it in range(n_iter):
        slide = (rng.random(C) < 0.1) & niche
        u_slide, z, u_acc = rng.random(C), rng.standard_normal(C), rng.random(C)
        ff, u = rng.random((C, 8)) < M.um[None], rng.random((C, 8))
        m = np.where(ff, np.exp((s[:, None] * (2 * np.log(1.1))) * (u - .5)), 1.0)
        mult = args * m
        res = args.copy()
        ii = res[:, 2] + (u_slide - .5) * (1.5 * s)
        ii = np.where(ii > M.present, M.present - (ii - M.present), ii)
        res[:, 2] = np.abs(ii)
        if M.m_death == -1:
            res[:, 1] = res[:, 1] + z * (0.2 * s)
        new = np.where(slide[:, None], res, mult)
        hastings = np.where(slide, 0.0, np.sum(np.log(m), axis=1))
        lik_n, prior_n = lik_vec(M, new), prior_vec(M, new)
        with np.errstate(all="ignore"):
            dl = np.where(beta == 0.0, 0.0, beta * (lik_n - lik))
            ok = (dl + (prior_n - prior) + hastings > np.log(u_acc)) | (it == 0)
        k = slide.astype(int)
        prop[np.arange(C), k] += 1
        acc[np.arange(C), k] += ok
        args, lik, prior = np.where(ok[:, None], new, args), np.where(ok, lik_n, lik), np.where(ok, prior_n, prior)
        if it % s_freq == 0:
            q = rows[it // s_freq]
            q[:, R_IT], q[:, R_BETA], q[:, R_LIK], q[:, R_PRIOR], q[:, R_ARGS:] = it, beta, lik, prior, args
    with np.errstate(all="ignore"):
        return rows.reshape(n, n_reps, T, ROW_W), (acc / prop).reshape(n_reps, T, 2)


# ---- the estimators ----------------------------------------------------------------------------------------------------
def log_mean_exp(x, d):
    """log mean exp(d x) over the 1-d array x, shifted by its maximum; -inf entries contribute 0, all -inf gives -inf"""
    x = np.asarray(x, dtype=float)
    m = np.max(x)
    if m == -np.inf:
        return -np.inf
    with np.errstate(all="ignore"):
        t = np.where(x == -np.inf, 0.0, np.exp(d * (x - m)))
    return d * m + np.log(np.sum(t) / len(x))


def estimate(rows, betas, row0=0):
    """rows [n_rows, R, T, ROW_W] -> dict(stone [R, T - 1], ss [R], lik_mean, lik_var [R, T], ti [R], pooled [T])"""
    betas = np.asarray(betas, dtype=float)
    lik = np.asarray(rows)[row0:, :, :, R_LIK]
    n, R, T = lik.shape
    d = np.diff(betas)
    stone = np.array([[log_mean_exp(lik[:, r, j], d[j]) for j in range(T - 1)] for r in range(R)]).reshape(R, T - 1)
    with np.errstate(all="ignore"):
        mean = np.mean(lik, axis=0)
        var = np.sum((lik - mean[None]) ** 2, axis=0) / (n - 1) if n > 1 else np.full((R, T), np.nan)
        ti = np.sum(d[None] * ((mean[:, :-1] + mean[:, 1:]) / 2.0), axis=1)
        pooled = np.array([log_mean_exp(lik[:, :, j].ravel(), d[j]) for j in range(T - 1)])
        return dict(stone=stone, ss=np.sum(stone, axis=1), lik_mean=mean, lik_var=var, ti=ti,
                    pooled=np.concatenate([pooled, [np.sum(pooled)]]))


# the long run of the constant-rate model that tests/test_mlik_host.py (b), (c) and tests/test_hip_mlik.py (g) share
B, D, S = 40, 25, 300.0
T, R, N_IT, S_FREQ, BURN, ALPHA, WIDEN, SEED = 16, 32, 20000, 10, 0.2, 0.3, 8.0, 20261019
REF_SD = 0.1844        # sd of ss over the 32 replicates of run_vec on these settings (test_mlik_host.py (b) holds it to that)


# ---- the constant-rate model's closed forms (m_birth = 0, m_death = 0: Exp(scale 10) priors on two rates) -------------
def const_model(B=40, D=25):
    """5 bins with B births, D deaths and sum DT = 300"""
    assert B % 5 == 0 and D % 5 == 0
    return Model([B // 5] * 5, [D // 5] * 5, [40., 50., 60., 70., 80.], 0.0, 6.0, 0, 0)


def const_log_z(B, D, S):
    from math import lgamma, log
    return 2 * log(0.1) + lgamma(B + 1) - (B + 1) * log(S + 0.1) + lgamma(D + 1) - (D + 1) * log(S + 0.1)


def const_mean_lik(beta, B, D, S):
    """E_beta[lik]: under beta the rates are Gamma(beta B + 1, rate beta S + 0.1) and Gamma(beta D + 1, rate beta S + 0.1)"""
    from scipy.special import digamma
    beta = np.asarray(beta, dtype=float)

    def half(N):
        return N * (digamma(beta * N + 1) - np.log(beta * S + .1)) - S * (beta * N + 1) / (beta * S + .1)

    return half(B) + half(D)
