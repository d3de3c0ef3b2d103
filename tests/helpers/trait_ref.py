"""A plain numpy restatement of the trait-dependent model (include/literate_hip_trait.h): the per-lineage, per-bin double loop
for W and Slog, the likelihood, the sampler's trait move and a small sampler for the end-to-end comparison.  Nothing here
shares code with the device path."""
import math

import numpy as np

P_TRAIT_MOVE, P_TRAIT_ACCEPT = 60, 61
F = 38                          # LR_TRAIT_F
LOG_2PI = math.log(2.0 * math.pi)


def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(z, dtype=float)))


def log_sigmoid(z):
    """-softplus(-z), finite for every finite z"""
    z = np.asarray(z, dtype=float)
    return np.minimum(z, 0.0) - np.log1p(np.exp(-np.abs(z)))


def counted(ts, te, t0, n_bins):
    """(born, died): the births lr_bin_unit_events counts in sp (ts in [t0, t0 + n_bins)) and the deaths it counts in ex
    (te in (t0, t0 + n_bins])"""
    ts, te = np.asarray(ts, dtype=float), np.asarray(te, dtype=float)
    return (ts >= t0) & (ts < t0 + n_bins), (te > t0) & (te <= t0 + n_bins)


def weights_loop(ts, te, x, t0, n_bins, x0, kappa):
    """The explicit double loop: W [n_bins], Slog_birth, Slog_death and the lineages overlapping each bin"""
    W, cnt = np.zeros(n_bins), np.zeros(n_bins, dtype=np.int64)
    sb = sd = 0.0
    for i in range(len(ts)):
        z = kappa * (x[i] - x0)
        s = float(sigmoid(z))
        if t0 <= ts[i] < t0 + n_bins:
            sb += float(log_sigmoid(z))
        if t0 < te[i] <= t0 + n_bins:
            sd += float(log_sigmoid(z))
        for b in range(n_bins):
            e = min(te[i], t0 + b + 1.0) - max(ts[i], t0 + b)
            if e > 0.0:
                W[b] += s * e
                cnt[b] += 1
    return W, sb, sd, cnt


def overlaps(ts, te, t0, n_bins):
    """e [n, n_bins], the loop's overlaps at once"""
    ts, te = np.asarray(ts, dtype=float)[:, None], np.asarray(te, dtype=float)[:, None]
    lo = t0 + np.arange(n_bins, dtype=float)[None, :]
    e = np.minimum(te, lo + 1.0) - np.maximum(ts, lo)
    return np.where(e > 0.0, e, 0.0)


def weights(ts, te, x, t0, n_bins, params, e=None):
    """weights_loop for params [C, 2] at once -> W [C, n_bins], Slog_birth [C], Slog_death [C], cnt [n_bins]"""
    params = np.asarray(params, dtype=float).reshape(-1, 2)
    e = overlaps(ts, te, t0, n_bins) if e is None else e
    born, died = counted(ts, te, t0, n_bins)
    x = np.asarray(x, dtype=float)
    with np.errstate(invalid="ignore", over="ignore"):
        z = params[:, 1][:, None] * (x[None, :] - params[:, 0][:, None])
    s, ls = sigmoid(z), log_sigmoid(z)
    return s @ e, (ls * born[None, :]).sum(1), (ls * died[None, :]).sum(1), (e > 0.0).sum(0)


def baseline_lik(lam, mu, sp, ex, WL, WM):
    """the binned Keiding likelihood with the two exposures apart"""
    return float(np.sum(np.log(lam) * sp - lam * WL) + np.sum(np.log(mu) * ex - mu * WM))


def loglik(lam, mu, sp, ex, WL, WM, SlogL, SlogM):
    return baseline_lik(lam, mu, sp, ex, WL, WM) + SlogL + SlogM


def trait_prior(kappa_l, kappa_m):
    return -0.5 * kappa_l * kappa_l - 0.5 * kappa_m * kappa_m - LOG_2PI


def propose(stream, it, x0, kappa, win_x0, win_kappa):
    """the trait proposal of iteration `it` from an oracle.philox.Stream: (side, x0', kappa'); x0, kappa, windows: [birth, death]"""
    side = 0 if stream.pair(it, P_TRAIT_MOVE, 0)[0] < 0.5 else 1
    ux, uk = stream.pair(it, P_TRAIT_MOVE, 1)
    return side, x0[side] + (ux - 0.5) * win_x0[side], kappa[side] + (uk - 0.5) * win_kappa[side]


def settle(stream, it, lam, mu, sp, ex, W, slog, kappa, likA, side, x0p, kp, Wp, slog_p, x0_range):
    """the decision on a proposal whose W' and Slog' are given: (accept, delta, log u, lik')"""
    WL, WM = (Wp, W[1]) if side == 0 else (W[0], Wp)
    lik = baseline_lik(lam, mu, sp, ex, WL, WM)
    delta = (lik + slog_p) - (likA + slog[side]) + (-0.5 * kp * kp + 0.5 * kappa[side] * kappa[side])
    log_u = math.log(stream.pair(it, P_TRAIT_ACCEPT, 0)[0])
    in_range = x0_range[0] <= x0p <= x0_range[1]
    return bool(in_range and delta >= log_u), delta, log_u, lik


def simulate(n, n_bins, kappa_l, kappa_m, seed, lam=0.25, mu=0.35):
    """n lineages on [0, n_bins] with a standard normal trait: births thinned by s^L, deaths at rate mu s^M; the lineages alive
    at the end get te = n_bins + 1 (alive past the window)"""
    rng = np.random.default_rng(seed)
    ts, te, xs = [], [], []
    while len(ts) < n:
        x = rng.normal()
        if rng.random() >= 2.0 * lam * float(sigmoid(kappa_l * x)):
            continue
        s = rng.random() * n_bins
        d = s + rng.exponential(1.0 / (mu * float(sigmoid(kappa_m * x))))
        ts.append(s), te.append(d if d < n_bins else n_bins + 1.0), xs.append(x)
    return np.array(ts), np.array(te), np.array(xs)


def run_sampler(ts, te, x, t0, n_bins, n_iter, s_freq, trait_every, win_x0, win_kappa, x0_range, seed, update_fraction=0.75):
    """One chain of the sampler with constant baseline rates (const_rates: one rate per process, the multiplier moves and the
    Gibbs draws of the Gamma rates as runMCMC makes them) on numpy's generator -> rows [samples, 4] = (x0_l, kappa_l, x0_m,
    kappa_m).  The posterior it samples is the device's at const_rates = 1."""
    rng = np.random.default_rng(seed)
    e = overlaps(ts, te, t0, n_bins)
    born, died = counted(ts, te, t0, n_bins)
    sp = np.array([np.count_nonzero((ts >= t0 + b) & (ts < t0 + b + 1)) for b in range(n_bins)], dtype=float)
    ex = np.array([np.count_nonzero((te > t0 + b) & (te <= t0 + b + 1)) for b in range(n_bins)], dtype=float)
    n_sp, n_ex = sp.sum(), ex.sum()

    def side_stats(x0, k, mask):
        z = k * (x - x0)
        return float((sigmoid(z) @ e).sum()), float(log_sigmoid(z)[mask].sum())
    x0, kappa = [0.0, 0.0], [0.0, 0.0]
    (WL, SL), (WM, SM) = side_stats(0.0, 0.0, born), side_stats(0.0, 0.0, died)
    Wt, S = [WL, WM], [SL, SM]
    L, M = rng.gamma(2.0, 2.0), rng.gamma(2.0, 2.0)
    g = [1.0, 1.0]
    lik = lambda l, m, w: math.log(l) * n_sp - l * w[0] + math.log(m) * n_ex - m * w[1]
    pri = lambda l, m, gg: (2 * math.log(gg[0]) + math.log(l) - gg[0] * l) + (2 * math.log(gg[1]) + math.log(m) - gg[1] * m)
    likA, priorA = lik(L, M, Wt), pri(L, M, [2.0, 2.0])
    lm = 2.0 * math.log(1.1)
    rows = []
    for it in range(n_iter):
        if trait_every > 0 and (it + 1) % trait_every == 0:
            side = 0 if rng.random() < 0.5 else 1
            x0p = x0[side] + (rng.random() - 0.5) * win_x0[side]
            kp = kappa[side] + (rng.random() - 0.5) * win_kappa[side]
            u = rng.random()
            if x0_range[0] <= x0p <= x0_range[1]:
                Wp, Sp = side_stats(x0p, kp, born if side == 0 else died)
                w2 = [Wp, Wt[1]] if side == 0 else [Wt[0], Wp]
                l2 = lik(L, M, w2)
                if (l2 + Sp) - (likA + S[side]) - 0.5 * kp * kp + 0.5 * kappa[side] ** 2 >= math.log(u):
                    x0[side], kappa[side], Wt, S[side], likA = x0p, kp, w2, Sp, l2
        else:
            r0 = rng.random()
            u = rng.random()
            if r0 < 0.8:
                m = math.exp(lm * (rng.random() - 0.5)) if rng.random() < update_fraction else 1.0
                L2, M2 = (L * m, M) if r0 < 0.4 else (L, M * m)
                l2, p2 = lik(L2, M2, Wt), pri(L2, M2, g)
                if l2 - likA + p2 - priorA + math.log(m) >= math.log(u):
                    L, M, likA, priorA = L2, M2, l2, p2
            else:
                # the Gibbs draws of the Gamma rates (LRF:99-108); accepted as they are, with the prior under the new rates
                g = [rng.gamma(1.2 + 2.0, 1.0 / (0.1 + L)), rng.gamma(1.2 + 2.0, 1.0 / (0.1 + M))]
                priorA = pri(L, M, g)
        if it % s_freq == 0:
            rows.append([x0[0], kappa[0], x0[1], kappa[1]])
    return np.array(rows)
