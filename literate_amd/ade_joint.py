"""Age-dependent extinction, sampled jointly: the posterior of (death-rate skyline, Weibull shape) together.

--ade fits the Weibull shape k CONDITIONAL on death rates that were sampled under k = 1, and profiles a multiplier out per
(draw, shape); how much of a `P(k < 1) = 0.99` survives once the rate shifts may move with k it cannot say.  This module runs
the sampler that can (include/literate_hip_adej.h, csrc/lr_adej.hip): many independent chains over the baseline rates of a
skyline (the RJ moves, priors and hyper-priors of the death side of LiteRateForward.py), and log k under a flat prior on
[-log 8, log 8] - the range and prior of --ade's grid, so the two results can be set side by side.

Model, at the resolution of the bins (include/literate_hip_ade.h with c = 1): a birth is placed at the start of its bin; a
death is known to its bin only (interval-censored); at age a (in bins) a lineage's hazard in bin b is mu[b] k a^(k - 1).  The
baseline mu at k != 1 is NOT LiteRate's death rate: it is the hazard of a lineage of age 1 bin.  The likelihood depends on
the data only through the class table of ops.ade_classes: the cost of an iteration does not depend on the number of lineages.

1. ops.ade_classes, ops.adej_prepare: the classes and the numbers at risk, once.
2. ops.adej_run: `chains` chains, n_iter iterations, a row every s_freq.
3. int(burnin * samples) rows dropped per chain; ops.col_summary: mean and 95 % HPD of shape, log shape, K and the
   hyper-parameters; ops.ess_summary: pooled ESS and split R-hat of log shape, the likelihood and K; ops.expand_rates +
   ops.col_summary: the baseline rate per bin.
4. <stem>_ADE_joint.tsv (one row), <stem>_ADE_joint_rates.tsv (one row per bin), <stem>_ADE_joint_draws.npz (the kept shape, K,
   lik and prior per sample and chain).

Refused where --ade is refused, and with more than LR_ADEJ_MAX_BINS = 128 bins."""
import math
from collections import namedtuple

import numpy as np

from . import ade

MAX_BINS = 128                      # LR_ADEJ_MAX_BINS
MOVES = ("mult", "shape", "add", "remove", "gibbs")
FIT_INTS = ["chains", "iterations", "samples_kept", "lineages", "lineages_used", "lineages_unused", "bins", "deaths", "censored",
            "classes", "K_mode"]
FIT_FLOATS = ["shape_mean", "shape_median", "shape_hpd_low", "shape_hpd_high", "p_shape_lt_1", "log_shape_mean", "log_shape_ess",
              "log_shape_rhat", "lik_ess", "lik_rhat", "K_mean", "K_hpd_low", "K_hpd_high", "K_ess", "K_rhat", "rate_hp_mean",
              "poi_hp_mean"] + ["accept_" + m for m in MOVES]
FIT_HEAD = FIT_INTS + FIT_FLOATS
RATES_HEAD = ["bin", "rate_mean", "rate_hpd_low", "rate_hpd_high"]
DRAW_KEYS = ("shape", "K", "lik", "prior")

AdeJointResult = namedtuple("AdeJointResult", "rows state dead cens totals kept fit rates draws")
AdeJointResult.__doc__ = """run's results.  rows [samples, chains, LR_ADEJ_ROW_W], state [chains, LR_ADEJ_STATE_W]: device tensors as
ops.adej_run returns them; dead [A, A], cens [A], totals [2]: the classes (host); kept: samples per chain after burn-in;
fit: dict of <stem>_ADE_joint.tsv (FIT_HEAD); rates: per bin (bin, mean, HPD low, HPD high); draws: dict of [kept, chains]
host arrays (DRAW_KEYS)."""


def arg_error(burnin, n_iter, s_freq, win, n_bins=None, model=2, pyrate_output=False, rm_first_bin=False):
    """Why a CLI's --ade_joint BURNIN cannot run (None when it can): what --ade refuses, for the same reasons, and more
    than 128 bins."""
    if not (0.0 <= burnin < 1.0):
        return "--ade_joint takes a burn-in fraction in [0, 1)"
    if n_iter < 1:
        return "--ade_joint_n must be at least 1"
    if s_freq < 1:
        return "--ade_joint_s must be at least 1"
    if not (win > 0.0 and math.isfinite(win)):
        return "--ade_joint_win must be a positive width in log shape"
    n = (int(n_iter) + int(s_freq) - 1) // int(s_freq)
    if n - int(burnin * n) < 4:
        return "--ade_joint: %d iterations at one row per %d leave fewer than 4 samples after the burn-in" % (n_iter, s_freq)
    shared = ade.shared_refusal("--ade_joint", "run", model, pyrate_output, rm_first_bin)
    if shared is None and n_bins is not None and n_bins > MAX_BINS:
        return too_many_bins(n_bins)
    return shared


def too_many_bins(n_bins):
    return ("--ade_joint: the run has %d time bins, and the joint sampler takes at most %d (LR_ADEJ_MAX_BINS): a chain keeps "
            "the table of the numbers at risk, bins x bins / 2, in a workgroup's LDS" % (n_bins, MAX_BINS))


def bin_rates(rows, t0, n_bins):
    """the per-bin baseline rate of every row of rows [n, C, LR_ADEJ_ROW_W] (ops.expand_rates) -> [n, C, n_bins]"""
    import torch
    from . import _hip, ops
    n, C, W = rows.shape
    flat = rows.reshape(n * C, W)
    kmax, head = _hip.LR_KMAX, len(ops.ADEJ_ROW_HEAD)
    K = flat[:, ops.ADEJ_ROW_HEAD.index("K")].to(torch.int32)
    rates = torch.nan_to_num(flat[:, head:head + kmax], nan=0.0).contiguous()
    times = torch.zeros((n * C, kmax + 1), dtype=torch.float64, device=rows.device)
    times[:, 0] = float(t0)
    times[:, 1:kmax] = torch.nan_to_num(flat[:, head + kmax:head + 2 * kmax - 1], nan=0.0)
    times.scatter_(1, K.to(torch.int64)[:, None], float(t0) + float(n_bins))
    return ops.expand_rates(rates, times, K, int(n_bins), mode=0).reshape(n, C, int(n_bins))


def summarise(rows, state, t0, n_bins, n_iter, burnin, counts):
    """rows, state as ops.adej_run returns them -> (fit dict, rates list, draws dict, samples kept per chain)"""
    import torch
    from . import ops
    col = {k: i for i, k in enumerate(ops.ADEJ_ROW_HEAD)}
    n, C = int(rows.shape[0]), int(rows.shape[1])
    burn = int(burnin * n)
    cs = ops.col_summary(rows, n, [col[k] for k in ("shape", "log_shape", "K", "rate_hp", "poi_hp")], burnin=burnin, pooled=True)
    mean, lo, hi = (x[0].cpu().numpy() for x in (cs.mean, cs.lo, cs.hi))
    es = ops.ess_summary(rows, n, [col[k] for k in ("log_shape", "lik", "K")], burnin=burnin)
    ess, rhat = es.pooled_ess.cpu().numpy(), es.rhat.cpu().numpy()
    kept = rows[burn:]
    shape = kept[:, :, col["shape"]]
    Kc = kept[:, :, col["K"]]
    st = state.cpu().numpy()
    prop = st[:, ops.ADEJ_STATE["proposed"]:ops.ADEJ_STATE["proposed"] + len(MOVES)].sum(axis=0)
    acc = st[:, ops.ADEJ_STATE["accepted"]:ops.ADEJ_STATE["accepted"] + len(MOVES)].sum(axis=0)
    fit = dict(counts)
    fit.update({"chains": C, "iterations": int(n_iter), "samples_kept": n - burn, "bins": int(n_bins),
                "K_mode": int(torch.mode(Kc.reshape(-1)).values.item()),
                "shape_mean": mean[0], "shape_median": float(torch.median(shape.reshape(-1)).item()), "shape_hpd_low": lo[0],
                "shape_hpd_high": hi[0], "p_shape_lt_1": float((shape < 1.0).double().mean().item()), "log_shape_mean": mean[1],
                "log_shape_ess": ess[0], "log_shape_rhat": rhat[0], "lik_ess": ess[1], "lik_rhat": rhat[1], "K_mean": mean[2],
                "K_hpd_low": lo[2], "K_hpd_high": hi[2], "K_ess": ess[2], "K_rhat": rhat[2], "rate_hp_mean": mean[3],
                "poi_hp_mean": mean[4]})
    for i, m in enumerate(MOVES):
        fit["accept_" + m] = float(acc[i] / prop[i]) if prop[i] > 0 else float("nan")
    fit = {k: (int(fit[k]) if k in FIT_INTS else float(fit[k])) for k in FIT_HEAD}
    bins = bin_rates(kept.contiguous(), t0, n_bins)
    bs = ops.col_summary(bins, n - burn, range(int(n_bins)), burnin=0.0, pooled=True)
    bm, bl, bh = (x[0].cpu().numpy() for x in (bs.mean, bs.lo, bs.hi))
    rates = [(float(b), float(bm[b]), float(bl[b]), float(bh[b])) for b in range(int(n_bins))]
    draws = {k: kept[:, :, col[k]].cpu().numpy() for k in DRAW_KEYS}
    return fit, rates, draws, n - burn


def run(ts, te, t0, n_bins, chains, n_iter, s_freq, seed, settings=None, burnin=0.2):
    """The joint sampler on the lineages (ts, te) and the window [t0, t0 + n_bins) -> AdeJointResult."""
    from . import ops
    settings = ops.AdejSettings() if settings is None else settings
    if int(n_bins) > MAX_BINS:
        raise ValueError(too_many_bins(int(n_bins)))
    dead, cens, tot = ops.ade_classes(ts, te, t0, n_bins)
    data = ops.adej_prepare(dead, cens)
    rows, state = ops.adej_run(data, t0, chains, n_iter, s_freq, seed, settings)
    dead_h, cens_h, tot_h = dead.cpu().numpy(), cens.cpu().numpy(), tot.cpu().numpy()
    fit, rates, draws, kept = summarise(rows, state, t0, n_bins, n_iter, burnin, ade.class_counts(dead_h, cens_h, tot_h))
    return AdeJointResult(rows, state, dead_h, cens_h, tot_h, kept, fit, rates, draws)


def write_tables(stem, fit, rates, draws):
    """<stem>_ADE_joint.tsv (FIT_HEAD, one row), <stem>_ADE_joint_rates.tsv (RATES_HEAD, one row per bin),
    <stem>_ADE_joint_draws.npz (DRAW_KEYS).  Numbers as str(float), counts as integers, as ade.write_tables writes them."""
    with open(stem + "_ADE_joint.tsv", "w") as f:
        f.write("\t".join(FIT_HEAD) + "\n")
        f.write("\t".join("%d" % fit[k] if k in FIT_INTS else str(float(fit[k])) for k in FIT_HEAD) + "\n")
    with open(stem + "_ADE_joint_rates.tsv", "w") as f:
        f.write("\t".join(RATES_HEAD) + "\n")
        for r in rates:
            f.write("\t".join(str(float(v)) for v in r) + "\n")
    np.savez(stem + "_ADE_joint_draws.npz", **{k: np.asarray(draws[k]) for k in DRAW_KEYS})


def read_tables(stem):
    """what write_tables wrote -> (fit dict, rates as a list of (bin, mean, low, high), draws dict)"""
    with open(stem + "_ADE_joint.tsv") as f:
        head, vals = [l.rstrip("\n").split("\t") for l in f]
    fit = {k: int(v) if k in FIT_INTS else float(v) for k, v in zip(head, vals)}
    with open(stem + "_ADE_joint_rates.tsv") as f:
        rows = [l.rstrip("\n").split("\t") for l in f][1:]
    with np.load(stem + "_ADE_joint_draws.npz") as z:
        draws = {k: z[k] for k in DRAW_KEYS}
    return fit, [tuple(float(v) for v in r) for r in rows], draws


def _say(stem, res):
    f = res.fit
    return ("ADE joint: %s_ADE_joint.tsv, _ADE_joint_rates.tsv, _ADE_joint_draws.npz (%d chains x %d iterations, %d samples kept "
            "per chain; %d of %d lineages used, %d deaths in %d classes; Weibull shape %.4f (95 %% HPD %.4f - %.4f), "
            "P(shape < 1) %.3f, ESS of log shape %.0f, R-hat %.3f; K mean %.2f, mode %d)"
            % (stem, f["chains"], f["iterations"], f["samples_kept"], f["lineages_used"], f["lineages"], f["deaths"], f["classes"],
               f["shape_median"], f["shape_hpd_low"], f["shape_hpd_high"], f["p_shape_lt_1"], f["log_shape_ess"],
               f["log_shape_rhat"], f["K_mean"], f["K_mode"]))


def write_run(eng, total_chains, rank, burnin, n_iter, s_freq, win, seed, stem, const=0, use_rate_hp=1, poisson_prior=0.0):
    """The three CLIs' --ade_joint, after the run, on rank 0 alone: the engine's lineages and window, `total_chains` chains
    and the run's seed; the cost does not depend on the lineages, so one GPU carries every chain.  It does not read the
    run's trace.  -> the three files and one line on stdout."""
    from . import ops
    if int(eng.n_bins) > MAX_BINS:
        raise ValueError(too_many_bins(int(eng.n_bins)))
    if rank != 0:
        return None
    st = ops.AdejSettings(const=int(const), use_rate_hp=int(use_rate_hp), poisson_prior=float(poisson_prior), win=float(win))
    res = run(eng.ts, eng.te, eng.t0, int(eng.n_bins), int(total_chains), int(n_iter), int(s_freq), int(seed), st, burnin)
    write_tables(stem, res.fit, res.rates, res.draws)
    print(_say(stem, res))
    return res
