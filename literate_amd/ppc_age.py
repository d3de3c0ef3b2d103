"""Lifespan check of a finished run: do lineages die at the ages the sampled death rates predict?

The three samplers share one assumption that no other post-run check tests: a lineage's chance of dying depends on the time
bin only, not on how old the lineage is.  The posterior the run holds tests it without a new model: condition on the
observed birth times, draw a death time for every lineage under every posterior draw of the per-bin death rates
(ops.ppc_age: lr_ppc_age, include/literate_hip_age.h, one inversion of the draw's cumulative hazard per pair), and set the
simulated deaths and hazard by AGE beside the observed ones.  A liability of newness shows as an observed hazard at age 0
far above the band, and as more observed deaths than predicted.

1. Draws, as --ppc chooses them (ppc.draw_indices); their per-bin death rates by the engine's own draw_rates.
2. The device counts, per age class a = 0 .. A - 1 (A = n_bins classes of width one bin; the top class also holds what is
   older): the observed dead and the censored (alive at the end of the window T_c = t0 + n_bins), and per draw the
   simulated dead and survivors.  A draw with a rate that is not finite or negative is flagged and left out.
3. Per class, over the kept draws: deaths[a]; at_risk[a] = sum_{a' >= a} (deaths + censored)[a']; hazard[a] = deaths[a] /
   at_risk[a].  Over all classes: total_deaths, mean_class_at_death = sum a d_a / sum d_a, median_survival_class = the
   smallest a with prod_{a' <= a} (1 - hazard[a']) <= 0.5, or A when there is none.  Every statistic is reported as
   (obs, mean, hpd_low, hpd_high, p_ge) by ppc._summarise (ops.col_summary on the values as doubles; p_ge = the share of
   kept draws >= the observed value).  A statistic that is undefined in the data or in any kept draw (a hazard with nobody
   at risk, a mean class without deaths) reports NaN for mean, HPD and p_ge.
4. <stem>_PPC_age.tsv (one row per class) and <stem>_PPC_age_fit.tsv (one row).

Time convention.  Age is time since birth in bins: the observed class is floor(te - ts), a lineage alive at T_c is censored
in class floor(T_c - ts), a simulated lifespan in [k, k + 1) is class k.  On year-resolution input (ts = y, te = y +
death_jitter) the observed class is the number of whole years lived: a lineage that dies in its birth year is class 0.  A
lineage is observed dead iff te <= T_c, the rule by which ex_events counts a death.  Lineages born outside [t0, T_c), or with
te <= ts, are not used (lineages_unused).

Not with -model_BDI 3: its death rates were fitted to the extinct lineages only, so the extant ones this check censors were
never in that likelihood.  -model_BDI 1 is allowed: its death process is the same."""
from collections import namedtuple

import numpy as np

STATS = ("obs", "mean", "hpd_low", "hpd_high", "p_ge")
AGE_HEAD = ["age", "at_risk_obs"] + ["%s_%s" % (k, s) for k in ("deaths", "hazard") for s in STATS]
FIT_INTS = ["draws", "draws_flagged", "lineages", "lineages_used", "lineages_unused", "classes"]
FIT_STATS = ("total_deaths", "mean_class_at_death", "median_survival_class")
FIT_HEAD = (FIT_INTS + ["%s_%s" % (k, s) for k in FIT_STATS for s in STATS]
            + ["coverage_deaths", "coverage_hazard", "hazard_classes_extreme"])

AgeResult = namedtuple("AgeResult", "draw_rows obs rep totals plan kept at_risk_obs deaths hazard overall fit")
AgeResult.__doc__ = """check_rates' results (host arrays).  draw_rows [S]: the trace rows the draws came from (None when rates were given
directly); obs [2, A], rep [S, 2, A], totals [4], plan: what ops.ppc_age returned; kept [S]: the unflagged draws;
at_risk_obs [A]; deaths, hazard [A, 5] and overall [3, 5] (FIT_STATS): the statistics as STATS; fit: dict of
<stem>_PPC_age_fit.tsv (FIT_HEAD)."""


def arg_error(burnin, n_draws, model=2, pyrate_output=False, rm_first_bin=False):
    """Why a CLI's --ppc_age BURNIN cannot run (None when it can).  LiteRateForward.py passes its -model_BDI and
    -pyrate_output, DDRate.py / trend_rate.py their -rm_first_bin."""
    if not (0.0 <= burnin < 1.0):
        return "--ppc_age takes a burn-in fraction in [0, 1)"
    if n_draws < 1:
        return "--ppc_age_draws must be at least 1"
    if pyrate_output:
        return ("--ppc_age reads the AD / TBP times of the trace; -pyrate_output flips them in the logs: not supported "
                "together")
    if rm_first_bin:
        return ("--ppc_age lets every lineage of the data die under the sampled rates; under -rm_first_bin 1 the lineages of "
                "the removed bin were born outside the window the model was fitted on: not supported together")
    if model == 3:
        return ("--ppc_age censors the extant lineages; under -model_BDI 3 the death rates were fitted to the extinct "
                "lineages only, so the extant ones were never in that likelihood: not supported together")
    return None


def class_stats(counts):
    """counts [..., 2, A] (dead, censored / survivors per class) -> the values the check summarises, as doubles:
    (deaths [..., A], at_risk [..., A], hazard [..., A] - NaN with nobody at risk -, overall [..., 3] = total deaths, mean
    class at death - NaN without deaths -, median survival class)"""
    c = np.asarray(counts, dtype=np.int64)
    A = c.shape[-1]
    d = c[..., 0, :]
    at_risk = np.flip(np.cumsum(np.flip(d + c[..., 1, :], axis=-1), axis=-1), axis=-1)
    dd, rr = d.astype(np.float64), at_risk.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        hazard = np.where(at_risk > 0, dd / rr, np.nan)
        total = d.sum(axis=-1)
        mean_class = np.where(total > 0, (d * np.arange(A)).sum(axis=-1).astype(np.float64) / total.astype(np.float64), np.nan)
    surv = np.ones(hazard.shape[:-1])
    median = np.full(hazard.shape[:-1], float(A))
    for a in range(A):                                        # (sequential products: the same doubles wherever this runs)
        surv = surv * (1.0 - hazard[..., a])
        median = np.where((median == float(A)) & (surv <= 0.5), float(a), median)
    overall = np.stack([total.astype(np.float64), mean_class, median], axis=-1)
    return dd, at_risk, hazard, overall


def summarise(obs, rep_kept, summarise_cols=None, device="cuda"):
    """obs [2, A], rep_kept [n, 2, A] (host integers) -> (at_risk_obs [A], deaths [A, 5], hazard [A, 5], overall [3, 5]).
    summarise_cols(vals [n, K] host doubles, obs [K]) -> [K, 5]: ppc._summarise on `device` by default."""
    if summarise_cols is None:
        from . import ppc
        import torch

        def summarise_cols(vals, o):
            return ppc._summarise(torch.as_tensor(vals, device=device), o)
    A = np.shape(obs)[-1]
    od, orisk, oh, oall = class_stats(obs)
    rd, _, rh, rall = class_stats(rep_kept)
    vals = np.concatenate([rd, rh, rall], axis=1)
    o = np.concatenate([od, oh, oall])
    st = np.array(summarise_cols(np.ascontiguousarray(vals), o), dtype=np.float64)
    undefined = np.isnan(o) | np.isnan(vals).any(axis=0)
    st[undefined, 1:] = np.nan
    return orisk, st[:A], st[A:2 * A], st[2 * A:]


def check_rates(ts, te, t0, mu_bins, seed, draw_rows=None):
    """The check of the module docstring on S draws of per-bin death rates mu_bins [S, n_bins] -> AgeResult.  The Philox
    counter of a pair is (position of the lineage in ts / te, draw): the result belongs to the ORDER the lineages are
    given in.  ValueError when fewer unflagged draws are left than a 95 % HPD takes (round(0.95 n) >= 2)."""
    from . import ops, ppc
    obs, rep, tot, plan = ops.ppc_age(ts, te, t0, mu_bins, seed)
    dev = rep.device                                                    # (the summary runs where the counts were made)
    obs, rep, tot = obs.cpu().numpy(), rep.cpu().numpy(), tot.cpu().numpy()
    S, _, A = rep.shape
    kept = rep[:, 0, 0] >= 0
    n_k = int(kept.sum())
    if n_k != int(tot[2]) or S - n_k != int(tot[3]):
        raise RuntimeError("lr_ppc_age: the totals (%d draws used, %d flagged) disagree with the rows (%d of %d kept)"
                           % (tot[2], tot[3], n_k, S))
    if int(round(0.95 * n_k)) < 2:
        raise ValueError("lifespan check: %d of the %d draws hold a death rate that is not finite or negative, and the %d left "
                         "are fewer than a 95 %% HPD takes (round(0.95 n) >= 2)" % (S - n_k, S, n_k))
    at_risk, deaths, hazard, overall = summarise(obs, rep[kept], device=dev)
    fit = dict(draws=S, draws_flagged=S - n_k, lineages=int(tot[0] + tot[1]), lineages_used=int(tot[0]),
               lineages_unused=int(tot[1]), classes=A)
    for name, row in zip(FIT_STATS, overall):
        for s, v in zip(STATS, row):
            fit["%s_%s" % (name, s)] = float(v)
    fit["coverage_deaths"], fit["coverage_hazard"] = ppc.coverage(deaths), ppc.coverage(hazard)
    fit["hazard_classes_extreme"] = int(np.sum((hazard[:, 4] < 0.025) | (hazard[:, 4] > 0.975)))
    idx = None if draw_rows is None else np.asarray(draw_rows, dtype=np.int64)
    return AgeResult(idx, obs, rep, tot, plan, kept, at_risk, deaths, hazard, overall, fit)


def write_tables(stem, res):
    """<stem>_PPC_age.tsv (AGE_HEAD, one row per age class) and <stem>_PPC_age_fit.tsv (FIT_HEAD, one row).  Numbers as
    str(float), counts as integers, as the other summary writers write them."""
    with open(stem + "_PPC_age.tsv", "w") as f:
        f.write("\t".join(AGE_HEAD) + "\n")
        for a in range(len(res.at_risk_obs)):
            f.write("\t".join(["%d" % a, "%d" % res.at_risk_obs[a]] + [str(float(v)) for v in res.deaths[a]]
                              + [str(float(v)) for v in res.hazard[a]]) + "\n")
    ints = set(FIT_INTS) | {"hazard_classes_extreme"}
    with open(stem + "_PPC_age_fit.tsv", "w") as f:
        f.write("\t".join(FIT_HEAD) + "\n")
        f.write("\t".join("%d" % res.fit[k] if k in ints else str(float(res.fit[k])) for k in FIT_HEAD) + "\n")


def _say(stem, res):
    f = res.fit
    return ("PPC age: %s_PPC_age.tsv, %s_PPC_age_fit.tsv (%d draws, %d flagged; %d of %d lineages used; deaths %d observed, "
            "%.1f predicted; hazard at age 0 %.4f observed, %.4f predicted, p_ge %.3f; %d of %d classes extreme)"
            % (stem, stem, f["draws"], f["draws_flagged"], f["lineages_used"], f["lineages"], f["total_deaths_obs"],
               f["total_deaths_mean"], res.hazard[0, 0], res.hazard[0, 1], res.hazard[0, 4], f["hazard_classes_extreme"],
               f["classes"]))


def write_run(eng, n_local, total_chains, world, rank, burnin, n_draws, seed, stem):
    """The three CLIs' --ppc_age, on the path of waic._run: the rows the run sampled, int(burnin * S) dropped per chain,
    gathered to rank 0; there n_draws of them chosen as --ppc chooses them, their per-bin death rates by the engine's own
    draw_rates, and check_rates on the engine's lineages and window (eng.ts, eng.te, eng.t0, eng.n_bins) -> the two files
    and one line on stdout.  The lineage index of the Philox counter is the ENGINE'S order of the lineages (eng.ts), not
    the data file's."""
    from . import ppc
    from ._hip import LR_TRACE_W
    rows = ppc._gathered_rows(eng, n_local, total_chains, world, burnin)     # (every rank calls: a collective)
    if rank != 0:
        return None
    if rows.dim() != 3 or rows.shape[2] != LR_TRACE_W:
        raise ValueError("rows must be [samples, chains, LR_TRACE_W]")
    flat = rows.reshape(-1, LR_TRACE_W)
    idx = ppc.draw_indices(flat.shape[0], n_draws)
    _, mu = eng.draw_rates(flat, idx)
    if int(mu.shape[1]) != int(eng.n_bins):
        raise ValueError("draw_rates gave %d bins, the engine has %d" % (mu.shape[1], eng.n_bins))
    res = check_rates(eng.ts, eng.te, eng.t0, mu, seed, draw_rows=idx)
    write_tables(stem, res)
    print(_say(stem, res))
    return res
