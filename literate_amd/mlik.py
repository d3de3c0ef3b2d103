"""Marginal likelihoods of the DDRate models: the Bayes factor between -m_birth / -m_death combinations.

--waic and --loo rank models by predictive scores; the marginal likelihood log Z = log int L(theta) p(theta) dtheta is what a
Bayes factor is made of.  It is estimated from power posteriors L^beta p on a ladder of temperatures 0 = beta_0 < .. <
beta_{T-1} = 1, one chain per (replicate, temperature), all of them in one kernel (include/literate_hip_mlik.h,
csrc/lr_mlik.hip).  The DDRate likelihood is a function of create_bins' per-bin statistics alone, so an iteration costs
O(bins) whatever the number of lineages.

1. beta_j = (j / (T - 1)) ** (1 / alpha); window scales s_j = min(beta_j ** -1/2, widen): DDRate.py's +-5 % multiplier cannot
   sample the Exp(scale 10) and Exp(scale max DT) priors the cold chains see.
2. ops.mlik_run: `reps` x T chains, n_iter iterations, a row every s_freq.
3. ops.mlik_estimate on the rows after the burn-in: the stepping-stone estimate per replicate and pooled, the trapezoid
   thermodynamic integration (biased by its discretisation: with few temperatures it is the worse of the two).
4. <stem>_MLIK.tsv (one row), <stem>_MLIK_temps.tsv (one row per temperature), <stem>_MLIK.npz.

What the number is: the marginal likelihood under the prior AS THE SAMPLER REALISES IT.  A parameter moved by the multiplier
never changes sign, so the Normal priors on k, nuB and nuD act as half-Normals on the side of the initial value; the midpoint
is uniform on its reflected range [0, present) with the prior's cut at origin + x0 < present.  The stones start at beta = 0, so
that prior is normalised by construction and the value needs no constant.  Values of runs on the same data compare;
compare A_MLIK.npz B_MLIK.npz refuses files of other data.

trend_rate.py's models have a module of their own (literate_amd/trend_mlik.py: a grid of models per launch, the additive
window tuned during the burn-in); its <stem>_MLIK.npz holds several models and the tool below expands it into one row each.
Not built: LiteRateForward.py (its RJ sampler already averages over its models), swaps between temperatures, several GPUs
(rank 0 carries every chain).

    python -m literate_amd.mlik A_MLIK.npz B_MLIK.npz [-o table.tsv]
"""
import math
import sys
from collections import namedtuple

import numpy as np

MAX_BINS, MAX_TEMPS = 512, 128                      # LR_MLIK_MAX_BINS, LR_MLIK_MAX_TEMPS
MOVES = ("mult", "slide")
FIT_HEAD = ["model", "logZ_ss", "logZ_ss_se", "logZ_ti", "temps", "reps", "iterations", "s_freq", "burnin", "alpha", "widen",
            "samples_kept", "bins", "min_lik_ess", "accept_min", "accept_max"]
FIT_STRS, FIT_INTS = ["model"], ["temps", "reps", "iterations", "s_freq", "samples_kept", "bins"]
TEMPS_HEAD = ["temp", "beta", "scale", "lik_mean", "lik_sd", "lik_ess", "accept_mult", "accept_slide", "stone"]
FIT_COMMENT = ("# logZ_ss: stepping stones pooled over the replicates, logZ_ss_se: sd of the per-replicate values / sqrt(reps); "
               "logZ_ti: trapezoid thermodynamic integration, biased by its discretisation in beta (no such bias in logZ_ss); "
               "the prior is the one the sampler realises (multiplier-moved parameters keep their sign)")
COMPARE_HEAD = ["name", "model", "logZ_ss", "logZ_ss_se", "two_ln_bf", "two_ln_bf_se"]

MlikResult = namedtuple("MlikResult", "rows state betas scales est ess fit temps ss pooled fingerprint")
MlikResult.__doc__ = """run's results.  rows [samples, reps, T, LR_MLIK_ROW_W], state [reps, T, LR_MLIK_STATE_W]: device tensors as
ops.mlik_run returns them; betas, scales [T]; est: ops.MlikEstimate; ess [T]: the smallest ESS of lik over the replicates;
fit: dict of <stem>_MLIK.tsv (FIT_HEAD); temps: rows of <stem>_MLIK_temps.tsv (TEMPS_HEAD); ss [reps], pooled: the
stepping-stone estimates; fingerprint: of the data (waic.fingerprint)."""


def temperatures(T, alpha):
    """beta_j = (j / (T - 1)) ** (1 / alpha)"""
    return (np.arange(int(T)) / (int(T) - 1.0)) ** (1.0 / float(alpha))


def window_scales(betas, widen):
    """s_j = min(beta_j ** -1/2, widen)"""
    with np.errstate(divide="ignore"):
        return np.minimum(np.asarray(betas, dtype=float) ** -0.5, float(widen))


def arg_error(burnin, temps, reps, n_iter, s_freq, alpha, widen, n_bins=None):
    """Why --mlik BURNIN cannot run (None when it can)."""
    if not (0.0 <= burnin < 1.0):
        return "--mlik takes a burn-in fraction in [0, 1)"
    if not (2 <= temps <= MAX_TEMPS):
        return "--mlik_temps must be between 2 and %d" % MAX_TEMPS
    if reps < 1:
        return "--mlik_reps must be at least 1"
    if n_iter < 1:
        return "--mlik_n must be at least 1"
    if s_freq < 1:
        return "--mlik_s must be at least 1"
    if not (alpha > 0.0 and math.isfinite(alpha)):
        return "--mlik_alpha must be a positive exponent"
    if not (widen >= 1.0 and math.isfinite(widen)):
        return "--mlik_widen must be at least 1 (1: the reference's windows at every temperature)"
    n = (int(n_iter) + int(s_freq) - 1) // int(s_freq)
    if n - int(burnin * n) < 4:
        return "--mlik: %d iterations at one row per %d leave fewer than 4 samples after the burn-in" % (n_iter, s_freq)
    if n_bins is not None and n_bins > MAX_BINS:
        return too_many_bins(n_bins)
    return None


def too_many_bins(n_bins):
    return ("--mlik: the run has %d time bins, and the sampler takes at most %d (LR_MLIK_MAX_BINS): a lane keeps 8 bins' "
            "statistics in registers" % (n_bins, MAX_BINS))


def run(n_spec, n_exti, DT, origin, present, m_birth, m_death, init_death=0.1, temps=16, reps=8, n_iter=10000, s_freq=10, seed=1,
        burnin=0.2, alpha=0.3, widen=8.0, fingerprint=None):
    """The power-posterior chains on the statistics (n_spec, n_exti, DT) and the estimates from them -> MlikResult."""
    from . import ops
    from .ddrate import model_suffix
    err = arg_error(burnin, temps, reps, n_iter, s_freq, alpha, widen, len(DT))
    if err:
        raise ValueError(err)
    betas = temperatures(temps, alpha)
    scales = window_scales(betas, widen)
    data = ops.MlikData(n_spec, n_exti, DT, origin, present, m_birth, m_death, init_death)
    rows, state = ops.mlik_run(data, betas, scales, reps, n_iter, s_freq, seed)
    n = int(rows.shape[0])
    burn = int(burnin * n)
    est = ops.mlik_estimate(rows, betas, row0=burn)
    T, R = int(temps), int(reps)
    es = ops.ess_summary(rows.reshape(n, R * T, rows.shape[3]), n, [ops.MLIK_ROW.index("lik")], burnin=burnin)
    ess = es.ess.cpu().numpy().reshape(R, T)
    with np.errstate(all="ignore"):
        ess_t = np.nanmin(np.where(np.isnan(ess), np.inf, ess), axis=0)          # (NaN: a constant column)
    st = state.cpu().numpy()
    prop = st[:, :, ops.MLIK_STATE["proposed"]:ops.MLIK_STATE["proposed"] + 2].sum(axis=0)
    acc = st[:, :, ops.MLIK_STATE["accepted"]:ops.MLIK_STATE["accepted"] + 2].sum(axis=0)
    with np.errstate(all="ignore"):
        rate = acc / prop                                                          # [T, 2]; NaN: the move is never made
    ss, pooled = est.ss.cpu().numpy(), est.pooled.cpu().numpy()
    mean, var = est.lik_mean.cpu().numpy(), est.lik_var.cpu().numpy()
    fit = {"model": model_suffix(m_birth, m_death), "logZ_ss": float(pooled[-1]),
           "logZ_ss_se": float(np.std(ss, ddof=1) / math.sqrt(R)) if R > 1 else float("nan"),
           "logZ_ti": float(np.mean(est.ti.cpu().numpy())), "temps": T, "reps": R, "iterations": int(n_iter), "s_freq": int(s_freq),
           "burnin": float(burnin), "alpha": float(alpha), "widen": float(widen), "samples_kept": n - burn, "bins": len(DT),
           "min_lik_ess": float(np.min(ess_t)), "accept_min": float(np.nanmin(rate)), "accept_max": float(np.nanmax(rate))}
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.mean(var, axis=0))
    trows = [(j, float(betas[j]), float(scales[j]), float(np.mean(mean[:, j])), float(sd[j]), float(ess_t[j]), float(rate[j, 0]),
              float(rate[j, 1]), float(pooled[j]) if j < T - 1 else float("nan")) for j in range(T)]
    fp = np.zeros(6) if fingerprint is None else np.asarray(fingerprint, dtype=np.float64)
    return MlikResult(rows, state, betas, scales, est, ess_t, fit, trows, ss, float(pooled[-1]), fp)


def _fmt(k, v):
    return str(v) if k in FIT_STRS else ("%d" % v if k in FIT_INTS else str(float(v)))


def write_tables(stem, res):
    """<stem>_MLIK.tsv (a comment line, FIT_HEAD, one row), <stem>_MLIK_temps.tsv (TEMPS_HEAD, one row per temperature),
    <stem>_MLIK.npz (ss per replicate, the pooled value, its standard error, the model suffix and the data's fingerprint)."""
    with open(stem + "_MLIK.tsv", "w") as f:
        f.write(FIT_COMMENT + "\n")
        f.write("\t".join(FIT_HEAD) + "\n")
        f.write("\t".join(_fmt(k, res.fit[k]) for k in FIT_HEAD) + "\n")
    with open(stem + "_MLIK_temps.tsv", "w") as f:
        f.write("\t".join(TEMPS_HEAD) + "\n")
        for r in res.temps:
            f.write("%d\t" % r[0] + "\t".join(str(float(v)) for v in r[1:]) + "\n")
    np.savez(stem + "_MLIK.npz", ss=np.asarray(res.ss), logZ_ss=np.float64(res.pooled), logZ_ss_se=np.float64(res.fit["logZ_ss_se"]),
             model=np.str_(res.fit["model"]), fingerprint=np.asarray(res.fingerprint, dtype=np.float64))


def read_fit(stem):
    """<stem>_MLIK.tsv -> dict (FIT_HEAD)"""
    with open(stem + "_MLIK.tsv") as f:
        head, vals = [l.rstrip("\n").split("\t") for l in f if not l.startswith("#")]
    return {k: v if k in FIT_STRS else (int(v) if k in FIT_INTS else float(v)) for k, v in zip(head, vals)}


def _say(stem, res):
    f = res.fit
    return ("MLIK: %s_MLIK.tsv, _MLIK_temps.tsv, _MLIK.npz (%s: log Z %.4f +- %.4f by stepping stones, %.4f by thermodynamic "
            "integration; %d temperatures x %d replicates x %d iterations, %d samples kept per chain; smallest ESS of the "
            "likelihood %.0f, acceptance %.3f - %.3f)"
            % (stem, f["model"], f["logZ_ss"], f["logZ_ss_se"], f["logZ_ti"], f["temps"], f["reps"], f["iterations"],
               f["samples_kept"], f["min_lik_ess"], f["accept_min"], f["accept_max"]))


def write_run(eng, rank, burnin, temps, reps, n_iter, s_freq, alpha, widen, seed, stem, init_death=0.1):
    """DDRate.py's --mlik, after the run, on rank 0 alone: the engine's statistics (create_bins' output, so -rm_first_bin 1 is
    what the run saw), window, model and seed.  It does not read the run's trace.  -> the three files and one line on stdout."""
    from . import ops, waic
    if len(eng.DT) > MAX_BINS:
        raise ValueError(too_many_bins(len(eng.DT)))
    if rank != 0:
        return None
    # (the model field stays 0: files of different models on the same data are what the tool compares)
    fp = waic.fingerprint(ops._host_f64(eng.ts), ops._host_f64(eng.te), eng.origin, len(eng.DT), 0)
    res = run(eng.n_spec, eng.n_exti, eng.DT, eng.origin, eng.present, eng.m_birth, eng.m_death, init_death, temps, reps, n_iter,
              s_freq, seed, burnin, alpha, widen, fingerprint=fp)
    write_tables(stem, res)
    print(_say(stem, res))
    return res


# ---- the comparison tool -----------------------------------------------------------------------------------------------
def compare(paths):
    """Rows (dicts, COMPARE_HEAD) of <stem>_MLIK.npz files sorted by log Z, best first; two_ln_bf = 2 (logZ - logZ of the
    best), its standard error from the two replicate standard errors.  A file of several models (trend_rate.py --mlik) gives
    a row per model.  Files of other data (fingerprints) are refused."""
    from .waic import fingerprint_mismatch
    items = []
    for p in paths:
        with np.load(p) as z:
            if np.ndim(z["logZ_ss"]) == 1:          # a file of several models (trend_mlik.write_tables): one row each
                for name, lz, se in zip(z["names"], z["logZ_ss"], z["logZ_ss_se"]):
                    items.append(dict(name=p, model=str(name), logZ_ss=float(lz), logZ_ss_se=float(se), fp=np.asarray(z["fingerprint"])))
                continue
            items.append(dict(name=p, model=str(z["model"]), logZ_ss=float(z["logZ_ss"]), logZ_ss_se=float(z["logZ_ss_se"]),
                              fp=np.asarray(z["fingerprint"])))
    for it in items[1:]:
        bad = fingerprint_mismatch(items[0]["fp"], it["fp"])
        if bad:
            raise ValueError("%s and %s were computed on different data (%s differs): their marginal likelihoods do not compare"
                             % (items[0]["name"], it["name"], bad))
    items.sort(key=lambda d: -d["logZ_ss"])
    best = items[0]
    for it in items:
        it["two_ln_bf"] = 2.0 * (it["logZ_ss"] - best["logZ_ss"])
        it["two_ln_bf_se"] = 0.0 if it is best else 2.0 * math.sqrt(it["logZ_ss_se"] ** 2 + best["logZ_ss_se"] ** 2)
        del it["fp"]
    return items


def format_compare(rows):
    out = ["\t".join(COMPARE_HEAD)]
    for r in rows:
        out.append("\t".join(str(r[k]) if k in ("name", "model") else str(float(r[k])) for k in COMPARE_HEAD))
    return "\n".join(out) + "\n"


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m literate_amd.mlik", description="rank <stem>_MLIK.npz files of runs on the same "
                                "data by their marginal likelihood: 2 ln BF against the best")
    p.add_argument("files", nargs="+")
    p.add_argument("-o", default=None, help="write the table here (default: stdout)")
    a = p.parse_args(argv)
    try:
        text = format_compare(compare(a.files))
    except ValueError as e:
        raise SystemExit(str(e))
    if a.o:
        with open(a.o, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
