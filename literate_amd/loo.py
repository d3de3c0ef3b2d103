"""Model comparison of finished runs: PSIS-LOO, Pareto-smoothed importance-sampling leave-one-out cross-validation
(Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman, Yao & Gabry, "Pareto smoothed importance sampling"; the
generalized-Pareto fit of Zhang & Stephens 2009), from the same posterior draws and per-lineage terms as WAIC (waic.py).

Under draw s lineage i adds l[i, s] to the log-likelihood (csrc/lr_device.h lr_score_lineage).  Leaving lineage i out
reweights the draws by r = exp(-l[i, s]); the largest M = min(floor(0.2 S), ceil(3 sqrt S)) of these ratios are replaced by
the quantiles of a generalized Pareto distribution fitted to them (ops.loo_pointwise, csrc/lr_loo.hip; the exact rules
stand in include/literate_hip.h):

    elpd_loo_i = log sum_s w[i, s] exp l[i, s] - log sum_s w[i, s]        lppd_i as WAIC defines it
    elpd_loo = sum_i elpd_loo_i    p_loo = sum_i (lppd_i - elpd_loo_i)    se_elpd = sqrt(n var_i(elpd_loo_i))    looic = -2 elpd_loo

pareto_k_i, the fitted shape, says WHERE the estimate fails: k <= 0.5 is good, up to 0.7 usable, above it the importance
ratios of that lineage have too heavy a tail for the S draws at hand.  k = +inf marks a lineage whose tail was not
smoothed (fewer than 25 draws, a constant tail, a fit that did not come out finite); such lineages are counted apart.

The relative efficiency of the draws is taken as 1: the draws are rows thinned by -s and pooled over many independent
chains (ppc.draw_indices spreads them over all post-burn-in rows), so their autocorrelation is what the thinning left,
and the tail length M - the only place r_eff enters - changes by a factor sqrt(r_eff) at most.

A lineage whose term is not finite under some draw is flagged as WAIC flags it: NaN in the pointwise file, left out of
every total.  What is comparable is what waic.py says: the pointwise files carry waic.fingerprint and `compare` refuses
files whose fingerprints differ, and files that are not PSIS-LOO files (a WAIC file beside LOO files does not compare).

    python -m literate_amd.loo A_LOO_pointwise.npz B_LOO_pointwise.npz [...] [-o table.tsv]
"""
from collections import namedtuple

import numpy as np

from . import waic
from .waic import fingerprint, fingerprint_mismatch  # noqa: F401  (the same fingerprint, by import)

METHOD = "psis-loo"
MAX_DRAWS = 8192
TSV_HEAD = ["draws", "lineages", "lineages_used", "lineages_flagged", "elpd_loo", "se_elpd", "p_loo", "lppd", "looic", "se_looic",
            "n_k_gt_0.5", "n_k_gt_0.7", "n_unsmoothed", "max_k"]
TSV_INTS = ("draws", "lineages", "lineages_used", "lineages_flagged", "n_k_gt_0.5", "n_k_gt_0.7", "n_unsmoothed")
COMPARE_HEAD = ["model", "elpd_loo", "p_loo", "elpd_diff", "se_diff", "lineages_used", "n_k_gt_0.7"]

LooResult = namedtuple("LooResult", "draws lineages lineages_used lineages_flagged elpd_loo se_elpd p_loo lppd looic se_looic "
                                    "n_k_gt_05 n_k_gt_07 n_unsmoothed max_k elpd pareto_k pointwise fingerprint plan draw_rows")
LooResult.__doc__ = """loo_from_rates' results (host values).  The totals of lr_loo_pointwise by name, looic = -2 elpd_loo,
se_looic = 2 se_elpd; elpd [n] and pareto_k [n] (NaN where flagged; k = +inf where unsmoothed), pointwise [n, 4] =
(elpd_loo_i, pareto_k_i, lppd_i, n_eff_i); fingerprint [6] (waic.FINGERPRINT); plan = (tail length, grid points of the fit,
lineages per batch, batches); draw_rows: the trace rows the draws came from (None when rates were given directly)."""


def arg_error(burnin, n_draws, model=2, pyrate_output=False, rm_first_bin=False):
    """Why a CLI's --loo BURNIN cannot run (None when it can): waic.arg_error's rules, and --loo_draws in [2, 8192]."""
    err = waic._arg_error("--loo", "--loo_draws must lie in [2, %d]" % MAX_DRAWS, burnin, n_draws, model, pyrate_output,
                          rm_first_bin)
    if err is None and n_draws > MAX_DRAWS:
        return "--loo_draws must lie in [2, %d] (a lineage's draws are sorted in the GPU's local memory)" % MAX_DRAWS
    return err


def loo_from_rates(ts, te, t0, lam_bins, mu_bins, model=2, br_length=None, end_time=0.0, draw_rows=None):
    """PSIS-LOO of S draws of per-bin rates lam_bins, mu_bins [S, n_bins] on the lineages (ts, te) -> LooResult."""
    from . import ops
    pw, tot, plan = ops.loo_pointwise(ts, te, t0, lam_bins, mu_bins, model=model, br_length=br_length, end_time=end_time)
    pw, tot = pw.cpu().numpy(), tot.cpu().numpy()
    S, n_bins = int(np.shape(lam_bins)[0]), int(np.shape(lam_bins)[1])
    fp = fingerprint(ops._host_f64(ts), ops._host_f64(te), t0, n_bins, model)
    return LooResult(S, len(pw), int(tot[0]), int(tot[1]), float(tot[2]), float(tot[3]), float(tot[4]), float(tot[5]),
                     -2.0 * float(tot[2]), 2.0 * float(tot[3]), int(tot[6]), int(tot[7]), int(tot[8]), float(tot[9]),
                     pw[:, 0].copy(), pw[:, 1].copy(), pw, fp, plan, draw_rows)


def write_files(stem, res):
    """<stem>_LOO.tsv (TSV_HEAD, one row; numbers as str(float), counts as integers) and <stem>_LOO_pointwise.npz (elpd [n]
    and pareto_k [n] in the order of the scored lineages, NaN where flagged; fingerprint [6]; method = "psis-loo")."""
    waic._write_row(stem + "_LOO.tsv", TSV_HEAD, TSV_INTS,
                    [res.draws, res.lineages, res.lineages_used, res.lineages_flagged, res.elpd_loo, res.se_elpd, res.p_loo,
                     res.lppd, res.looic, res.se_looic, res.n_k_gt_05, res.n_k_gt_07, res.n_unsmoothed, res.max_k])
    np.savez(stem + "_LOO_pointwise.npz", elpd=np.asarray(res.elpd, dtype=np.float64),
             pareto_k=np.asarray(res.pareto_k, dtype=np.float64), fingerprint=res.fingerprint, method=np.array(METHOD))


def _say(stem, res):
    return ("LOO: %s_LOO.tsv, %s_LOO_pointwise.npz (%d draws, %d lineages, %d flagged; elpd_loo %.6f, se %.6f, p_loo %.6f; "
            "%d lineages with k > 0.7)" % (stem, stem, res.draws, res.lineages, res.lineages_flagged, res.elpd_loo, res.se_elpd,
                                           res.p_loo, res.n_k_gt_07))


def write_run(eng, n_local, total_chains, world, rank, burnin, n_draws, stem):
    """The three CLIs' --loo (waic._run with loo_from_rates): <stem>_LOO.tsv, <stem>_LOO_pointwise.npz, one line on stdout."""
    return waic._run(loo_from_rates, write_files, _say, eng, n_local, total_chains, world, rank, burnin, n_draws, stem,
                     cap=(MAX_DRAWS, "PSIS-LOO takes at most %d draws" % MAX_DRAWS))


# ------------------------------------------------------------------------------------------------
# comparison of pointwise files (host only)
# ------------------------------------------------------------------------------------------------
def _read(p, z):
    if "method" not in z.files or str(z["method"]) != METHOD:
        raise ValueError("%s is not a PSIS-LOO pointwise file (method=\"%s\"): WAIC and LOO values are not "
                         "comparable with each other" % (p, METHOD))
    k = np.asarray(z["pareto_k"], dtype=np.float64) if "pareto_k" in z.files else None
    return np.asarray(z["elpd"], dtype=np.float64), np.asarray(z["fingerprint"], dtype=np.float64), k


def compare(paths):
    """Two or more <stem>_LOO_pointwise.npz -> rows sorted by elpd_loo, best first (waic.compare_arrays' arithmetic, with
    p_loo and the number of lineages with k > 0.7 per run); ValueError for a file that is not a PSIS-LOO file and unless
    every file's fingerprint equals the first one's."""
    paths, loaded = waic._comparable(paths, _read)
    rows = waic.compare_arrays(paths, [e for e, _, _ in loaded], [waic._beside(p, "p_loo") for p in paths])
    n_bad = {p: (-1 if k is None else int(np.sum(np.isfinite(k) & (k > 0.7)))) for p, (_, _, k) in zip(paths, loaded)}
    return [{"model": r["model"], "elpd_loo": r["elpd_waic"], "p_loo": r["p_waic"], "elpd_diff": r["elpd_diff"],
             "se_diff": r["se_diff"], "lineages_used": r["lineages_used"], "n_k_gt_0.7": n_bad[r["model"]]} for r in rows]


def format_table(rows):
    return waic._format_rows(COMPARE_HEAD, rows)


def main(argv=None):
    return waic._main(argv, "loo", "PSIS-LOO", "LOO", compare, format_table)


if __name__ == "__main__":
    main()
