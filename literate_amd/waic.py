"""Model comparison of finished runs: WAIC (Watanabe 2010; Vehtari, Gelman & Gabry 2017) from posterior draws.

The birth-death likelihood factorises over lineages: under draw s lineage i adds l[i, s], the term the lineage scan adds
for it (csrc/lr_device.h lr_score_lineage).  ops.waic_pointwise reduces the [lineages, draws] matrix over the draws on the
device without storing it:

    lppd_i = log mean_s exp l[i, s]        var_i = the sample variance over s of l[i, s]        elpd_i = lppd_i - var_i
    elpd_waic = sum_i elpd_i    p_waic = sum_i var_i    se_elpd = sqrt(n var_i(elpd_i))    waic = -2 elpd_waic

A lineage whose term is not finite under some draw (a zero rate: -inf; a nan rate) is flagged: NaN in the pointwise file,
left out of every total.  var_i > 0.4 is the usual sign that WAIC is unreliable for that lineage; the count is reported.

Draws are chosen as --ppc chooses them (ppc.draw_indices: row floor(i M / R) of the M post-burn-in rows).

What is comparable.  elpd values are sums over the SAME lineages of densities of the SAME data: two runs compare only when
they were scored on the same lineages, window and model id.  Every pointwise file carries the fingerprint
[n, t0, n_bins, model id, sum ts, sum te] and `compare` refuses files whose fingerprints differ.  Runs of one CLI on one
data set agree (DDRate.py's nine models, trend_rate.py's variants, LiteRateForward.py's -const_rates / -const_death_rate
against the full RJ skyline); LiteRateForward.py against DDRate.py does not (DDRate drops the last bin, and under
-model_BDI 0 the term carries log k_b of the data's own branch length: the lineages are then the units of a conditional
factorisation, as in the reference's BD_partial_lik form).  Under model 0 the values are still comparable between runs
of model 0 on the same data: the log k_b terms are the same data-only constants in both.

    python -m literate_amd.waic A_WAIC_pointwise.npz B_WAIC_pointwise.npz [...] [-o table.tsv]
"""
import math
from collections import namedtuple

import numpy as np

TSV_HEAD = ["draws", "lineages", "lineages_used", "lineages_flagged", "lppd", "p_waic", "elpd_waic", "se_elpd", "waic",
            "se_waic", "n_var_gt_0.4", "max_var"]
TSV_INTS = ("draws", "lineages", "lineages_used", "lineages_flagged", "n_var_gt_0.4")
COMPARE_HEAD = ["model", "elpd_waic", "p_waic", "elpd_diff", "se_diff", "lineages_used"]
FINGERPRINT = ("n", "t0", "n_bins", "model", "sum_ts", "sum_te")

WaicResult = namedtuple("WaicResult", "draws lineages lineages_used lineages_flagged lppd p_waic elpd_waic se_elpd waic "
                                      "se_waic n_var_gt_04 max_var elpd pointwise fingerprint plan draw_rows")
WaicResult.__doc__ = """waic_from_rates' results (host values).  The totals of lr_waic_pointwise by name, waic = -2 elpd_waic,
se_waic = 2 se_elpd; elpd [n] = lppd_i - var_i (NaN where flagged), pointwise [n, 3] = (lppd_i, mean_i, var_i);
fingerprint [6] (FINGERPRINT); plan = (lineages per tile, draws per LDS chunk, draw slices, tiles); draw_rows: the trace
rows the draws came from (None when rates were given directly)."""


def _arg_error(flag, few_draws, burnin, n_draws, model, pyrate_output, rm_first_bin):
    """arg_error's rules for the CLI flag `flag` ("--waic", "--loo"); few_draws: what to say of fewer than 2 draws"""
    if not (0.0 <= burnin < 1.0):
        return "%s takes a burn-in fraction in [0, 1)" % flag
    if n_draws < 2:
        return few_draws
    if model == 1:
        return ("%s sums per-lineage terms; under -model_BDI 1 (immigration-death) the likelihood carries a per-bin "
                "constant that belongs to no lineage: not supported together" % flag)
    if rm_first_bin:
        return ("%s scores every lineage of the data; under -rm_first_bin 1 the lineages of the removed bin would be "
                "scored outside the window the model was fitted on: not supported together" % flag)
    if pyrate_output:
        return ("%s reads the AD / TBP times of the trace; -pyrate_output flips them in the logs: not supported together"
                % flag)
    return None


def arg_error(burnin, n_draws, model=2, pyrate_output=False, rm_first_bin=False):
    """Why a CLI's --waic BURNIN cannot run (None when it can).  LiteRateForward.py passes its -model_BDI and
    -pyrate_output, DDRate.py / trend_rate.py their -rm_first_bin."""
    return _arg_error("--waic", "--waic_draws must be at least 2 (a variance over the draws)", burnin, n_draws, model,
                      pyrate_output, rm_first_bin)


def fingerprint(ts, te, t0, n_bins, model):
    """[n, t0, n_bins, model id, sum ts, sum te]: the sums exact (math.fsum), so the order of the lineages does not enter"""
    ts, te = np.asarray(ts, dtype=np.float64).ravel(), np.asarray(te, dtype=np.float64).ravel()
    return np.array([float(len(ts)), float(t0), float(n_bins), float(model), math.fsum(ts), math.fsum(te)])


def waic_from_rates(ts, te, t0, lam_bins, mu_bins, model=2, br_length=None, end_time=0.0, draw_rows=None):
    """WAIC of S draws of per-bin rates lam_bins, mu_bins [S, n_bins] on the lineages (ts, te) -> WaicResult."""
    from . import ops
    pw, tot, plan = ops.waic_pointwise(ts, te, t0, lam_bins, mu_bins, model=model, br_length=br_length, end_time=end_time)
    pw, tot = pw.cpu().numpy(), tot.cpu().numpy()
    S, n_bins = int(np.shape(lam_bins)[0]), int(np.shape(lam_bins)[1])
    fp = fingerprint(ops._host_f64(ts), ops._host_f64(te), t0, n_bins, model)
    return WaicResult(S, len(pw), int(tot[0]), int(tot[1]), float(tot[2]), float(tot[3]), float(tot[4]), float(tot[5]),
                      -2.0 * float(tot[4]), 2.0 * float(tot[5]), int(tot[6]), float(tot[7]), pw[:, 0] - pw[:, 2], pw, fp, plan,
                      draw_rows)


def _write_row(path, head, ints, vals):
    """a tsv of one row under `head`: numbers as str(float), the columns named in `ints` as integers"""
    with open(path, "w") as f:
        f.write("\t".join(head) + "\n")
        f.write("\t".join("%d" % v if k in ints else str(float(v)) for k, v in zip(head, vals)) + "\n")


def write_files(stem, res):
    """<stem>_WAIC.tsv (TSV_HEAD, one row; numbers as str(float), counts as integers) and <stem>_WAIC_pointwise.npz (elpd [n]
    in the order of the scored lineages, NaN where flagged; fingerprint [6])."""
    _write_row(stem + "_WAIC.tsv", TSV_HEAD, TSV_INTS,
               [res.draws, res.lineages, res.lineages_used, res.lineages_flagged, res.lppd, res.p_waic, res.elpd_waic, res.se_elpd,
                res.waic, res.se_waic, res.n_var_gt_04, res.max_var])
    np.savez(stem + "_WAIC_pointwise.npz", elpd=np.asarray(res.elpd, dtype=np.float64), fingerprint=res.fingerprint)


def _say(stem, res):
    return ("WAIC: %s_WAIC.tsv, %s_WAIC_pointwise.npz (%d draws, %d lineages, %d flagged; elpd_waic %.6f, se %.6f, p_waic %.6f; "
            "%d lineages with var > 0.4)" % (stem, stem, res.draws, res.lineages, res.lineages_flagged, res.elpd_waic, res.se_elpd,
                                            res.p_waic, res.n_var_gt_04))


def _run(from_rates, write, say, eng, n_local, total_chains, world, rank, burnin, n_draws, stem, cap=None):
    """What --waic and --loo do after a run: the rows it sampled, int(burnin * S) dropped per chain, gathered to rank 0; there
    n_draws of them chosen as --ppc chooses them, their per-bin rates by the engine's own draw_rates, scored by from_rates
    against the engine's lineages, window, model id and br_length -> write's two files and say's line on stdout.
    cap: (most n_draws the criterion takes, what to say of more)."""
    from . import ppc
    from ._hip import LR_TRACE_W
    rows = ppc._gathered_rows(eng, n_local, total_chains, world, burnin)     # (every rank calls: a collective)
    if rank != 0:
        return None
    if cap is not None and n_draws > cap[0]:
        raise ValueError(cap[1])
    if rows.dim() != 3 or rows.shape[2] != LR_TRACE_W:
        raise ValueError("rows must be [samples, chains, LR_TRACE_W]")
    flat = rows.reshape(-1, LR_TRACE_W)
    idx = ppc.draw_indices(flat.shape[0], n_draws)
    if len(idx) < 2:
        raise ValueError("WAIC needs at least 2 draws (%d post-burn-in rows)" % flat.shape[0])
    lam, mu = eng.draw_rates(flat, idx)
    res = from_rates(eng.ts, eng.te, eng.t0, lam, mu, model=eng.model, br_length=eng.br_length if eng.model == 0 else None,
                     end_time=eng.end_time, draw_rows=idx)
    write(stem, res)
    print(say(stem, res))
    return res


def write_run(eng, n_local, total_chains, world, rank, burnin, n_draws, stem):
    """The three CLIs' --waic (_run with waic_from_rates): <stem>_WAIC.tsv, <stem>_WAIC_pointwise.npz, one line on stdout."""
    return _run(waic_from_rates, write_files, _say, eng, n_local, total_chains, world, rank, burnin, n_draws, stem)


# ------------------------------------------------------------------------------------------------
# comparison of pointwise files (host only)
# ------------------------------------------------------------------------------------------------
def fingerprint_mismatch(fa, fb):
    """the first field of two fingerprints that differs (its name), or None"""
    fa, fb = np.asarray(fa, dtype=np.float64).ravel(), np.asarray(fb, dtype=np.float64).ravel()
    if fa.shape != (6,) or fb.shape != (6,):
        return "shape"
    for name, a, b in zip(FINGERPRINT, fa, fb):
        if a != b:
            return name
    return None


def compare_arrays(names, elpds, p_waics=None):
    """Rows (dicts, COMPARE_HEAD) sorted by elpd_waic, best first.  elpds: one [n] array per model, NaN where flagged.
    elpd_waic of a row is over ITS used lineages; elpd_diff and se_diff against the best model are over the lineages used
    in BOTH: elpd_diff = sum (elpd_i - elpd_i^best), se_diff = sqrt(n_both * sample variance of those differences)
    (nan with fewer than 2); the best model's own row holds 0 and 0."""
    E = [np.asarray(e, dtype=np.float64) for e in elpds]
    tot = [float(np.sum(e[np.isfinite(e)])) for e in E]
    order = sorted(range(len(E)), key=lambda k: -tot[k])
    best = order[0]
    rows = []
    for k in order:
        both = np.isfinite(E[k]) & np.isfinite(E[best])
        d = E[k][both] - E[best][both]
        nb = int(both.sum())
        if k == best:
            diff, se = 0.0, 0.0
        else:
            diff = float(np.sum(d))
            se = float(np.sqrt(nb * np.var(d, ddof=1))) if nb >= 2 else float("nan")
        rows.append({"model": names[k], "elpd_waic": tot[k], "p_waic": float("nan") if p_waics is None else float(p_waics[k]),
                     "elpd_diff": diff, "se_diff": se, "lineages_used": int(np.isfinite(E[k]).sum())})
    return rows


def _beside(path, name):
    """column `name` of the one-row <stem>_X.tsv that write_files left beside <stem>_X_pointwise.npz (nan when it is not there)"""
    import os
    tsv = path[:-len("_pointwise.npz")] + ".tsv" if path.endswith("_pointwise.npz") else None
    if not tsv or not os.path.exists(tsv):
        return float("nan")
    with open(tsv) as f:
        head, row = f.readline().rstrip("\n").split("\t"), f.readline().rstrip("\n").split("\t")
    return float(row[head.index(name)]) if name in head and len(row) == len(head) else float("nan")


def _comparable(paths, read):
    """read(path, npz) -> a tuple that begins (elpd, fingerprint, ...) for each of two or more pointwise files; ValueError
    unless every file's fingerprint (and number of lineages) equals the first one's"""
    paths = list(paths)
    if len(paths) < 2:
        raise ValueError("compare takes two or more pointwise files")
    loaded = []
    for p in paths:
        with np.load(p) as z:
            loaded.append(read(p, z))
    for p, rec in zip(paths[1:], loaded[1:]):
        bad = fingerprint_mismatch(loaded[0][1], rec[1])
        if bad is None and len(rec[0]) != len(loaded[0][0]):
            bad = "n"
        if bad:
            raise ValueError("fingerprint mismatch (%s): %s and %s were not scored on the same lineages, window and model id; "
                             "their WAIC values are not comparable" % (bad, paths[0], p))
    return paths, loaded


def compare(paths):
    """Two or more <stem>_WAIC_pointwise.npz -> rows sorted by elpd (compare_arrays); ValueError unless every file's
    fingerprint equals the first one's (the runs were then not scored on the same lineages, window and model id)."""
    paths, loaded = _comparable(paths, lambda p, z: (np.asarray(z["elpd"], dtype=np.float64),
                                                     np.asarray(z["fingerprint"], dtype=np.float64)))
    return compare_arrays(paths, [e for e, _ in loaded], [_beside(p, "p_waic") for p in paths])


def _format_rows(head, rows):
    """rows (dicts) under `head`: the model's name, four numbers as str(float), the remaining columns as integers"""
    lines = ["\t".join(head)]
    for r in rows:
        lines.append("\t".join([str(r["model"])] + [str(float(r[k])) for k in head[1:5]] + ["%d" % r[k] for k in head[5:]]))
    return "\n".join(lines) + "\n"


def format_table(rows):
    return _format_rows(COMPARE_HEAD, rows)


def _main(argv, module, name, tag, compare_, format_):
    """python -m literate_amd.<module>: the table of compare_ on stdout (and in -o).  name and tag: "WAIC" and "WAIC",
    "PSIS-LOO" and "LOO"."""
    import argparse
    p = argparse.ArgumentParser(prog="python -m literate_amd.%s" % module,
                                description="rank runs by %s from their <stem>_%s_pointwise.npz files" % (name, tag))
    p.add_argument("files", nargs="+", help="two or more <stem>_%s_pointwise.npz written by --%s" % (tag, module))
    p.add_argument("-o", default="", help="also write the table to this file")
    args = p.parse_args(argv)
    try:
        text = format_(compare_(args.files))
    except ValueError as ex:
        raise SystemExit(str(ex))
    print(text, end="")
    if args.o:
        with open(args.o, "w") as f:
            f.write(text)
    return 0


def main(argv=None):
    return _main(argv, "waic", "WAIC", "WAIC", compare, format_table)


if __name__ == "__main__":
    main()
