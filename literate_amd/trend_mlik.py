"""Marginal likelihoods of the trend_rate.py models and a covariate screen: the Bayes factor of "the rates follow column c"
against "the rates are constant", and of column c against column d.

The chains are trend_rate.py's sampler on the power posteriors L^beta p of a ladder of temperatures, one chain per (model,
replicate, temperature), all of them in one kernel (include/literate_hip_tmlik.h, csrc/lr_tmlik.hip); the trend likelihood is
a function of create_bins' per-bin statistics and the covariate alone, so an iteration costs O(bins).  The estimator is
mlik's (ops.mlik_estimate on rows[m]); temperatures and multiplier scales are mlik.temperatures / mlik.window_scales.

The window schedule.  trend_rate.py moves its slopes by an additive normal step of sd 0.001, under a Normal(0, 5) prior: at
that window no chain of a few thousand iterations samples the prior (beta = 0), nor the posterior well.  The additive
window therefore starts at 0.001 and is tuned per (model, temperature) during the burn-in: the burn-in iterations are cut
into TUNE_BLOCKS blocks of launches, and after block b = 1 .. the acceptance rate of the additive move in that block, pooled
over the replicates (from the state's counters), gives win <- clip(win exp(4 (rate - 0.3) / sqrt(b)), 0.001, 20) (a
diminishing adaptation towards 30 % acceptance).  The counters leave out the additive steps whose mask fires for no slope
(a quarter of them when both rates vary): they propose the state itself and are always accepted, and a rate that counted them
would sit at 0.25 + 0.75 a for a real acceptance a - under the prior alone above 0.3 at any window, so that the clip, not the
rule, would set the cold windows.  A model with both rates constant makes no counted additive proposal and is never tuned.
The windows are frozen from the end of the burn-in and only rows after it are estimated, so the estimate comes from a fixed
kernel.  burnin = 0: the reference's 0.001 at every temperature, which cannot sample the priors.

The null model _CONB_COND does not read the covariate; it is always among the models, and every other model gets
two_ln_bf = 2 (log Z - log Z of the null) with the standard error from the two replicate standard errors.  Models go to the
device in groups whose rows fit `workspace_bytes`; key0[m] = (global model index) reps, so the grouping never shows in the
results.
"""
import math
from collections import namedtuple

import numpy as np

from . import mlik

MAX_BINS, MAX_TEMPS, MAX_MODELS = 512, 128, 64          # LR_TMLIK_MAX_BINS, LR_TMLIK_MAX_TEMPS, LR_TMLIK_MAX_MODELS
WIN0, WIN_MIN, WIN_MAX, TUNE_BLOCKS, TUNE_GAIN, TUNE_TARGET = 0.001, 0.001, 20.0, 20, 4.0, 0.3
ROW_BYTES = 96
NULL = (0, True, True)                                    # (column, const_B, const_D): the column is not read
FIT_HEAD = ["model", "column", "column_name", "logZ_ss", "logZ_ss_se", "logZ_ti", "two_ln_bf", "two_ln_bf_se", "min_lik_ess",
            "accept_mult_min", "accept_mult_max", "accept_add_min", "accept_add_max"]
TEMPS_HEAD = ["model", "column", "temp", "beta", "scale", "win", "lik_mean", "lik_sd", "lik_ess", "accept_mult", "accept_add", "stone"]
FIT_COMMENT = ("# logZ_ss: stepping stones pooled over the replicates, logZ_ss_se: sd of the per-replicate values / sqrt(reps); "
               "logZ_ti: trapezoid thermodynamic integration, biased by its discretisation in beta; two_ln_bf: 2 (logZ_ss - logZ_ss "
               "of _CONB_COND, the constant-rate model); additive windows tuned per temperature during the burn-in; accept_add: of the additive "
               "steps that move a slope (one that fires for neither is always accepted and not counted: not the raw rate of the move); "
               "%d temperatures x %d replicates x %d iterations, a row every %d, burn-in %s, alpha %s, widen %s, %d bins")

ModelResult = namedtuple("ModelResult", "col const_b const_d name fit temps ss pooled wins")
ModelResult.__doc__ = """One model of trend_mlik.run.  name: the model suffix; fit: dict (FIT_HEAD without column_name); temps: rows
(TEMPS_HEAD from `temp` on); ss [reps]; pooled: logZ_ss; wins [T]: the tuned additive windows."""
TrendMlikResult = namedtuple("TrendMlikResult", "models betas scales settings fingerprint")


def model_name(const_b, const_d):
    from .trendrate import model_suffix
    return model_suffix(const_b, const_d)


def arg_error(burnin, temps, reps, n_iter, s_freq, alpha, widen, n_bins=None, n_models=None):
    """Why --mlik BURNIN cannot run (None when it can)."""
    err = mlik.arg_error(burnin, temps, reps, n_iter, s_freq, alpha, widen, n_bins)
    if err:
        return err
    if n_models is not None and n_models * reps * temps > 2 ** 31 - 1:
        return "--mlik: %d models x %d replicates x %d temperatures are more chains than the sampler numbers" % (n_models, reps, temps)
    return None


def with_null(models):
    """the null first, then the given (column, const_B, const_D) in order, duplicates and further nulls dropped"""
    out = [NULL]
    for c, b, d in models:
        m = NULL if (b and d) else (int(c), bool(b), bool(d))
        if m not in out:
            out.append(m)
    return out


def tune_blocks(burn_iters):
    """the burn-in iterations [0, burn_iters) cut into TUNE_BLOCKS blocks -> their ends (block b is [ends[b - 1], ends[b]))"""
    return [(int(burn_iters) * b) // TUNE_BLOCKS for b in range(TUNE_BLOCKS + 1)]


def tuned(win, accepted, proposed, b, tunable):
    """the rule of the module docstring after block b (1-based).  win, accepted, proposed [M, T]: the additive move's
    counts of the block, pooled over the replicates; tunable [M]; a (model, temperature) without a proposal keeps its window"""
    with np.errstate(all="ignore"):
        rate = accepted / proposed
        new = np.clip(win * np.exp(TUNE_GAIN * (rate - TUNE_TARGET) / math.sqrt(b)), WIN_MIN, WIN_MAX)
    return np.where((proposed > 0) & np.asarray(tunable, dtype=bool)[:, None], new, win)


def group_size(n_rows, reps, temps, workspace_bytes):
    """models per device call: their rows fit workspace_bytes (at least one, at most LR_TMLIK_MAX_MODELS)"""
    per = max(int(n_rows), 1) * int(reps) * int(temps) * ROW_BYTES
    return int(max(1, min(MAX_MODELS, int(workspace_bytes) // per)))


def _run_group(data, grid, n_iter, s_freq, seed, burn):
    """the chains of one group of models -> (rows [M, n, R, T, 12], wins [M, T], acceptance after the burn-in [M, T, 2])"""
    import torch
    from . import ops
    S = ops.TMLIK_STATE
    M, T = grid.M, grid.T
    tunable = (grid.flags != 3)
    wins = np.full((M, T), WIN0)
    n = ops.rows_due(0, n_iter, s_freq)
    rows = ops.alloc_output((M, n, grid.R, T, 12), torch.float64, data.device)
    w_dev = torch.as_tensor(wins, device=data.device)
    state = ops.tmlik_init(data, grid, w_dev, seed)

    def counts():
        st = state.cpu().numpy()
        return st[:, :, :, S["proposed"]:S["proposed"] + 2].sum(axis=1), st[:, :, :, S["accepted"]:S["accepted"] + 2].sum(axis=1)

    it, slot = 0, 0
    prop0, acc0 = counts()
    ends = tune_blocks(burn * s_freq)
    for b in range(1, TUNE_BLOCKS + 1):
        if ends[b] > it:
            ops.tmlik_steps(data, grid, w_dev, state, it, ends[b] - it, s_freq, seed, rows=rows, slot0=slot)
            slot += ops.rows_due(it, ends[b] - it, s_freq)
            it = ends[b]
            prop, acc = counts()
            wins = tuned(wins, (acc - acc0)[:, :, 1], (prop - prop0)[:, :, 1], b, tunable)
            prop0, acc0 = prop, acc
            w_dev = torch.as_tensor(wins, device=data.device)
    if n_iter > it:
        ops.tmlik_steps(data, grid, w_dev, state, it, n_iter - it, s_freq, seed, rows=rows, slot0=slot)
    prop, acc = counts()
    with np.errstate(all="ignore"):
        rate = (acc - acc0) / (prop - prop0)                                        # NaN: the move is never made
    return rows, wins, rate


def run(n_spec, n_exti, DT, trends, models, temps=16, reps=8, n_iter=10000, s_freq=10, seed=1, burnin=0.3, alpha=0.3, widen=8.0,
        workspace_bytes=1 << 30, fingerprint=None):
    """The power-posterior chains of every model on the statistics (n_spec, n_exti, DT) and the normalised covariates trends
    [n_cols, n_bins], and the estimates from them.  models: (column, const_B, const_D) each; the null model is added
    (with_null) -> TrendMlikResult, .models in with_null's order."""
    from . import ops
    trends = np.atleast_2d(np.asarray(trends, dtype=float))
    models = with_null(models)
    err = arg_error(burnin, temps, reps, n_iter, s_freq, alpha, widen, len(DT), len(models))
    if err:
        raise ValueError(err)
    for c, _, _ in models:
        if not 0 <= c < len(trends):
            raise ValueError("--mlik: column %d is not among the %d covariates" % (c, len(trends)))
    betas = mlik.temperatures(temps, alpha)
    scales = mlik.window_scales(betas, widen)
    T, R = int(temps), int(reps)
    data = ops.TmlikData(n_spec, n_exti, DT, trends)
    n = ops.rows_due(0, n_iter, s_freq)
    burn = int(burnin * n)
    G = group_size(n, R, T, workspace_bytes)
    whole = ops.TmlikGrid([m[0] for m in models], [int(m[1]) + 2 * int(m[2]) for m in models], [g * R for g in range(len(models))],
                          betas, scales, R)
    out = []
    for a in range(0, len(models), G):
        grid = whole.part(models=(a, min(a + G, len(models))))
        rows, wins, rate = _run_group(data, grid, n_iter, s_freq, seed, burn)
        for i in range(grid.M):
            col, cb, cd = models[a + i]
            est = ops.mlik_estimate(rows[i], betas, row0=burn)
            es = ops.ess_summary(rows[i].reshape(n, R * T, rows.shape[4]), n, [ops.TMLIK_ROW.index("lik")], burnin=burnin)
            ess = es.ess.cpu().numpy().reshape(R, T)
            with np.errstate(all="ignore"):
                ess_t = np.nanmin(np.where(np.isnan(ess), np.inf, ess), axis=0)          # (NaN: a constant column)
                ss, pooled = est.ss.cpu().numpy(), est.pooled.cpu().numpy()
                mean, sd = est.lik_mean.cpu().numpy(), np.sqrt(np.mean(est.lik_var.cpu().numpy(), axis=0))
                rng = lambda k, f: float(f(rate[i, :, k])) if np.isfinite(rate[i, :, k]).any() else float("nan")
            fit = {"model": model_name(cb, cd), "column": col, "logZ_ss": float(pooled[-1]),
                   "logZ_ss_se": float(np.std(ss, ddof=1) / math.sqrt(R)) if R > 1 else float("nan"),
                   "logZ_ti": float(np.mean(est.ti.cpu().numpy())), "min_lik_ess": float(np.min(ess_t)),
                   "accept_mult_min": rng(0, np.nanmin), "accept_mult_max": rng(0, np.nanmax),
                   "accept_add_min": rng(1, np.nanmin), "accept_add_max": rng(1, np.nanmax)}
            trows = [(j, float(betas[j]), float(scales[j]), float(wins[i, j]), float(np.mean(mean[:, j])), float(sd[j]), float(ess_t[j]),
                      float(rate[i, j, 0]), float(rate[i, j, 1]), float(pooled[j]) if j < T - 1 else float("nan")) for j in range(T)]
            out.append(ModelResult(col, cb, cd, fit["model"], fit, trows, ss, float(pooled[-1]), wins[i].copy()))
        del rows
    null = out[0]
    for r in out:
        r.fit["two_ln_bf"] = 2.0 * (r.fit["logZ_ss"] - null.fit["logZ_ss"])
        r.fit["two_ln_bf_se"] = 0.0 if r is null else 2.0 * math.sqrt(r.fit["logZ_ss_se"] ** 2 + null.fit["logZ_ss_se"] ** 2)
    settings = dict(temps=T, reps=R, iterations=int(n_iter), s_freq=int(s_freq), burnin=float(burnin), alpha=float(alpha),
                    widen=float(widen), bins=len(DT), samples_kept=n - burn)
    fp = np.zeros(6) if fingerprint is None else np.asarray(fingerprint, dtype=np.float64)
    return TrendMlikResult(out, betas, scales, settings, fp)


def label(r):
    """`<model suffix>_<column>` (the null: its suffix alone)"""
    return r.name if (r.const_b and r.const_d) else "%s_%d" % (r.name, r.col)


def write_tables(stem, res, names=None):
    """<stem>_MLIK.tsv (a comment line, FIT_HEAD, one row per model, best log Z first), <stem>_MLIK_temps.tsv (TEMPS_HEAD, one
    row per model and temperature, in the same order), <stem>_MLIK.npz (names [M], ss [M, R], logZ_ss, logZ_ss_se [M], the data's
    fingerprint: what `python -m literate_amd.mlik` expands into one row per model).  names: the covariates' header names."""
    order = sorted(res.models, key=lambda r: -r.fit["logZ_ss"])
    s = res.settings
    cname = lambda r: "-" if (r.const_b and r.const_d) or names is None else str(names[r.col])
    with open(stem + "_MLIK.tsv", "w") as f:
        f.write(FIT_COMMENT % (s["temps"], s["reps"], s["iterations"], s["s_freq"], s["burnin"], s["alpha"], s["widen"], s["bins"]) + "\n")
        f.write("\t".join(FIT_HEAD) + "\n")
        for r in order:
            vals = [r.name, "%d" % r.col, cname(r)] + [str(float(r.fit[k])) for k in FIT_HEAD[3:]]
            f.write("\t".join(vals) + "\n")
    with open(stem + "_MLIK_temps.tsv", "w") as f:
        f.write("\t".join(TEMPS_HEAD) + "\n")
        for r in order:
            for t in r.temps:
                f.write("%s\t%d\t%d\t" % (r.name, r.col, t[0]) + "\t".join(str(float(v)) for v in t[1:]) + "\n")
    np.savez(stem + "_MLIK.npz", names=np.array([label(r) for r in order]), ss=np.array([r.ss for r in order]),
             logZ_ss=np.array([r.pooled for r in order]), logZ_ss_se=np.array([r.fit["logZ_ss_se"] for r in order]),
             model=np.str_("trend_rate"), fingerprint=np.asarray(res.fingerprint, dtype=np.float64))


def read_fit(stem):
    """<stem>_MLIK.tsv -> list of dicts (FIT_HEAD), in the file's order"""
    with open(stem + "_MLIK.tsv") as f:
        lines = [l.rstrip("\n").split("\t") for l in f if not l.startswith("#")]
    strs = ("model", "column_name")
    return [{k: v if k in strs else (int(v) if k == "column" else float(v)) for k, v in zip(lines[0], vals)} for vals in lines[1:]]


def _columns(columns, trend_index):
    """--mlik_columns -> the column indices, None for `all`"""
    if columns == "run":
        return [int(trend_index)]
    if columns == "all":
        return None
    try:
        return [int(c) for c in columns.split(",")]
    except ValueError:
        raise ValueError("--mlik_columns takes run, all or a comma-separated list of column indices")


def selection_error(columns, which, trend_index=0):
    """Why --mlik_columns / --mlik_models cannot be used, as far as it shows before the trend file is read (None: nothing)"""
    try:
        cols = _columns(columns, trend_index)
    except ValueError as e:
        return str(e)
    if cols is not None and min(cols) < 0:
        return "--mlik_columns: column %d is not a column index" % min(cols)
    return None if which in ("run", "all") else "--mlik_models takes run or all"


def select_models(columns, which, trend_index, const_b, const_d, n_cols):
    """--mlik_columns run|all|i,j,k and --mlik_models run|all -> (column, const_B, const_D) list (without the null)"""
    cols = _columns(columns, trend_index)
    if cols is None:
        cols = list(range(n_cols))
    for c in cols:
        if not 0 <= c < n_cols:
            raise ValueError("--mlik_columns: column %d is not among the trend file's %d columns" % (c, n_cols))
    if which == "run":
        kinds = [(bool(const_b), bool(const_d))]
    elif which == "all":
        kinds = [(False, False), (False, True), (True, False)]
    else:
        raise ValueError("--mlik_models takes run or all")
    return [(c, b, d) for c in cols for b, d in kinds]


def read_trends(path, rm_first_bin, cols=None):
    """the columns `cols` (None: every column; may be empty) of the trend file, normalised as the run normalises its own
    (trendrate.normalise_trend) -> (trends [n_cols, n_bins], a row of ones for a column not asked for; header names); a
    constant column is refused by name"""
    import pandas as pd
    from .trendrate import normalise_trend
    df = pd.read_csv(path, sep="\t")
    n = len(df) - 1 - (1 if rm_first_bin else 0)          # normalise_trend drops the last bin, and the first with -rm_first_bin
    if n < 1:
        raise ValueError("--mlik: %s holds too few rows" % path)
    out = np.ones((len(df.columns), n))
    for i, name in enumerate(df.columns):
        if cols is not None and i not in cols:
            continue
        x = df.iloc[:, i].to_numpy().astype(float)
        kept = x[:-1][1:] if rm_first_bin else x[:-1]
        if not np.all(np.isfinite(kept)) or np.max(kept) == np.min(kept):
            raise ValueError("--mlik: column %d (%s) of %s is constant or not finite over the run's bins: it cannot be normalised"
                             % (i, name, path))
        out[i] = normalise_trend(x, rm_first_bin)
    return out, [str(c) for c in df.columns]


def read_selection(trend_path, columns, which, trend_index, const_b, const_d, rm_first_bin):
    """Everything of --mlik that depends on the trend file, to be called BEFORE the run, on every rank: the models of
    --mlik_columns / --mlik_models (select_models) and their covariates (read_trends of the columns they name - none when the
    run's own model is the null) -> (trends, names, models); ValueError says what is wrong with the selection or the file"""
    import pandas as pd
    n_cols = len(pd.read_csv(trend_path, sep="\t", nrows=0).columns)
    models = select_models(columns, which, trend_index, const_b, const_d, n_cols)
    trends, names = read_trends(trend_path, rm_first_bin, sorted({m[0] for m in with_null(models)[1:]}))
    return trends, names, models


def _say(stem, res):
    s = res.settings
    best = max(res.models, key=lambda r: r.fit["logZ_ss"])
    return ("MLIK: %s_MLIK.tsv, _MLIK_temps.tsv, _MLIK.npz (%d models; best %s: log Z %.4f +- %.4f, 2 ln BF against %s %.3f +- %.3f; "
            "%d temperatures x %d replicates x %d iterations, %d samples kept per chain)"
            % (stem, len(res.models), label(best), best.fit["logZ_ss"], best.fit["logZ_ss_se"], res.models[0].name, best.fit["two_ln_bf"],
               best.fit["two_ln_bf_se"], s["temps"], s["reps"], s["iterations"], s["samples_kept"]))


def write_run(eng, rank, selection, burnin, temps, reps, n_iter, s_freq, alpha, widen, seed, stem, workspace_bytes=1 << 30):
    """trend_rate.py's --mlik, after the run, on rank 0 alone: the engine's statistics (create_bins' output) and seed, the
    covariates and models of `selection` (read_selection's result, made before the run).  It does not read the run's trace.
    -> the three files and one line on stdout.  What can be refused is refused on every rank alike."""
    from . import ops, waic
    trends, names, models = selection
    if len(eng.DT) > MAX_BINS:
        raise ValueError(mlik.too_many_bins(len(eng.DT)))
    if trends.shape[1] != len(eng.DT):
        raise ValueError("--mlik: the trend file gives %d bins, the data %d" % (trends.shape[1], len(eng.DT)))
    if rank != 0:
        return None
    fp = waic.fingerprint(ops._host_f64(eng.ts), ops._host_f64(eng.te), eng.origin, len(eng.DT), 0)
    res = run(eng.n_spec, eng.n_exti, eng.DT, trends, models, temps, reps, n_iter, s_freq, seed, burnin, alpha, widen,
              workspace_bytes, fingerprint=fp)
    write_tables(stem, res, names)
    print(_say(stem, res))
    return res
