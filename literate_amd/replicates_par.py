"""DDRate.py's and trend_rate.py's samplers on many replicate data sets in one launch (include/literate_hip_parbin.h,
csrc/lr_parbin.hip): the restricted models' counterpart of literate_amd/replicates.py.

Both likelihoods are functions of create_bins' per-bin statistics alone, so every chain carries the statistics of its own
replicate - one stochastic imputation of the death times, say - and all chains of all replicates run in one kernel:

    load_binned_replicates       the files parsed and binned by the CLIs' own rules (parse_ts_te, create_bins)
    ParametricReplicateEngine    the part of DDRateEngine's / TrendRateEngine's surface the run loop and the writers use, on
                                 lr_parbin_*
    pooled_summary               --summary over all replicates, from lr_col_summary / lr_curve_summary / lr_dd_rates alone
    replicates_table             <stem>_replicates.tsv: every replicate's own means beside their spread (logAverager.py per
                                 imputation)
    run                          DDRate.py / trend_rate.py --replicates: the reference's log per replicate beside its own file,
                                 the pooled outputs beside the first one
"""
import os
import sys
import time

import numpy as np

from . import _hip
from .replicates import (ESS_NOTE, ONE_DATA_SET, chains_per_replicate, default_name, expand_pattern, replicate_of,
                         write_div_replicates)

MAX_BINS = _hip.LR_PARBIN_MAX_BINS
REPLICATES_HEAD = ["replicate", "file", "parameter", "mean", "minHPD", "maxHPD", "sd_of_means_between_replicates"]
# flags that need ONE data set: replicates.ONE_DATA_SET's, and the marginal likelihood
REFUSED = ONE_DATA_SET + [
    ("mlik", -1.0, "--mlik runs its temperature ladder on one data set's statistics: not with --replicates"),
]


def arg_error(args, world=1):
    """Why DDRate.py / trend_rate.py --replicates cannot run with these flags (None when it can), one sentence each."""
    if args.d:
        return "--replicates names the data files itself: leave -d empty"
    for name, off, why in REFUSED:
        if getattr(args, name, off) != off:
            return why
    if world > 1:
        return "--replicates runs on one GPU (WORLD_SIZE is %d): all chains of all replicates are one launch" % world
    if args.chains < 1:
        return "--chains must be at least 1"
    return None


def _bin(origin, present, ts, te, rm_first_bin):
    """create_bins of one file (binned on the GPU): (origin, present, n_spec, n_exti, DT, n_bins, time_range) - the seam the
    host tests replace"""
    from .literate_library import create_bins
    return create_bins(origin, present, ts, te, rm_first_bin)


def _parse(path, args):
    from .literate_library import parse_ts_te
    return parse_ts_te(path, args.TBP, args.first_year, args.last_year, args.death_jitter)


class BinnedReplicates:
    """What load_binned_replicates returns: paths [R]; n_spec, n_exti, DT [R, n_bins] float64; origin, present (create_bins',
    after -rm_first_bin), n_lineages [R]; trend [n_bins] or None, the normalised covariate all replicates share."""

    def __init__(self, paths, n_spec, n_exti, DT, origin, present, n_lineages=None, trend=None):
        self.paths = list(paths)
        self.n_spec, self.n_exti, self.DT = [np.ascontiguousarray(np.atleast_2d(np.asarray(x, dtype=np.float64))) for x in (n_spec, n_exti, DT)]
        self.origin, self.present = np.asarray(origin, dtype=np.float64).reshape(-1), np.asarray(present, dtype=np.float64).reshape(-1)
        self.R, self.n_bins = int(self.DT.shape[0]), int(self.DT.shape[1])
        self.n_lineages = np.zeros(self.R, dtype=np.int64) if n_lineages is None else np.asarray(n_lineages, dtype=np.int64)
        self.trend = None if trend is None else np.ascontiguousarray(trend, dtype=np.float64)
        if self.n_spec.shape != self.DT.shape or self.n_exti.shape != self.DT.shape or self.origin.size != self.R or self.present.size != self.R:
            raise ValueError("shape mismatch: n_spec, n_exti, DT [R, n_bins]; origin, present [R]")
        if self.trend is not None and self.trend.size != self.n_bins:
            raise ValueError("the trend has %d entries, the replicates %d time bins" % (self.trend.size, self.n_bins))

    def empirical(self, r):
        """(B_EMP, D_EMP) of replicate r, as the CLIs compute them (print_empirical_rates)"""
        with np.errstate(all="ignore"):
            return self.n_spec[r] / self.DT[r], self.n_exti[r] / self.DT[r]


def load_binned_replicates(paths, args, parse=None, trend=None):
    """Every file through parse_ts_te and create_bins, the CLIs' own path (parse(path, args) -> (ts, te, PRESENT, ORIGIN) to
    replace the first).  The number of time bins must be common to all files (ValueError naming the first one that differs and
    both counts) and at most 512; origin, present, the lineage counts and all statistics may differ."""
    parse = parse or _parse
    rows = {k: [] for k in ("ns", "ne", "dt", "o", "p", "n")}
    nb0 = None
    for path in paths:
        ts, te, present, origin = parse(path, args)
        ts, te = np.asarray(ts, dtype=float), np.asarray(te, dtype=float)
        origin, present, n_spec, n_exti, DT, nb, _ = _bin(origin, present, ts, te, int(args.rm_first_bin))
        if nb0 is None:
            nb0 = nb
            if nb < 1:
                raise ValueError("%s: no time bin" % path)
            if nb > MAX_BINS:
                raise ValueError("%s: %d time bins; the replicate sampler holds at most %d" % (path, nb, MAX_BINS))
        elif nb != nb0:
            raise ValueError("%s: %d time bins, the first replicate (%s) has %d: replicates must share their number of time bins"
                             % (path, nb, paths[0], nb0))
        rows["ns"].append(np.asarray(n_spec, dtype=float)), rows["ne"].append(np.asarray(n_exti, dtype=float))
        rows["dt"].append(np.asarray(DT, dtype=float)), rows["o"].append(float(origin)), rows["p"].append(float(present))
        rows["n"].append(ts.size)
    if nb0 is None:
        raise ValueError("no replicate given")
    return BinnedReplicates(list(paths), np.array(rows["ns"]), np.array(rows["ne"]), np.array(rows["dt"]), rows["o"], rows["p"],
                            rows["n"], trend)


def _engine_class(sampler):
    if sampler == 1:
        from .ddrate import DDRateEngine as E
    else:
        from .trendrate import TrendRateEngine as E
    return E


class ReplicateLog:
    """One replicate's statistics with the engines' own log code on them: log_head, log_table_from, start_log and append_logs
    are DDRateEngine's / TrendRateEngine's functions, which read origin, DT, n_spec, n_exti and the model of `self` alone."""

    def __init__(self, sampler, reps, r, m_birth, m_death):
        self.sampler = int(sampler)
        self.origin, self.present = float(reps.origin[r]), float(reps.present[r])
        self.n_spec, self.n_exti, self.DT = reps.n_spec[r], reps.n_exti[r], reps.DT[r]
        if self.sampler == 1:
            self.m_birth, self.m_death = int(m_birth), int(m_death)
        else:
            self.trend, self.const_birth, self.const_death = reps.trend, bool(m_birth), bool(m_death)
        self._E = _engine_class(self.sampler)

    def log_head(self):
        return self._E.log_head(self)

    def log_table_from(self, tr, emp=None):
        return self._E.log_table_from(self, tr, emp)

    def start_log(self, path):
        return self._E.start_log(self, path)

    def append_logs(self, paths, rows, emp=None):
        return self._E.append_logs(self, paths, rows, emp)


def log_names(sampler, m_birth, m_death, no_death=False, trend_index=0):
    """(model suffix, what follows the chain tag in a log's name, what follows the suffix in the pooled stem)"""
    if sampler == 1:
        from .ddrate import model_suffix
        return model_suffix(m_birth, m_death), ".log", ""
    from .trendrate import model_suffix
    return model_suffix(bool(m_birth), bool(m_death), bool(no_death)), "_%s.trendrate.log" % trend_index, "_%s" % trend_index


def replicate_log_paths(path, seed, suffix, tail, chains_per_rep):
    """[per chain of the replicate] the CLI's own log name beside the file: <file stem>_<seed><suffix><tail>, _c<k> before the
    tail with more than one chain each, k counted within the replicate"""
    stem = "%s_%s%s" % (os.path.splitext(path)[0], seed, suffix)
    return [stem + ("" if chains_per_rep == 1 else "_c%d" % k) + tail for k in range(chains_per_rep)]


class ParametricReplicateEngine:
    """Chains of DDRate.py's (sampler 1) or trend_rate.py's (sampler 2) loop on replicate data sets: chain c samples the
    posterior of replicate c // chains_per_rep with the Philox key (seed, chain_offset + c).  The surface is the part of
    DDRateEngine's / TrendRateEngine's that the run loop and the writers use; the trace [n_trace_slots, C, LR_TRACE_W] is
    resident and has those engines' row layout.  m_birth, m_death: -m_birth / -m_death, or -const_B / -const_D."""

    def __init__(self, reps, n_chains, sampler=1, m_birth=2, m_death=2, init_death=0.1, seed=1, s_freq=1000, n_trace_slots=0,
                 chain_offset=0, device=None):
        from . import ops
        torch = _hip.require_gpu()
        if sampler not in (1, 2):
            raise ValueError("sampler 1 (DDRate) or 2 (trend_rate)")
        if sampler == 2 and reps.trend is None:
            raise ValueError("trend_rate needs the replicates' shared covariate (reps.trend)")
        self.reps, self.sampler = reps, int(sampler)
        self.chains_per_rep = chains_per_replicate(int(n_chains), reps.R)
        self.data = ops.ParbinData(reps.n_spec, reps.n_exti, reps.DT, reps.origin, reps.present, self.chains_per_rep,
                                   reps.trend if sampler == 2 else None, device)
        self.device = self.data.device
        self.settings = ops.ParbinSettings(self.sampler, int(m_birth), int(m_death), float(init_death))
        self.m_birth, self.m_death = int(m_birth), int(m_death)
        self.seed, self.chain_offset, self.s_freq, self.n_trace_slots = int(seed), int(chain_offset), int(s_freq), int(n_trace_slots)
        self.n_chains, self.n_bins, self.npar = int(n_chains), reps.n_bins, ops.PARBIN_NPAR[self.sampler]
        self.trace = ops.alloc_output((self.n_trace_slots, self.n_chains, _hip.LR_TRACE_W), torch.float64, self.device, zero=True)
        # the origin of every chain's replicate (ess_rows: x0 + ORIGIN)
        self.chain_origin = torch.as_tensor(np.repeat(reps.origin, self.chains_per_rep), dtype=torch.float64).to(self.device)
        self.logs = [ReplicateLog(self.sampler, reps, r, m_birth, m_death) for r in range(reps.R)]
        self.state = None
        self.iterations = 0

    def replicate_of(self, chain):
        return replicate_of(chain, self.chains_per_rep)

    def chains_of(self, r):
        return slice(r * self.chains_per_rep, (r + 1) * self.chains_per_rep)

    def init(self):
        from . import ops
        self.state = ops.parbin_init(self.data, self.seed, self.settings, self.chain_offset)
        self.iterations = 0

    def samples_done(self):
        """Trace rows written so far: iterations 0, s, 2 s, ... below `iterations`"""
        return min(self.n_trace_slots, (self.iterations + self.s_freq - 1) // self.s_freq)

    def steps(self, n):
        from . import ops
        if self.state is None:
            raise _hip.HipLibraryError("ParametricReplicateEngine.steps before init")
        n = int(n)
        due = ops.rows_due(self.iterations, n, self.s_freq) if n > 0 else 0
        slot0 = (self.iterations + self.s_freq - 1) // self.s_freq
        if slot0 + due > self.n_trace_slots:
            raise ValueError("the trace holds %d samples; %d iterations from %d on sample up to row %d" %
                             (self.n_trace_slots, n, self.iterations, slot0 + due))
        ops.parbin_steps(self.data, self.state, self.iterations, n, self.s_freq, self.seed, self.settings, self.chain_offset,
                         rows=self.trace, slot0=slot0)
        self.iterations += n

    def check_status(self):
        """Synchronise (the kernel has no waits between blocks, so there is no status word to read)"""
        import torch
        torch.cuda.synchronize(self.device)

    def snapshot(self):
        """the accepted state of every chain as host arrays, by name (L: the parameter vectors, as the engines' snapshot)"""
        from .ops import PARBIN_STATE as X
        S = self.state.cpu().numpy()
        return dict(L=[S[c, :self.npar] for c in range(self.n_chains)], likA=S[:, X["lik"]], priorA=S[:, X["prior"]],
                    proposed=S[:, X["proposed"]:X["proposed"] + 2].astype(np.int64),
                    accepted=S[:, X["accepted"]:X["accepted"] + 2].astype(np.int64))

    def ess_rows(self, rows):
        """The engines' ess_rows on rows [samples, C, LR_TRACE_W]: for DDRate the first 12 columns with midpoint_x0 + ORIGIN
        of the chain's OWN replicate and maxCarryingCap = L + div_0, as the log holds them; for trend_rate the rows as they are."""
        E = _engine_class(self.sampler)
        if self.sampler == 2:
            return E.ess_rows(self, rows)
        from .ddrate import LOG_HEAD
        out = rows[..., :12].clone()
        out[..., 6] += self.chain_origin.to(out.device)          # DD:224, per chain
        out[..., 8] += out[..., 7]                               # DD:225
        return out, list(range(1, 12)), ["it", "posterior", "likelihood", "prior"] + LOG_HEAD[6:14]

    def ess_summary(self, burnin=0.1, columns=None, max_lag=2000):
        from . import ops
        self.check_status()
        S = self.samples_done()
        rows, cols, head = self.ess_rows(self.trace[:S])
        if columns is not None:
            cols = [int(c) for c in columns]
        return ops.ess_summary(rows, S, cols, burnin, max_lag), [head[c] for c in cols]

    def trace_rows(self, n_samples=None):
        self.check_status()
        n_avail = self.samples_done()
        n = n_avail if n_samples is None else min(n_samples, n_avail)
        return self.trace[:n].cpu().numpy()

    def close(self):
        self.state = self.trace = self.data = self.chain_origin = None


def _ops():
    """literate_amd.ops (the seam the host tests replace with numpy stand-ins of col_summary, curve_summary and dd_rates)"""
    from . import ops
    return ops


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _triples(cs):
    """ColSummary of one group -> [columns, (mean, lo, hi)] on the host"""
    return np.stack([_host(cs.mean)[0], _host(cs.lo)[0], _host(cs.hi)[0]], axis=1)


def pooled_summary(eng, burnin):
    """--summary over all chains of all replicates -> (kinds, values [kinds, (mean, lo, hi), n_bins], names, params [columns,
    (mean, lo, hi)]), from existing kernels only.  Parameters: lr_col_summary pooled over ess_rows' table (after the origin
    and div_0 shifts).  trend_rate curves: lr_curve_summary pooled, the covariate being shared.  DDRate curves: a row's
    per-bin rates depend on its replicate's DT, so the [S, C, n_bins] table of every kind (lr_curve_summary's five) is formed
    by lr_dd_rates on each replicate's chain slice and summarised by lr_col_summary pooled, the columns being the bins."""
    import torch
    o = _ops()
    S = eng.samples_done()
    trace = eng.trace[:S]
    table, cols, head = eng.ess_rows(trace)
    params = _triples(o.col_summary(table, S, cols, burnin, True))
    names = [head[c] for c in cols]
    nb = eng.n_bins
    if eng.sampler == 2:
        cur = o.curve_summary(trace, S, 2, eng.reps.trend, eng.m_birth, eng.m_death, 4, burnin, True)
        return tuple(cur.kinds), _host(cur.values)[0], names, params
    kinds = tuple(o.CURVE_KINDS[1])
    tabs = [torch.empty((S, eng.n_chains, nb), dtype=torch.float64, device=trace.device) for _ in kinds]
    for r in range(eng.reps.R):
        sl = eng.chains_of(r)
        args = trace[:, sl, 4:12].reshape(-1, 8).contiguous()
        b, d, niche, frac = o.dd_rates(args, eng.reps.DT[r], eng.m_birth, eng.m_death)
        for t, x in zip(tabs, (b, d, b - d, niche, frac)):          # lr_curve_summary's kinds: birth, death, net, niche, nicheFrac
            t[:, sl] = x.reshape(S, -1, nb)
    values = np.stack([_triples(o.col_summary(t, S, list(range(nb)), burnin, True)).T for t in tabs], axis=0)
    return kinds, values, names, params


def replicates_table(eng, burnin):
    """(names [K], triples [R, K, (mean, lo, hi)], sd [K]): mean and 95 % HPD of every logged parameter over the pooled chains
    of each replicate (lr_col_summary on its chain slice: utilities/logAverager.py per imputation), and the standard deviation
    (ddof 1; nan with one replicate) of the replicates' means: do the imputations disagree?"""
    o = _ops()
    S = eng.samples_done()
    table, cols, head = eng.ess_rows(eng.trace[:S])
    tri = np.stack([_triples(o.col_summary(table[:, eng.chains_of(r)].contiguous(), S, cols, burnin, True))
                    for r in range(eng.reps.R)], axis=0)
    with np.errstate(all="ignore"):
        sd = np.std(tri[:, :, 0], axis=0, ddof=1) if eng.reps.R > 1 else np.full(tri.shape[1], np.nan)
    return [head[c] for c in cols], tri, sd


def write_replicates_table(path, files, names, tri, sd):
    with open(path, "w") as f:
        f.write("\t".join(REPLICATES_HEAD) + "\n")
        for r, name_r in enumerate(files):
            for k, name in enumerate(names):
                f.write("\t".join(["%d" % r, os.path.basename(name_r), name] + [str(float(v)) for v in tri[r, k]] + [str(float(sd[k]))]) + "\n")


def write_pooled_summary(stem, reps, kinds, values, names, params):
    """<stem>_summary.tsv and <stem>_summary_params.tsv in logs.write_summary_tables' layout; time (origin + i + 0.5),
    net_diversity (DT) and the empirical rates (N / DT per replicate, the first entry nan) are the MEANS over replicates."""
    from . import logs
    with np.errstate(all="ignore"):
        emp_b, emp_d = (reps.n_spec / reps.DT).mean(axis=0), (reps.n_exti / reps.DT).mean(axis=0)
    emp_b[0] = emp_d[0] = np.nan
    nb = reps.n_bins
    head = ["time", "net_diversity", "emp_birth", "emp_death"]
    cols = [float(np.mean(reps.origin)) + np.arange(nb) + .5, reps.DT.mean(axis=0), emp_b, emp_d]
    for kind in logs.SUMMARY_KIND_ORDER:
        if kind in kinds:
            head += logs.SUMMARY_KIND_HEAD[kind]
            cols += [values[list(kinds).index(kind), s] for s in range(3)]
    with open(stem + "_summary.tsv", "w") as f:
        f.write("\t".join(head) + "\n")
        for i in range(nb):
            f.write("\t".join(str(float(c[i])) for c in cols) + "\n")
    with open(stem + "_summary_params.tsv", "w") as f:
        f.write("\t".join(logs.SUMMARY_PARAM_HEAD) + "\n")
        for k, name in enumerate(names):
            f.write("\t".join([name] + [str(float(v)) for v in params[k]]) + "\n")


def run(args, sampler):
    """DDRate.py (sampler 1) / trend_rate.py (sampler 2) --replicates PATTERN: every chain of every replicate in one engine;
    the reference's own log per replicate beside its own file, flushed per --block window; the pooled outputs (--summary,
    --ess, <NAME>_div_replicates.tsv) beside the first file, stem <NAME>_<seed><model suffix>."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    err = arg_error(args, world)
    if err:
        raise SystemExit(err)
    from . import logs
    try:
        files = expand_pattern(args.replicates)
        cpr = chains_per_replicate(args.chains, len(files))
    except ValueError as e:
        raise SystemExit(str(e))
    for flag, check in (("ess", lambda: logs.ess_arg_error(args.ess, args.n, args.s)),
                        ("summary", lambda: logs.summary_arg_error(args.summary, args.n, args.s, cpr))):
        if getattr(args, flag) != -1.0 and check():
            raise SystemExit(check())
    import torch
    from .literate_library import set_seed
    seed = set_seed(args.seed)
    if sampler == 1:
        m_birth, m_death, no_death, trend, tix = args.m_birth, args.m_death, False, None, 0
    else:
        from .trendrate import parse_trend_data
        no_death, tix = bool(args.no_death), args.trend_index
        m_birth, m_death = int(bool(args.const_B)), int(True if args.no_death else bool(args.const_D))          # trend_rate.py:42-44
        trend = parse_trend_data(args.trend_data, args.trend_index, args.rm_first_bin)
    try:
        reps = load_binned_replicates(files, args, trend=trend)
    except ValueError as e:
        raise SystemExit(str(e))
    R = len(files)
    suffix, tail, pooled_tail = log_names(sampler, m_birth, m_death, no_death, tix)
    name = args.replicates_name or default_name(R)
    n_samples = (args.n + args.s - 1) // args.s if args.n > 0 else 0
    eng = ParametricReplicateEngine(reps, args.chains, sampler=sampler, m_birth=m_birth, m_death=m_death,
                                    init_death=getattr(args, "fix_death", 0.1), seed=seed, s_freq=args.s, n_trace_slots=n_samples)
    print("%d replicates, %d chains each, %d time bins" % (R, cpr, reps.n_bins))
    paths = [replicate_log_paths(path, seed, suffix, tail, cpr) for path in files]
    emps = [reps.empirical(r) for r in range(R)]
    for r in range(R):
        for path in paths[r]:
            eng.logs[r].start_log(path)
    dir0 = os.path.dirname(files[0])
    base = os.path.join(dir0, name)
    stem = "%s_%s%s%s" % (base, seed, suffix, pooled_tail)
    write_div_replicates(base + "_div_replicates.tsv", reps.n_spec, reps.n_exti, reps.DT)
    eng.init()
    done, s_done = 0, 0
    t_start = time.time()
    block = args.block if args.block > 0 else args.p * max(1, 50000 // max(args.p, 1))
    while done < args.n:
        n = min(block, args.n - done)
        eng.steps(n)
        done += n
        s1 = eng.samples_done()
        rows = eng.trace[s_done:s1].cpu().numpy()          # (synchronises: the window has run)
        for r in range(R):
            eng.logs[r].append_logs(paths[r], np.ascontiguousarray(rows[:, eng.chains_of(r)]), emps[r])
        s_done = s1
        snap = eng.snapshot()
        print(done, snap["likA"][0], snap["L"][0])
        sys.stdout.flush()
    eng.check_status()
    if args.n > 0:
        el = time.time() - t_start
        print("%d iterations x %d chains in %.2f s (%.0f iterations/s/chain)" % (args.n, args.chains, el, args.n / el))
    if args.ess != -1.0 and n_samples:
        logs.write_run_ess(eng, args.chains, args.chains, 1, 0, args.ess, args.s, stem)
        with open(stem + "_ESS.tsv") as f:
            body = f.read()
        with open(stem + "_ESS.tsv", "w") as f:
            f.write(ESS_NOTE % (R, cpr) + body)
    if args.summary != -1.0 and n_samples:
        kinds, values, names, params = pooled_summary(eng, args.summary)
        write_pooled_summary(stem, reps, kinds, values, names, params)
        names, tri, sd = replicates_table(eng, args.summary)
        write_replicates_table(stem + "_replicates.tsv", files, names, tri, sd)
        print("posterior summary over %d replicates (%d chains pooled): %s_summary.tsv, _summary_params.tsv, _replicates.tsv" %
              (R, args.chains, stem))
    eng.close()
    torch.cuda.synchronize()
