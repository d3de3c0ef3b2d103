"""The RJ sampler on many replicate data sets in one launch (include/literate_hip_rjbin.h, csrc/lr_rjbin.hip).

An analysis whose death times are uncertain runs LiteRateForward.py once per stochastic imputation of them (the
reference's metal_bands example: 100 runs), pools the logs (plotRJforward.v3.py -combine, utilities/logCombiner.py) and
averages the div logs (utilities/imputation_averager.py).  The likelihood of runMCMC is a function of the per-bin
statistics alone, so here every chain carries the statistics of its own replicate and all chains of all replicates run in
one kernel:

    load_replicates    the files parsed by the CLI's rules and binned on the GPU on one common window
    ReplicateEngine    the part of ChainEngine's surface the run loop and the writers use, on lr_rjbin_*
    run                LiteRateForward.py --replicates: per-replicate logs under each file's own directory, the pooled
                       summaries under the first one's
"""
import copy
import glob
import os
import shutil
import sys
import tempfile
import time

import numpy as np

from . import _hip

MAX_BINS = _hip.LR_RJBIN_MAX_BINS
DIV_HEAD = ["bin", "emp_birth_mean", "emp_birth_min", "emp_birth_max", "emp_death_mean", "emp_death_min", "emp_death_max",
            "br_length_mean", "br_length_min", "br_length_max"]
ESS_NOTE = ("# chains of %d replicate data sets (%d each): split R-hat compares chains across replicates, so beside the "
            "sampler's convergence it also contains the between-imputation variance\n")
# flags that need ONE data set: (attribute, the value that leaves it off, why)
ONE_DATA_SET = [
    ("ppc", -1.0, "--ppc simulates forward from one data set's observed diversity: not with --replicates"),
    ("ppc_age", -1.0, "--ppc_age gives the lineages of one data set new death times: not with --replicates"),
    ("ade", -1.0, "--ade fits the Weibull shape to the lifespans of one data set: not with --replicates"),
    ("ade_joint", -1.0, "--ade_joint samples on the lineages of one data set: not with --replicates"),
    ("waic", -1.0, "--waic scores the lineages of one data set, and replicates differ in theirs: not with --replicates"),
    ("loo", -1.0, "--loo scores the lineages of one data set, and replicates differ in theirs: not with --replicates"),
]


def expand_pattern(pattern):
    """--replicates PATTERN -> the files, sorted: a comma-separated list of paths and / or globs (each expanded here, not
    by the shell).  A name that matches nothing is an error that names it."""
    files = []
    for part in [p.strip() for p in str(pattern).split(",") if p.strip()]:
        hits = glob.glob(part) if glob.has_magic(part) else ([part] if os.path.exists(part) else [])
        if not hits:
            raise ValueError("--replicates: no file matches %r" % part)
        files += hits
    files = sorted(set(os.path.normpath(f) for f in files))
    if not files:
        raise ValueError("--replicates: no file given")
    return files


def arg_error(args, world=1):
    """Why LiteRateForward.py --replicates cannot run with these flags (None when it can), one sentence each."""
    if args.d:
        return "--replicates names the data files itself: leave -d empty"
    for name, off, why in ONE_DATA_SET:
        if getattr(args, name, off) != off:
            return why
    if getattr(args, "checkpoint", ""):
        return "--checkpoint saves one engine's workspace, which the replicate sampler does not have: not with --replicates"
    if getattr(args, "init_shifts", 0):
        return "--init_shifts spaces its shifts over one data set's time span: not with --replicates"
    if world > 1:
        return "--replicates runs on one GPU (WORLD_SIZE is %d): all chains of all replicates are one launch" % world
    if getattr(args, "rm_first_bin", 0):
        return ("-rm_first_bin 1 makes the reference's own sampler fail with IndexError at the first K>=2 proposal "
                "(SURVEY.md section 8a A13); not supported")
    if args.chains < 1:
        return "--chains must be at least 1"
    return None


def chains_per_replicate(n_chains, n_files):
    """--chains is the total over all replicates: a multiple of the number of files, or ValueError"""
    if n_files < 1 or n_chains < n_files or n_chains % n_files:
        raise ValueError("--chains %d is the total over all replicates: it must be a multiple of the %d files" % (n_chains, n_files))
    return n_chains // n_files


def replicate_of(chain, chains_per_rep):
    """the replicate chain `chain` belongs to (chain c of the kernel reads replicate c // chains_per_rep)"""
    return int(chain) // int(chains_per_rep)


def default_name(n_files):
    return "replicates%d" % n_files


def _bin(ts, te, t0, n_bins):
    """(sp, ex, br) [n_bins] of the unit windows from t0 on, binned on the GPU (the seam the host tests replace)"""
    from . import ops
    return [x.cpu().numpy() for x in ops.bin_unit_events(ts, te, float(t0), int(n_bins))]


def _bin_dead(ts, te, t0, n_bins, end_time):
    """(ex_dead, br_dead) [n_bins]: the te < end_time subset on the same windows (LRF:529-546)"""
    keep = te < end_time
    if not keep.any():
        return np.zeros(n_bins), np.zeros(n_bins)
    _, ex, br = _bin(ts[keep], te[keep], t0, n_bins)
    return ex, br


class Replicates:
    """What load_replicates returns: paths [R]; sp, ex, br (and ex_dead, br_dead for model 3, else None) [R, n_bins] float64;
    start_time, end_time, true_root_age, n_lineages [R]; t0, n_bins of the common window."""

    def __init__(self, paths, sp, ex, br, start_time, end_time, t0, ex_dead=None, br_dead=None, true_root_age=None, n_lineages=None):
        self.paths = list(paths)
        self.sp, self.ex, self.br = [np.ascontiguousarray(x, dtype=np.float64) for x in (sp, ex, br)]
        self.ex_dead = None if ex_dead is None else np.ascontiguousarray(ex_dead, dtype=np.float64)
        self.br_dead = None if br_dead is None else np.ascontiguousarray(br_dead, dtype=np.float64)
        self.start_time, self.end_time = np.asarray(start_time, dtype=np.float64), np.asarray(end_time, dtype=np.float64)
        self.R, self.n_bins, self.t0 = int(self.sp.shape[0]), int(self.sp.shape[1]), int(t0)
        self.true_root_age = np.zeros(self.R) if true_root_age is None else np.asarray(true_root_age, dtype=float)
        self.n_lineages = np.zeros(self.R, dtype=np.int64) if n_lineages is None else np.asarray(n_lineages, dtype=np.int64)

    @classmethod
    def from_lineages(cls, data, model=0, paths=None):
        """data: [(ts, te)] per replicate, te with its jitter -> Replicates (binned through the same seam)"""
        return _assemble(paths or ["replicate%d" % r for r in range(len(data))], [(ts, te, 0.0) for ts, te in data], model)

    @classmethod
    def from_counts(cls, sp, ex, br, start_time, end_time, t0=0, paths=None):
        """Per-bin statistics that somebody else has counted - a simulator's, say - as they are: sp, ex, br [R, n_bins] (or
        [n_bins]: one replicate), start_time / end_time: one value for all replicates or [R] -> Replicates (model 0 - 2:
        no ex_dead, br_dead)."""
        sp, ex, br = [np.atleast_2d(np.asarray(x, dtype=np.float64)) for x in (sp, ex, br)]
        if sp.ndim != 2 or sp.shape != ex.shape or sp.shape != br.shape or sp.shape[0] < 1:
            raise ValueError("sp, ex and br must share their shape [R, n_bins]")
        R, nb = sp.shape
        if nb < 1 or nb > MAX_BINS:
            raise ValueError("%d time bins; the replicate sampler holds 1 to %d" % (nb, MAX_BINS))
        if not (np.all(np.isfinite(sp)) and np.all(np.isfinite(ex)) and np.all(np.isfinite(br))) or (sp < 0).any() or (ex < 0).any() \
                or (br < 0).any():
            raise ValueError("sp, ex and br must be finite and not negative")
        start, end = [np.broadcast_to(np.asarray(x, dtype=np.float64), (R,)).copy() for x in (start_time, end_time)]
        if not np.all(end > start):
            raise ValueError("every end_time must lie after its start_time")
        paths = list(paths) if paths is not None else ["replicate%d" % r for r in range(R)]
        if len(paths) != R:
            raise ValueError("paths names %d replicates, the statistics hold %d" % (len(paths), R))
        return cls(paths, sp, ex, br, start, end, t0)

    def empirical(self, r):
        """(B_EMP, D_EMP) of replicate r, as the CLI computes them (LRF:566-568)"""
        with np.errstate(all="ignore"):
            return self.sp[r] / self.br[r], self.ex[r] / self.br[r]


def _assemble(paths, parsed, model):
    if not parsed:
        raise ValueError("no replicate given")
    rows = {k: [] for k in ("sp", "ex", "br", "exd", "brd", "start", "end", "root", "n")}
    lo0 = hi0 = None
    for path, (ts, te, root) in zip(paths, parsed):
        ts, te = np.asarray(ts, dtype=float), np.asarray(te, dtype=float)
        if ts.size == 0 or ts.size != te.size:
            raise ValueError("%s: no lineages (or ts and te differ in length)" % path)
        lo, hi = int(np.min(ts)), int(np.max(te))
        if lo0 is None:
            lo0, hi0 = lo, hi
            if hi - lo < 1:
                raise ValueError("%s: the window [%d, %d] holds no unit bin" % (path, lo, hi))
            if hi - lo > MAX_BINS:
                raise ValueError("%s: %d time bins; the replicate sampler holds at most %d" % (path, hi - lo, MAX_BINS))
        elif (lo, hi) != (lo0, hi0):
            raise ValueError("%s: its window [%d, %d] (int(min ts), int(max te)) differs from the first replicate's [%d, %d] "
                             "(%s): replicates must share their time bins" % (path, lo, hi, lo0, hi0, paths[0]))
        nb = hi0 - lo0
        sp, ex, br = _bin(ts, te, lo0, nb)
        rows["sp"].append(sp), rows["ex"].append(ex), rows["br"].append(br)
        rows["start"].append(float(np.min(ts))), rows["end"].append(float(np.max(te)))
        rows["root"].append(float(root)), rows["n"].append(ts.size)
        if model == 3:
            exd, brd = _bin_dead(ts, te, lo0, nb, float(np.max(te)))
            rows["exd"].append(exd), rows["brd"].append(brd)
    return Replicates(paths, np.array(rows["sp"], dtype=float), np.array(rows["ex"], dtype=float), np.array(rows["br"], dtype=float),
                      rows["start"], rows["end"], lo0, np.array(rows["exd"], dtype=float) if model == 3 else None,
                      np.array(rows["brd"], dtype=float) if model == 3 else None, rows["root"], rows["n"])


def load_replicates(paths, args, parse=None):
    """Parse every file by the CLI's rules (parse(args with .d = the file) -> (ts, te, true_root_age); default:
    LiteRateForward.parse_data) and bin it on the GPU on the FIRST file's windows; for -model_BDI 3 also the te < end_time
    subset.  The window - int(min ts), int(max te) - must be common to all files (ValueError naming the one that differs);
    lineage counts, start_time and end_time may differ.  At most 512 bins."""
    if parse is None:
        from LiteRateForward import parse_data as parse
    parsed = []
    for path in paths:
        a = copy.copy(args)
        a.d = path
        parsed.append(parse(a))
    return _assemble(list(paths), parsed, int(args.model_BDI))


class ReplicateEngine:
    """Chains of runMCMC on replicate data sets: chain c samples the posterior of replicate c // chains_per_rep.  The
    surface is the part of ChainEngine's that the run loop and the writers use; the trace [n_trace_slots, C, LR_TRACE_W] is
    resident and has the engines' row layout.  start_time / end_time: the smallest / largest over the replicates (what the
    pooled summaries bin over); a row's columns 8, 9 hold its own replicate's."""

    def __init__(self, reps, n_chains, model=0, seed=1, const_rates=0, const_death_rate=0, use_rate_HP=1, poisson_HP=0.0,
                 update_fraction=0.75, s_freq=1000, n_trace_slots=0, chain_offset=0, device=None):
        from . import ops
        torch = _hip.require_gpu()
        self.reps = reps
        self.chains_per_rep = chains_per_replicate(int(n_chains), reps.R)
        if model == 3 and (reps.ex_dead is None or reps.br_dead is None):
            raise ValueError("model 3 needs the replicates' ex_dead and br_dead")
        self.data = ops.RjbinData(reps.sp, reps.ex, reps.br, reps.start_time, reps.end_time, self.chains_per_rep,
                                  reps.ex_dead if model == 3 else None, reps.br_dead if model == 3 else None, device)
        self.device = self.data.device
        self.settings = ops.RjbinSettings(int(model), int(const_rates), int(const_death_rate), int(use_rate_HP), float(poisson_HP),
                                          float(update_fraction))
        self.seed, self.chain_offset, self.s_freq, self.n_trace_slots = int(seed), int(chain_offset), int(s_freq), int(n_trace_slots)
        self.n_chains, self.n_bins, self.model, self.t0 = int(n_chains), reps.n_bins, int(model), float(reps.t0)
        self.start_time, self.end_time = float(np.min(reps.start_time)), float(np.max(reps.end_time))
        self.trace = ops.alloc_output((self.n_trace_slots, self.n_chains, _hip.LR_TRACE_W), torch.float64, self.device, zero=True)
        self.state = None
        self.iterations = 0

    def replicate_of(self, chain):
        return replicate_of(chain, self.chains_per_rep)

    def init(self, L=None, M=None, tL=None, tM=None):
        """Initial state: None = the CLI's (K = 1, Gamma(2, 2) rates, times [start_time, end_time] of the chain's replicate);
        else per-chain lists as ChainEngine.init takes them."""
        from . import ops
        init = None
        if L is not None:
            C, K = self.n_chains, _hip.LR_KMAX
            Ls, Ms, tLs, tMs = np.zeros((C, K)), np.zeros((C, K)), np.zeros((C, K + 1)), np.zeros((C, K + 1))
            KL, KM = np.zeros(C, dtype=np.int32), np.zeros(C, dtype=np.int32)
            for c in range(C):
                l, m = np.atleast_1d(L[c]), np.atleast_1d(M[c])
                KL[c], KM[c] = len(l), len(m)
                Ls[c, :len(l)], Ms[c, :len(m)] = l, m
                tLs[c, :len(l) + 1], tMs[c, :len(m) + 1] = tL[c], tM[c]
            init = (Ls, Ms, tLs, tMs, KL, KM)
        self.data.warn.zero_()
        self.state = ops.rjbin_init(self.data, self.seed, self.settings, self.chain_offset, init=init)
        self.iterations = 0

    def samples_done(self):
        """Trace rows written so far: iterations 0, s, 2 s, ... below `iterations`"""
        return min(self.n_trace_slots, (self.iterations + self.s_freq - 1) // self.s_freq)

    def steps(self, n):
        from . import ops
        if self.state is None:
            raise _hip.HipLibraryError("ReplicateEngine.steps before init")
        n = int(n)
        due = ops.rows_due(self.iterations, n, self.s_freq) if n > 0 else 0
        slot0 = (self.iterations + self.s_freq - 1) // self.s_freq
        if slot0 + due > self.n_trace_slots:
            raise ValueError("the trace holds %d samples; %d iterations from %d on sample up to row %d" %
                             (self.n_trace_slots, n, self.iterations, slot0 + due))
        ops.rjbin_steps(self.data, self.state, self.iterations, n, self.s_freq, self.seed, self.settings, self.chain_offset,
                        rows=self.trace, slot0=slot0)
        self.iterations += n

    def check_status(self):
        """Synchronise (the kernel has no waits between blocks, so there is no status word to read)"""
        import torch
        torch.cuda.synchronize(self.device)

    def warnings(self):
        return self.data.warnings()

    def warning_text(self):
        if self.warnings() & _hip.LR_WARN_KCAP:
            return ("WARNING: an add-shift move was proposed from a state with %d rates and rejected: the device holds at "
                    "most %d rates per process (the reference has no cap, LiteRateForward.py:29-47); the posterior of "
                    "the number of shifts is truncated there" % (_hip.LR_KMAX, _hip.LR_KMAX))
        return ""

    def snapshot(self):
        """the accepted state of every chain as host arrays (ragged rows), by name"""
        S = self.state.cpu().numpy().reshape(self.n_chains, -1, _hip.LR_ROW)
        from .ops import RJBIN_ROWS as R, RJBIN_SCALARS as X
        sc = S[:, R["scalars"]]
        KL, KM = sc[:, X["K_l"]].astype(int), sc[:, X["K_m"]].astype(int)
        return dict(L=[S[c, R["L"], :KL[c]] for c in range(self.n_chains)], M=[S[c, R["M"], :KM[c]] for c in range(self.n_chains)],
                    tL=[S[c, R["tL"], :KL[c] + 1] for c in range(self.n_chains)], tM=[S[c, R["tM"], :KM[c] + 1] for c in range(self.n_chains)],
                    likA=sc[:, X["likA"]], priorA=sc[:, X["priorA"]], accepted=sc[:, X["accepted"]].astype(np.int64))

    def rtt_summary(self, burnin=0.2, pooled=True, workspace_bytes=None):
        from . import ops
        self.check_status()
        return ops.rtt_summary(self.trace, self.samples_done(), self.start_time, self.end_time, burnin, pooled, workspace_bytes)

    def ess_rows(self, rows):
        from .logs import MCMC_HEAD
        return rows, [1, 2, 3, 4, 5, 6, 7, 10, 11, 12], list(MCMC_HEAD)

    def ess_summary(self, burnin=0.1, columns=None, max_lag=2000):
        from . import ops
        self.check_status()
        S = self.samples_done()
        rows, cols, head = self.ess_rows(self.trace[:S])
        if columns is not None:
            cols = [int(c) for c in columns]
        names = [head[c] if c < len(head) else "col_%d" % c for c in cols]
        return ops.ess_summary(rows, S, cols, burnin, max_lag), names

    def trace_rows(self, n_samples=None):
        self.check_status()
        n_avail = self.samples_done()
        n = n_avail if n_samples is None else min(n_samples, n_avail)
        return self.trace[:n].cpu().numpy()

    def close(self):
        self.state = self.trace = self.data = None


def replicate_log_paths(path, model, out, chains_per_rep):
    """[per chain of the replicate] the reference's own log names under the file's literate_mcmc_logs/ with one chain per
    replicate, <stem>_c<k>_* beyond (logs.log_paths)"""
    from . import logs
    return [logs.log_paths(path, model, out, None if chains_per_rep == 1 else k)[1] for k in range(chains_per_rep)]


def div_replicates_table(sp, ex, br):
    """[n_bins, 10]: per bin the mean, min and max over replicates of the empirical birth rate sp / br, the empirical death
    rate ex / br and br_length (utilities/imputation_averager.py's numbers); columns DIV_HEAD"""
    with np.errstate(all="ignore"):
        eb, ed = sp / br, ex / br
    cols = [np.arange(sp.shape[1], dtype=float)]
    for x in (eb, ed, br):
        cols += [x.mean(axis=0), x.min(axis=0), x.max(axis=0)]
    return np.stack(cols, axis=1)


def write_div_replicates(path, sp, ex, br):
    tab = div_replicates_table(sp, ex, br)
    with open(path, "w") as f:
        f.write("\t".join(DIV_HEAD) + "\n")
        for row in tab:
            f.write("%d\t" % int(row[0]) + "\t".join(str(float(v)) for v in row[1:]) + "\n")


def run(args, parse=None, files=None, name=None, engine=None, finish=None):
    """LiteRateForward.py --replicates PATTERN: every chain of every replicate in one engine; the reference's logs per
    replicate under its own file's literate_mcmc_logs/, flushed per --block window; the pooled outputs (--rtt, --rtt_bf,
    --ess, --combine, <NAME>_div_replicates.tsv) under the first file's, stem NAME.
    A caller that has checked the arguments itself (literate_amd/mc3.py) names the files, may name the stem, builds the engine
    - engine(reps, n_chains, **ReplicateEngine's keywords) - and is called as finish(engine, stem) before the engine closes."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    err = arg_error(args, world) if files is None else None
    if err:
        raise SystemExit(err)
    try:
        files = expand_pattern(args.replicates) if files is None else list(files)
        cpr = chains_per_replicate(args.chains, len(files))
    except ValueError as e:
        raise SystemExit(str(e))
    import torch
    from . import logs, ops
    rseed = np.random.randint(0, 9999) if args.seed == -1 else args.seed
    np.random.seed(rseed)
    try:
        reps = load_replicates(files, args, parse)
    except ValueError as e:
        raise SystemExit(str(e))
    model, R = args.model_BDI, len(files)
    name = name or args.replicates_name or default_name(R)
    n_samples = (args.n + args.s - 1) // args.s if args.n > 0 else 0
    eng = (engine or ReplicateEngine)(reps, args.chains, model=model, seed=rseed, const_rates=args.const_rates,
                          const_death_rate=args.const_death_rate, use_rate_HP=args.use_rate_HP, poisson_HP=args.Poisson_prior,
                          update_fraction=args.update_fraction, s_freq=args.s, n_trace_slots=n_samples)
    print("%d replicates, %d chains each, %d time bins from %d on" % (R, cpr, reps.n_bins, reps.t0))
    writers = []
    for r, path in enumerate(files):
        out_dir, paths = logs.log_paths(path, model, args.out)
        os.makedirs(out_dir, exist_ok=True)
        logs.write_div_log(paths["div"], reps.sp[r].astype(np.int64), reps.ex[r].astype(np.int64), reps.br[r])
        emp = reps.empirical(r) if args.calc_adequacy else None
        if n_samples:
            writers.append(logs.ChainLogWriter(path, model, args.out, cpr, emp, reps.n_bins, args.pyrate_output, reps.true_root_age[r]))
    out_dir0 = logs.log_paths(files[0], model, args.out)[0]
    stem = "%s/%s" % (out_dir0, name)
    write_div_replicates(stem + "_div_replicates.tsv", reps.sp, reps.ex, reps.br)
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
        for r, w in enumerate(writers):
            w.append(np.ascontiguousarray(rows[:, r * cpr:(r + 1) * cpr]))
        s_done = s1
        snap = eng.snapshot()
        print(done, snap["likA"][0], snap["priorA"][0])
        print("\tsp.times:", snap["tL"][0]), print("\tex.times:", snap["tM"][0])
        print("\tsp.rates:", snap["L"][0]), print("\tex.rates:", snap["M"][0])
        sys.stdout.flush()
    eng.check_status()
    if args.n > 0:
        el = time.time() - t_start
        print("%d iterations x %d chains in %.2f s (%.0f iterations/s/chain)" % (args.n, args.chains, el, args.n / el))
    wtxt = eng.warning_text()
    if wtxt:
        print(wtxt, file=sys.stderr)
    if n_samples and args.combine >= 0:
        mcmc = [p["mcmc"] for path in files for p in replicate_log_paths(path, model, args.out, cpr)]
        tmp = tempfile.mkdtemp(dir=out_dir0)
        try:
            logs.combine_logs(mcmc, tmp, args.combine)
            for kind in ("mcmc", "sp_rates", "ex_rates", "div"):
                shutil.move("%s/COMBINED_%s.log" % (tmp, kind), "%s_COMBINED_%s.log" % (stem, kind))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if args.rtt >= 0 and n_samples:
        S = eng.samples_done()
        burn = int(args.rtt * S)
        res = ops.rtt_summary(eng.trace[burn:S], S - burn, eng.start_time, eng.end_time, burnin=0.0, pooled=True)
        logs.write_rtt_tables(stem, res.time, res.rates[0].cpu().numpy(), res.shift_freq[0].cpu().numpy(), res.k_counts[0].cpu().numpy())
        print("posterior rates through time over all replicates: %s_RTT.tsv, %s_RTT_K.tsv (%d samples)" % (stem, stem, res.n_samples))
        if args.rtt_bf > 0:
            lam = args.rtt_bf_lambda if args.rtt_bf_lambda > 0 else None
            prior = ops.shift_prior(eng.start_time, eng.end_time, n_reps=args.rtt_bf, seed=rseed, poi_lambda=lam)
            logs.write_rtt_bf_tables(stem, res.time, res.rates[0].cpu().numpy(), res.shift_freq[0].cpu().numpy(),
                                     res.k_counts[0].cpu().numpy(), prior.totals.cpu().numpy(), prior.shift_hist.cpu().numpy(),
                                     prior.k_accepted.cpu().numpy(), args.rtt_bf, args.rtt_bf_lambda)
            print("Bayes factors for rate shifts: %s_RTT_BF.tsv, _RTT_BF_prior.tsv, _RTT_BF_K.tsv" % stem)
    if args.ess != -1.0 and n_samples:
        logs.write_run_ess(eng, args.chains, args.chains, 1, 0, args.ess, args.s, stem)
        with open(stem + "_ESS.tsv") as f:
            body = f.read()
        with open(stem + "_ESS.tsv", "w") as f:
            f.write(ESS_NOTE % (R, cpr) + body)
    if finish is not None:
        finish(eng, stem)
    eng.close()
    torch.cuda.synchronize()
