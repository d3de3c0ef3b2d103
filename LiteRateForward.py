#!/usr/bin/env python
"""LiteRateForward.py - drop-in command line of the reference's RJMCMC sampler
(/root/reference/LiteRateForward.py:376-403: same flags, defaults and log files), running
`--chains` independent chains on MI355X GPUs through literate_amd.

Additive flags (not in the reference): --chains N (total chains; sharded over ranks when started
with torch.distributed.run), --init_shifts K (start every chain with K equally spaced shifts per
process and the CLI's Gamma(2,2) rates; SURVEY.md section 8c 'config-1 note'), --rtt BURNIN and --rtt_bf REPS
(posterior rates through time, and the frequencies of rate shifts as Bayes factors against their Monte Carlo prior:
what plotRJforward.v3.py derives from the logs, computed on the GPU).
With --chains 1 the log file names are exactly the reference's; with more, chain k >= 0 writes
<name>_c<k>_{mcmc,sp_rates,ex_rates}.log next to the shared _div.log.
--replicates PATTERN runs the sampler on many replicate data sets in one launch (literate_amd/replicates.py).
--mc3 T runs T - 1 heated chains beside every cold one, which swap their temperatures (literate_amd/mc3.py).
"""
import argparse
import os
import sys
import time
from warnings import warn

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('-v', action='version', version='%(prog)s')
    p.add_argument('-d', type=str, help='data file', default="", metavar="")
    p.add_argument('-n', type=int, help='n. MCMC iterations', default=10000000, metavar=10000000)
    p.add_argument('-p', type=int, help='print frequency', default=1000, metavar=1000)
    p.add_argument('-s', type=int, help='sampling frequency', default=1000, metavar=1000)
    p.add_argument('-seed', type=int, help='seed (set to -1 to make it random)', default=-1, metavar=-1)
    p.add_argument('-const_rates', type=int, help="set to: 1 for constant B/I and D rates", default=0, metavar=0)
    p.add_argument('-const_death_rate', type=int, help="set to: 1 for constant D rates", default=0, metavar=0)
    p.add_argument('-model_BDI', type=int, help='0: birth-death; 1: immigration-death; 2 birth-death (Keiding likelihood); 3 Keiding likelihood, only no extant', default=0, metavar=0)
    p.add_argument('-TBP', help='Default is AD. Include for TBP.', default=False, action='store_true')
    p.add_argument('-pyrate_output', help='Make output PyRate-compatible', default=False, action='store_true')
    p.add_argument('-first_year', type=int, help='different start of the dataset (unspecified for TBP)', default=-1, metavar=-1)
    p.add_argument('-last_year', type=int, help='different end of the dataset (unspecified for TBP)', default=-1, metavar=-1)
    p.add_argument('-death_jitter', type=float, help='amount added to death times', default=.5, metavar=.5)
    p.add_argument('-use_rate_HP', type=int, help='0: no hyper-prior on rates, 1: hyper-prior on rates', default=1, metavar=1)
    p.add_argument('-Poisson_prior', type=float, help='0: use hyper-prior on n. shifts, >0:  fixed prior on n. shifts', default=0, metavar=0)
    p.add_argument('-rm_first_bin', type=float, help='if set to 1 it removes the first time bin', default=0, metavar=0)
    p.add_argument('-calc_adequacy', type=int, help='if set to 1 calculates and log to file adequacy', default=1, metavar=1)
    p.add_argument('-update_fraction', type=float, help='', default=0.75, metavar=0.75)
    p.add_argument('-out', type=str, help='output tag', default="", metavar="")
    p.add_argument('-rev_se', type=int, help='reversed order of ts and te in input file', default=0, metavar=0)
    p.add_argument('--chains', type=int, default=1, help='total number of independent chains')
    p.add_argument('--checkpoint', type=str, default="", help='file the run is saved to after every print block and '
                   'resumed from if it exists (same data and flags; extension to the reference, which cannot resume)')
    p.add_argument('--combine', type=float, default=-1.0, help='with --chains > 1: also write COMBINED_{mcmc,sp_rates,'
                   'ex_rates,div}.log with this burn-in fraction dropped per chain (plotRJforward.v3.py combine_logs)')
    p.add_argument('--rtt', type=float, default=-1.0, help='after the run, write <stem>_RTT.tsv (posterior mean and 95 %% HPD '
                   'of the birth, death and net rates and the frequency of rate shifts per unit bin) and <stem>_RTT_K.tsv '
                   '(histogram of the number of rates) next to the logs, pooled over all chains with this burn-in fraction '
                   'dropped per chain (plotRJforward.v3.py -combine 1); computed on the GPU')
    p.add_argument('--rtt_bf', type=int, default=0, metavar='REPS', help='with --rtt: also write <stem>_RTT_BF.tsv (the shift '
                   'frequencies of <stem>_RTT.tsv as 2 ln Bayes factors against the prior on shift times, and the birth_BF2 / '
                   'birth_BF6 / death_BF2 / death_BF6 vectors of plotRJforward.v3.py), <stem>_RTT_BF_prior.tsv (the prior '
                   'frequency and the bf2 / bf6 thresholds) and <stem>_RTT_BF_K.tsv (prior and posterior of the number of '
                   'rates); the prior is simulated over REPS replicates on the GPU (get_prior_shift runs 100000 on the host)')
    p.add_argument('--rtt_bf_lambda', type=float, default=0.0, metavar='L', help='the prior --rtt_bf simulates: 0 = the '
                   'Gamma(2, 1) hyper-prior on the Poisson rate that plotRJforward.v3.py hard-codes, L > 0 = that fixed '
                   'rate (a run made with -Poisson_prior L)')
    p.add_argument('--ess', type=float, default=-1.0, help='after the run, write <stem>_ESS.tsv (per log column: pooled '
                   'mean and effective sample size, the lowest chain ESS, split R-hat) and <stem>_ESS_chains.tsv (ESS, '
                   'autocorrelation time and SE of the mean per chain and column) next to the logs, with this burn-in '
                   'fraction dropped per chain (what the tutorial checks in Tracer); computed on the GPU')
    p.add_argument('--ppc', type=float, default=-1.0, help='after the run, write <stem>_PPC.tsv and <stem>_PPC_fit.tsv next '
                   'to the logs: a posterior predictive check that simulates lineages forward under --ppc_draws posterior '
                   'draws of the rates (this burn-in fraction dropped per chain) and sets the predicted births, deaths and '
                   'diversity per bin beside the observed ones; simulated on the GPU')
    p.add_argument('--ppc_draws', type=int, default=1000, help='posterior draws the check simulates under')
    p.add_argument('--ppc_scale', type=int, default=100, help='simulation steps per time unit (the reference Simulator.scale)')
    p.add_argument('--ppc_start_bin', type=int, default=-1, help='bin at whose left edge the free-running simulations start '
                   '(default: the first bin after bin 0 that starts with an observed lineage)')
    p.add_argument('--ppc_age', type=float, default=-1.0, help='after the run, write <stem>_PPC_age.tsv and <stem>_PPC_age_fit.tsv next '
                   'to the logs: the lifespan check - every lineage, born when the data say, is given a death time under '
                   '--ppc_age_draws posterior draws of the death rates (this burn-in fraction dropped per chain), and the '
                   'predicted deaths and hazard by AGE are set beside the observed ones: does the chance of dying depend '
                   'on age, which the model assumes it does not; simulated on the GPU; not with -model_BDI 3 or -pyrate_output')
    p.add_argument('--ppc_age_draws', type=int, default=1000, help='posterior draws the lifespan check simulates under')
    p.add_argument('--ade', type=float, default=-1.0, help='after the run, write <stem>_ADE.tsv and <stem>_ADE_shape.tsv beside '
                   'the logs: age-dependent extinction - the Weibull shape of the hazard by lineage age (< 1: a liability of '
                   'newness, > 1: ageing, 1: what the model assumes), fitted on the GPU conditional on --ade_draws posterior '
                   'draws of the per-bin death rates (this burn-in fraction dropped per chain), beside the constant-baseline '
                   'Weibull of the reference ADE scripts; at most 512 time bins; not with -model_BDI 3 or -pyrate_output')
    p.add_argument('--ade_draws', type=int, default=1000, help='posterior draws the age-dependent extinction fit conditions on')
    p.add_argument('--ade_joint', type=float, default=-1.0, help='after the run, write <stem>_ADE_joint.tsv, <stem>_ADE_joint_rates.tsv '
                   'and <stem>_ADE_joint_draws.npz beside the logs: age-dependent extinction sampled jointly - a sampler of its own '
                   'over (baseline death-rate skyline, Weibull shape) on the GPU, --chains chains on the run\'s lineages, window '
                   'and seed, this burn-in fraction dropped per chain; what --ade\'s conditional fit becomes once the rate '
                   'shifts may move with the shape; at most 128 time bins; refused where --ade is')
    p.add_argument('--ade_joint_n', type=int, default=0, help='iterations of the joint sampler (default: -n)')
    p.add_argument('--ade_joint_s', type=int, default=0, help='sampling frequency of the joint sampler (default: -s)')
    p.add_argument('--ade_joint_win', type=float, default=0.4, help='width of the joint sampler\'s window move in log shape')
    p.add_argument('--waic', type=float, default=-1.0, help='after the run, write <stem>_WAIC.tsv and <stem>_WAIC_pointwise.npz next to the logs: WAIC (elpd, '
                   'p_waic and their standard errors) from --waic_draws posterior draws of the rates (this burn-in '
                   'fraction dropped per chain), the log-likelihood term of each lineage reduced over the draws on the GPU; '
                   'rank runs of the same program on the same data with `python -m literate_amd.waic '
                   'A_WAIC_pointwise.npz B_WAIC_pointwise.npz`; not with -model_BDI 1 or -pyrate_output')
    p.add_argument('--waic_draws', type=int, default=1000, help='posterior draws WAIC is computed from (at least 2)')
    p.add_argument('--loo', type=float, default=-1.0, help='after the run, write <stem>_LOO.tsv and <stem>_LOO_pointwise.npz next to the logs: PSIS-LOO '
                   '(Pareto-smoothed leave-one-out: elpd_loo, p_loo, their standard errors and the Pareto k of every lineage) '
                   'from --loo_draws posterior draws, chosen and scored as --waic does (this burn-in fraction dropped per '
                   'chain), every lineage\'s draws sorted, fitted and smoothed on the GPU; rank runs of the same program on '
                   'the same data with `python -m literate_amd.loo A_LOO_pointwise.npz B_LOO_pointwise.npz`; not with -model_BDI 1 or -pyrate_output')
    p.add_argument('--loo_draws', type=int, default=1000, help='posterior draws PSIS-LOO is computed from (2 to 8192)')
    p.add_argument('--init_shifts', type=int, default=0, help='initial number of rate shifts per process')
    p.add_argument('--block', type=int, default=0, help='iterations per device window: logs are written and flushed and '
                   'the state is printed once per window, while the next one runs (default: -p rounded up to ~50000)')
    p.add_argument('--replicates', type=str, default="", metavar='PATTERN', help='run on many replicate data sets at once (one '
                   'stochastic imputation of the death times each): a glob or a comma-separated list of data files, expanded '
                   'and sorted here; -d stays empty, --chains is the total and a multiple of the number of files; every '
                   'replicate gets the reference\'s logs under its own file\'s literate_mcmc_logs/, the pooled --rtt, --rtt_bf, '
                   '--ess and --combine outputs and <NAME>_div_replicates.tsv go under the first file\'s; the files must share '
                   'their window of time bins (at most 512)')
    p.add_argument('--mc3', type=int, default=1, metavar='T', help='Metropolis coupling: beside every cold chain run T - 1 heated chains '
                   'on likelihood^beta * prior, which cross between numbers of rate shifts more easily and hand their states '
                   'down by swaps (1 = off, at most 8; more than 4 with at most 256 time bins); --chains stays the number of '
                   'cold chains, the only ones logged; works on -d FILE and on --replicates, through the replicate sampler '
                   '(unit time bins, at most 512; not with --ppc, --ppc_age, --ade, --ade_joint, --waic, --loo, --checkpoint, '
                   '--init_shifts, several ranks); writes <stem>_MC3.tsv: the ladder, the swap rate of every pair and the '
                   'round trips of every ladder')
    p.add_argument('--mc3_dt', type=float, default=0.1, help='heating increment of --mc3: beta_j = 1 / (1 + mc3_dt * j)')
    p.add_argument('--mc3_every', type=int, default=100, help='iterations between two swap rounds of --mc3 (0: never)')
    p.add_argument('--replicates_name', type=str, default="", metavar='NAME', help='stem of the pooled outputs of --replicates '
                   '(default: replicates<number of files>)')
    return p


def parse_data(args):
    """LRF:438-474 (np.genfromtxt path), including its filters as written."""
    t_file = np.genfromtxt(args.d, skip_header=1)
    if t_file.shape[1] == 4:
        warn('Four column (with clade) LiteRate input is deprecated. Use three columns.', FutureWarning)
        ts_years, te_years = t_file[:, 2], t_file[:, 3]
    elif args.rev_se:
        ts_years, te_years = t_file[:, 2], t_file[:, 1]
    else:
        ts_years, te_years = t_file[:, 1], t_file[:, 2]
    if args.TBP:
        true_root_age = np.max(ts_years)
        ts, te = true_root_age - ts_years, true_root_age - te_years
    else:
        true_root_age = 0
        if args.first_year != -1:
            ts_years = ts_years[ts_years >= args.first_year]
            te_years = te_years[ts_years >= args.first_year]      # LRF:460-461 (filter on the filtered array)
        if args.last_year != -1:
            ts = ts_years[ts_years <= args.last_year]
            te = te_years[ts_years <= args.last_year]
            te[te > args.last_year] = args.last_year
        else:
            ts, te = ts_years, te_years
    te = te + args.death_jitter
    return np.asarray(ts, dtype=float), np.asarray(te, dtype=float), true_root_age


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mc3 != 1:
        from literate_amd import mc3
        err = mc3.arg_error(args, int(os.environ.get("WORLD_SIZE", "1")))
        if err:
            raise SystemExit(err)
    elif args.replicates:
        from literate_amd import replicates
        err = replicates.arg_error(args, int(os.environ.get("WORLD_SIZE", "1")))
        if err:
            raise SystemExit(err)
    if args.rtt >= 0 and args.pyrate_output:
        raise SystemExit("--rtt bins the AD / TBP times of the logs; -pyrate_output flips them, which the reference's plot "
                         "does not bin the same way: not supported together")
    if args.rtt >= 1:
        raise SystemExit("--rtt takes a burn-in fraction in [0, 1)")
    if args.rtt_bf != 0 or args.rtt_bf_lambda != 0:
        from literate_amd.logs import rtt_bf_arg_error
        err = rtt_bf_arg_error(args.rtt_bf, args.rtt_bf_lambda, args.rtt)
        if err:
            raise SystemExit(err)
    if args.ess != -1.0:
        from literate_amd.logs import ess_arg_error
        err = ess_arg_error(args.ess, args.n, args.s)
        if err:
            raise SystemExit(err)
    if args.ppc != -1.0:
        from literate_amd.ppc import arg_error
        err = arg_error(args.ppc, args.model_BDI, args.pyrate_output)
        if err:
            raise SystemExit(err)
        if args.ppc_draws < 1 or args.ppc_scale < 1:
            raise SystemExit("--ppc_draws and --ppc_scale must be at least 1")
    if args.ppc_age != -1.0:
        from literate_amd.ppc_age import arg_error as age_arg_error
        err = age_arg_error(args.ppc_age, args.ppc_age_draws, model=args.model_BDI, pyrate_output=args.pyrate_output)
        if err:
            raise SystemExit(err)
    if args.ade != -1.0:
        from literate_amd.ade import arg_error as ade_arg_error
        err = ade_arg_error(args.ade, args.ade_draws, model=args.model_BDI, pyrate_output=args.pyrate_output)
        if err:
            raise SystemExit(err)
    if args.ade_joint != -1.0:
        from literate_amd.ade_joint import arg_error as adej_arg_error
        err = adej_arg_error(args.ade_joint, args.ade_joint_n or args.n, args.ade_joint_s or args.s, args.ade_joint_win, model=args.model_BDI, pyrate_output=args.pyrate_output)
        if err:
            raise SystemExit(err)
    if args.waic != -1.0:
        from literate_amd.waic import arg_error as waic_arg_error
        err = waic_arg_error(args.waic, args.waic_draws, model=args.model_BDI, pyrate_output=args.pyrate_output)
        if err:
            raise SystemExit(err)
    if args.loo != -1.0:
        from literate_amd.loo import arg_error as loo_arg_error
        err = loo_arg_error(args.loo, args.loo_draws, model=args.model_BDI, pyrate_output=args.pyrate_output)
        if err:
            raise SystemExit(err)
    print("\n\n             LiteRate - 20200206 (MI355X engine)\n")
    if args.mc3 != 1:
        return mc3.run(args, parse_data)
    if args.replicates:
        return replicates.run(args, parse_data)
    import torch
    import torch.distributed as dist
    from literate_amd import dist as lrd
    from literate_amd import logs, ops
    from literate_amd.engine import ChainEngine

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        backend = os.environ.get("LR_DIST_BACKEND", "nccl")      # gloo: rehearsal of the sharded run on one GPU
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend)
    rseed = np.random.randint(0, 9999) if args.seed == -1 else args.seed
    if world > 1:
        s = torch.tensor([rseed], device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.broadcast(s, 0)
        rseed = int(s.item())
    np.random.seed(rseed)

    ts, te, true_root_age = parse_data(args)
    model = args.model_BDI
    offset, n_local = lrd.shard_chains(args.chains, world, rank)
    n_samples = (args.n + args.s - 1) // args.s if args.n > 0 else 0
    eng = ChainEngine(ts, te, max(n_local, 1), model=model, seed=rseed, const_rates=args.const_rates,
                      const_death_rate=args.const_death_rate, use_rate_HP=args.use_rate_HP,
                      poisson_HP=args.Poisson_prior, update_fraction=args.update_fraction, s_freq=args.s,
                      n_trace_slots=n_samples, chain_offset=offset)
    sp, ex, br = [x.cpu().numpy() for x in (eng.sp_events, eng.ex_events, eng.br_length)]
    if args.rm_first_bin:
        raise SystemExit("-rm_first_bin 1 makes the reference's own sampler fail with IndexError at the first "
                         "K>=2 proposal (SURVEY.md section 8a A13); not supported")
    if rank == 0:
        print(ex.tolist())
        print(br.sum(), range(int(np.min(ts)), int(np.max(te))))
        out_dir, paths = logs.log_paths(args.d, model, args.out)
        try:
            os.mkdir(out_dir)
        except OSError as e:
            print(e)
        logs.write_div_log(paths["div"], sp, ex, br)
    emp = None
    if args.calc_adequacy:
        with np.errstate(all="ignore"):
            emp = (sp / br, ex / br)
        if rank == 0:
            print("EMPIRICAL BIRTH RATES:"), print(emp[0]), print("EMPIRICAL DEATH RATES:"), print(emp[1])

    if args.init_shifts > 0:
        k = args.init_shifts + 1
        t = np.linspace(eng.start_time, eng.end_time, k + 1)
        rng = np.random.default_rng(rseed)
        L = [rng.gamma(2, 2, k) for _ in range(eng.n_chains)]
        M = [rng.gamma(2, 2, k) for _ in range(eng.n_chains)]
        eng.init(L, M, [t] * eng.n_chains, [t] * eng.n_chains)
    else:
        eng.init()
    done = 0
    ckpt = (args.checkpoint + (".rank%d" % rank if world > 1 else "")) if args.checkpoint else ""
    if ckpt and not ckpt.endswith(".npz"):
        ckpt += ".npz"
    if ckpt and os.path.exists(ckpt):
        eng.load(ckpt)
        done = eng.iterations
        if rank == 0:
            print("resumed from %s at iteration %d" % (ckpt, done))
    # The logs are written as the run goes (the reference flushes every sample, LRF:334-359): a window's rows leave the
    # device on a side stream - gathered over RCCL when the chains are sharded - while the next window runs.  A resumed
    # run rewrites the rows the checkpoint holds first (they are all in the workspace), then appends.  A checkpoint per
    # window: the state is copied on the device at the window's end (checkpoint_begin) and written - with the window's
    # trace rows appended to <file>.trace - behind the next window, after collect() has shown that the run is not void.
    from literate_amd.engine import TraceStreamer
    streamer = TraceStreamer(eng, args.chains, n_local)
    writer = None
    if rank == 0 and n_samples:
        writer = logs.ChainLogWriter(args.d, model, args.out, args.chains, emp, eng.n_bins, args.pyrate_output, true_root_age)
    tickets = []                     # one per marked window: its end as a checkpoint ticket (None: nothing to write)
    if done > 0:
        streamer.mark()
        tickets.append(None)         # (the rows a resumed run re-reads are the checkpoint's own)

    def flush_window():
        rows, snap, (s0, s1, its) = streamer.collect()      # (raises when the run is void: no checkpoint of it is written)
        ticket = tickets.pop(0)
        if ticket is not None:
            eng.checkpoint_write(ticket, ckpt)              # the window's end, on disk while the next window runs
        if rank == 0:
            if writer is not None:
                writer.append(rows)
            print(its, snap["likA"][0], snap["priorA"][0])
            print("\tsp.times:", snap["tL"][0]), print("\tex.times:", snap["tM"][0])
            print("\tsp.rates:", snap["L"][0]), print("\tex.rates:", snap["M"][0])
            sys.stdout.flush()

    t_start = time.time()
    block = args.block if args.block > 0 else args.p * max(1, 50000 // max(args.p, 1))
    while done < args.n:
        n = min(block, args.n - done)
        eng.steps(n)
        streamer.mark()
        done += n
        tickets.append(eng.checkpoint_begin() if ckpt else None)    # a device-side copy of the state at the window's end
        if len(streamer.pending) > 1:
            flush_window()          # the window before this one, while this one runs
    while streamer.pending:
        flush_window()
    torch.cuda.synchronize()
    eng.check_status()
    if rank == 0 and args.n > 0:
        el = time.time() - t_start
        print("%d iterations x %d chains in %.2f s (%.0f iterations/s/chain)" % (args.n, args.chains, el, args.n / el))
    wtxt = eng.warning_text()
    if wtxt:
        print(wtxt, file=sys.stderr)
    if rank == 0 and n_samples and args.combine >= 0 and args.chains > 1:
        files = [logs.log_paths(args.d, model, args.out, c)[1]["mcmc"] for c in range(args.chains)]
        logs.combine_logs(files, os.path.dirname(files[0]), args.combine)
    if args.rtt >= 0 and n_samples:
        res = write_rtt(args, eng, n_local, world, rank)
        if args.rtt_bf > 0 and rank == 0:
            write_rtt_bf(args, eng, res, rseed)
    if args.ess != -1.0:
        stem = logs.log_paths(args.d, args.model_BDI, args.out)[1]["div"][:-len("_div.log")]
        logs.write_run_ess(eng, n_local, args.chains, world, rank, args.ess, args.s, stem)
    if args.ppc != -1.0 and n_samples:
        from literate_amd import ppc
        stem = logs.log_paths(args.d, args.model_BDI, args.out)[1]["div"][:-len("_div.log")]
        ppc.write_run_ppc(eng, sp, ex, n_local, args.chains, world, rank, args.ppc, args.ppc_draws, args.ppc_scale, rseed,
                          stem, start_bin=args.ppc_start_bin if args.ppc_start_bin >= 0 else None)
    if args.ppc_age != -1.0 and n_samples:
        from literate_amd import ppc_age
        stem = logs.log_paths(args.d, args.model_BDI, args.out)[1]["div"][:-len("_div.log")]
        ppc_age.write_run(eng, n_local, args.chains, world, rank, args.ppc_age, args.ppc_age_draws, rseed, stem)
    if args.ade != -1.0 and n_samples:
        from literate_amd import ade
        stem = logs.log_paths(args.d, args.model_BDI, args.out)[1]["div"][:-len("_div.log")]
        ade.write_run(eng, n_local, args.chains, world, rank, args.ade, args.ade_draws, stem)
    if args.ade_joint != -1.0:
        from literate_amd import ade_joint
        stem = logs.log_paths(args.d, args.model_BDI, args.out)[1]["div"][:-len("_div.log")]
        ade_joint.write_run(eng, args.chains, rank, args.ade_joint, args.ade_joint_n or args.n, args.ade_joint_s or args.s,
                            args.ade_joint_win, rseed, stem, const=args.const_rates, use_rate_hp=args.use_rate_HP, poisson_prior=args.Poisson_prior)
    if args.waic != -1.0 and n_samples:
        from literate_amd import waic
        stem = logs.log_paths(args.d, args.model_BDI, args.out)[1]["div"][:-len("_div.log")]
        waic.write_run(eng, n_local, args.chains, world, rank, args.waic, args.waic_draws, stem)
    if args.loo != -1.0 and n_samples:
        from literate_amd import loo
        stem = logs.log_paths(args.d, args.model_BDI, args.out)[1]["div"][:-len("_div.log")]
        loo.write_run(eng, n_local, args.chains, world, rank, args.loo, args.loo_draws, stem)
    eng.close()
    if world > 1:
        dist.destroy_process_group()


def write_rtt(args, eng, n_local, world, rank):
    """--rtt: the posterior rates through time of the whole run, pooled over all chains (plotRJforward.v3.py -combine 1:
    combine_logs drops int(burnin * S) rows of every chain, then burnin = 0) -> <stem>_RTT.tsv and <stem>_RTT_K.tsv on
    rank 0.  The post-burn-in rows are gathered to rank 0's device once; the summary runs there (ops.rtt_summary)."""
    from literate_amd import dist as lrd
    from literate_amd import logs, ops
    S = eng.samples_done()
    burn = int(args.rtt * S)
    local = eng.trace[burn:S][:, :n_local]
    rows = lrd.gather_traces(local.contiguous(), args.chains) if world > 1 else local
    if rank != 0:
        return None
    res = ops.rtt_summary(rows, S - burn, eng.start_time, eng.end_time, burnin=0.0, pooled=True)
    out_dir, paths = logs.log_paths(args.d, args.model_BDI, args.out)
    stem = paths["div"][:-len("_div.log")]
    logs.write_rtt_tables(stem, res.time, res.rates[0].cpu().numpy(), res.shift_freq[0].cpu().numpy(),
                          res.k_counts[0].cpu().numpy())
    print("posterior rates through time: %s_RTT.tsv, %s_RTT_K.tsv (%d samples)" % (stem, stem, res.n_samples))
    return res


def write_rtt_bf(args, eng, res, rseed):
    """--rtt_bf REPS (rank 0, after write_rtt, on its RttSummary): the prior on shift times over the run's time span by
    Monte Carlo on the GPU (ops.shift_prior, the stream the run's seed names; get_prior_shift of plotRJforward.v3.py), then
    the Bayes-factor tables (logs.write_rtt_bf_tables).  The thresholds are computed once and serve births and deaths, as
    the script computes them in its birth call and reuses them."""
    from literate_amd import logs, ops
    lam = args.rtt_bf_lambda if args.rtt_bf_lambda > 0 else None
    prior = ops.shift_prior(eng.start_time, eng.end_time, n_reps=args.rtt_bf, seed=rseed, poi_lambda=lam)
    stem = logs.log_paths(args.d, args.model_BDI, args.out)[1]["div"][:-len("_div.log")]
    ps, bf2, bf6 = logs.write_rtt_bf_tables(stem, res.time, res.rates[0].cpu().numpy(), res.shift_freq[0].cpu().numpy(),
                                            res.k_counts[0].cpu().numpy(), prior.totals.cpu().numpy(),
                                            prior.shift_hist.cpu().numpy(), prior.k_accepted.cpu().numpy(), args.rtt_bf,
                                            args.rtt_bf_lambda)
    print("Bayes factors for rate shifts: %s_RTT_BF.tsv, _RTT_BF_prior.tsv, _RTT_BF_K.tsv (%d prior replicates, prior "
          "frequency %s, bf2 = %s, bf6 = %s)" % (stem, args.rtt_bf, ps, bf2, bf6))


if __name__ == "__main__":
    main()
