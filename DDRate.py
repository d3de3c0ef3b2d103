#!/usr/bin/env python3
"""DDRate.py - drop-in CLI for the reference's DDRate.py (diversity-dependent birth/death rates), with the whole
Metropolis-Hastings loop (DDRate.py:124-241) running on the MI355X for any number of independent chains.

Same flags as the reference (core_arguments lib:291-308 + -m_birth / -m_death / -fix_death, DD:22-27) and the same
log file beside the data, `<data>_<seed><model suffix>.log` (DD:135-143), one per chain (`_c<i>` appended when
--chains > 1).  Extension: --chains.  Randomness is the engine's addressed Philox stream keyed by (seed, chain), so
trajectories are reproducible but are not numpy's.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from literate_amd.literate_library import core_arguments, parse_ts_te, print_empirical_rates, set_seed  # noqa: E402


def build_parser():
    p = core_arguments()
    p.add_argument('-m_birth', type=int, help='0) use const b rates 1) DD birth 2) niche dep DD b', default=2, metavar=2)
    p.add_argument('-m_death', type=int, help='-1) fixed d rate 0) use const d rates 1) DD death 2) niche dep DD d',
                   default=2, metavar=2)
    p.add_argument('-fix_death', type=float, help='Fix death rate (with -m_death -1)', default=0.1, metavar=0.1)
    p.add_argument('--chains', type=int, default=1, help='total number of independent chains (extension)')
    p.add_argument('--ess', type=float, default=-1.0, help='after the run, write <stem>_ESS.tsv and <stem>_ESS_chains.tsv '
                   '(per-chain effective sample sizes and split R-hat of the logged parameters, this burn-in fraction '
                   'dropped per chain) beside the logs; computed on the GPU (extension)')
    p.add_argument('--summary', type=float, default=-1.0, help='after the run, write <stem>_summary.tsv (birth, death, net '
                   'rate, carrying capacity and niche fraction per time bin: mean and 95 %% HPD, with the empirical rates) and '
                   '<stem>_summary_params.tsv (mean and HPD of the logged parameters) beside the logs, all chains pooled '
                   'after this burn-in fraction is dropped from each; computed on the GPU from the resident trace '
                   '(extension)')
    p.add_argument('--ppc', type=float, default=-1.0, help='after the run, write <stem>_PPC.tsv and <stem>_PPC_fit.tsv beside '
                   'the logs: a posterior predictive check that simulates lineages forward under --ppc_draws posterior '
                   'draws of the parameters (this burn-in fraction dropped per chain), the rates of every simulated step recomputed from the diversity living at that step, and sets the predicted births, '
                   'deaths and diversity per bin beside the observed ones; simulated on the GPU; not with -rm_first_bin 1 '
                   '(extension)')
    p.add_argument('--ppc_draws', type=int, default=1000, help='posterior draws the check simulates under')
    p.add_argument('--ppc_scale', type=int, default=100, help='simulation steps per time unit (the reference Simulator.scale)')
    p.add_argument('--ppc_start_bin', type=int, default=-1, help='bin at whose left edge the free-running simulations start '
                   '(default: the first bin after bin 0 that starts with an observed lineage)')
    p.add_argument('--ppc_age', type=float, default=-1.0, help='after the run, write <stem>_PPC_age.tsv and <stem>_PPC_age_fit.tsv beside '
                   'the logs: the lifespan check - every lineage, born when the data say, is given a death time under '
                   '--ppc_age_draws posterior draws of the per-bin death rates (this burn-in fraction dropped per chain), and '
                   'the predicted deaths and hazard by AGE are set beside the observed ones: does the chance of dying depend '
                   'on age, which the model assumes it does not; simulated on the GPU; not with -rm_first_bin 1 (extension)')
    p.add_argument('--ppc_age_draws', type=int, default=1000, help='posterior draws the lifespan check simulates under')
    p.add_argument('--ade', type=float, default=-1.0, help='after the run, write <stem>_ADE.tsv and <stem>_ADE_shape.tsv beside '
                   'the logs: age-dependent extinction - the Weibull shape of the hazard by lineage age (< 1: a liability of '
                   'newness, > 1: ageing, 1: what the model assumes), fitted on the GPU conditional on --ade_draws posterior '
                   'draws of the per-bin death rates (this burn-in fraction dropped per chain), beside the constant-baseline '
                   'Weibull of the reference ADE scripts; at most 512 time bins; not with -rm_first_bin 1 (extension)')
    p.add_argument('--ade_draws', type=int, default=1000, help='posterior draws the age-dependent extinction fit conditions on')
    p.add_argument('--ade_joint', type=float, default=-1.0, help='after the run, write <stem>_ADE_joint.tsv, <stem>_ADE_joint_rates.tsv '
                   'and <stem>_ADE_joint_draws.npz beside the logs: age-dependent extinction sampled jointly - a sampler of its own '
                   'over (baseline death-rate skyline, Weibull shape) on the GPU, --chains chains on the run\'s lineages, window '
                   'and seed, this burn-in fraction dropped per chain; what --ade\'s conditional fit becomes once the rate '
                   'shifts may move with the shape; at most 128 time bins; refused where --ade is')
    p.add_argument('--ade_joint_n', type=int, default=0, help='iterations of the joint sampler (default: -n)')
    p.add_argument('--ade_joint_s', type=int, default=0, help='sampling frequency of the joint sampler (default: -s)')
    p.add_argument('--ade_joint_win', type=float, default=0.4, help='width of the joint sampler\'s window move in log shape')
    p.add_argument('--mlik', type=float, default=-1.0, help='after the run, write <stem>_MLIK.tsv, <stem>_MLIK_temps.tsv and <stem>_MLIK.npz '
                   'beside the logs: the marginal likelihood log Z of this -m_birth / -m_death model, by stepping stones (and '
                   'thermodynamic integration) over --mlik_temps power posteriors x --mlik_reps replicates, chains of their own '
                   'on the GPU on the run\'s per-bin statistics and seed, this burn-in fraction dropped per chain; it is the '
                   'marginal likelihood under the prior as the sampler realises it (a parameter moved by the multiplier keeps '
                   'its sign, the midpoint is uniform on its reflected range); rank models run on the same data with `python '
                   '-m literate_amd.mlik A_MLIK.npz B_MLIK.npz` (2 ln BF); at most 512 time bins; one GPU (extension)')
    p.add_argument('--mlik_temps', type=int, default=16, help='temperatures of the ladder, beta_j = (j / (T - 1)) ** (1 / alpha)')
    p.add_argument('--mlik_reps', type=int, default=8, help='independent replicates of the ladder (the standard error is theirs)')
    p.add_argument('--mlik_n', type=int, default=0, help='iterations of the power-posterior chains (default: -n)')
    p.add_argument('--mlik_s', type=int, default=0, help='their sampling frequency (default: -s)')
    p.add_argument('--mlik_alpha', type=float, default=0.3, help='exponent of the temperature ladder')
    p.add_argument('--mlik_widen', type=float, default=8.0, help='cap of the window scale min(beta ** -1/2, widen) of the cold '
                   'chains (1: the reference\'s windows at every temperature)')
    p.add_argument('--waic', type=float, default=-1.0, help='after the run, write <stem>_WAIC.tsv and <stem>_WAIC_pointwise.npz beside the logs: WAIC (elpd, '
                   'p_waic and their standard errors) from --waic_draws posterior draws of the parameters, at the '
                   'per-bin rates they give under the observed diversity (this burn-in fraction dropped per chain), the '
                   'term of the log-likelihood per lineage reduced over the draws on the GPU; rank runs of the same program on '
                   'the same data with `python -m literate_amd.waic A_WAIC_pointwise.npz B_WAIC_pointwise.npz`; not with '
                   '-rm_first_bin 1 (extension)')
    p.add_argument('--waic_draws', type=int, default=1000, help='posterior draws WAIC is computed from (at least 2)')
    p.add_argument('--loo', type=float, default=-1.0, help='after the run, write <stem>_LOO.tsv and <stem>_LOO_pointwise.npz beside the logs: PSIS-LOO '
                   '(Pareto-smoothed leave-one-out: elpd_loo, p_loo, their standard errors and the Pareto k of every lineage) '
                   'from --loo_draws posterior draws, chosen and scored as --waic does (this burn-in fraction dropped per '
                   'chain), every lineage\'s draws sorted, fitted and smoothed on the GPU; rank runs of the same program on '
                   'the same data with `python -m literate_amd.loo A_LOO_pointwise.npz B_LOO_pointwise.npz`; not with -rm_first_bin 1 (extension)')
    p.add_argument('--loo_draws', type=int, default=1000, help='posterior draws PSIS-LOO is computed from (2 to 8192)')
    p.add_argument('--block', type=int, default=0, help='iterations per device window (logs are flushed once per window; '
                   'default: -p rounded up to ~50000)')
    p.add_argument('--replicates', type=str, default='', help='run on many replicate data sets - stochastic imputations of the '
                   'death times, say - in one launch: a comma-separated list of files and / or globs (quote them), each parsed '
                   'and binned as -d would be; they must share their number of time bins (at most 512); -d stays empty and '
                   '--chains, the total, is a multiple of the number of files; every replicate gets the reference\'s own log '
                   'beside its own file, --ess and --summary pool all replicates beside the first (extension)')
    p.add_argument('--replicates_name', type=str, default='', help='stem of the pooled outputs of --replicates (default: '
                   'replicates<number of files>)')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.replicates:
        from literate_amd import replicates_par
        return replicates_par.run(args, 1)
    if args.ess != -1.0:
        from literate_amd.logs import ess_arg_error
        err = ess_arg_error(args.ess, args.n, args.s)
        if err:
            raise SystemExit(err)
    if args.summary != -1.0:
        from literate_amd.logs import summary_arg_error
        err = summary_arg_error(args.summary, args.n, args.s, args.chains)
        if err:
            raise SystemExit(err)
    if args.ppc != -1.0:
        from literate_amd.ppc import dd_arg_error
        err = dd_arg_error(args.ppc, args.rm_first_bin, args.ppc_draws, args.ppc_scale)
        if err:
            raise SystemExit(err)
    if args.ppc_age != -1.0:
        from literate_amd.ppc_age import arg_error as age_arg_error
        err = age_arg_error(args.ppc_age, args.ppc_age_draws, rm_first_bin=args.rm_first_bin)
        if err:
            raise SystemExit(err)
    if args.ade != -1.0:
        from literate_amd.ade import arg_error as ade_arg_error
        err = ade_arg_error(args.ade, args.ade_draws, rm_first_bin=args.rm_first_bin)
        if err:
            raise SystemExit(err)
    if args.ade_joint != -1.0:
        from literate_amd.ade_joint import arg_error as adej_arg_error
        err = adej_arg_error(args.ade_joint, args.ade_joint_n or args.n, args.ade_joint_s or args.s, args.ade_joint_win, rm_first_bin=args.rm_first_bin)
        if err:
            raise SystemExit(err)
    if args.mlik != -1.0:
        from literate_amd.mlik import arg_error as mlik_arg_error
        err = mlik_arg_error(args.mlik, args.mlik_temps, args.mlik_reps, args.mlik_n or args.n, args.mlik_s or args.s, args.mlik_alpha,
                             args.mlik_widen)
        if err:
            raise SystemExit(err)
    if args.waic != -1.0:
        from literate_amd.waic import arg_error as waic_arg_error
        err = waic_arg_error(args.waic, args.waic_draws, rm_first_bin=args.rm_first_bin)
        if err:
            raise SystemExit(err)
    if args.loo != -1.0:
        from literate_amd.loo import arg_error as loo_arg_error
        err = loo_arg_error(args.loo, args.loo_draws, rm_first_bin=args.rm_first_bin)
        if err:
            raise SystemExit(err)
    import torch
    import torch.distributed as dist
    from literate_amd import dist as lrd
    from literate_amd.ddrate import DDRateEngine, model_suffix

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group("nccl")
    seed = set_seed(args.seed)
    if world > 1:
        s = torch.tensor([seed], device="cuda")
        dist.broadcast(s, 0)
        seed = int(s.item())
    TS, TE, PRESENT, ORIGIN = parse_ts_te(args.d, args.TBP, args.first_year, args.last_year, args.death_jitter)
    offset, n_local = lrd.shard_chains(args.chains, world, rank)
    n_samples = (args.n + args.s - 1) // args.s if args.n > 0 else 0
    eng = DDRateEngine(np.asarray(TS, dtype=float), np.asarray(TE, dtype=float), ORIGIN, PRESENT, max(n_local, 1),
                       m_birth=args.m_birth, m_death=args.m_death, init_death=args.fix_death, seed=seed, s_freq=args.s,
                       n_trace_slots=n_samples, chain_offset=offset, rm_first_bin=int(args.rm_first_bin))
    if rank == 0:
        print(eng.origin, eng.present)
    emp = None
    with np.errstate(all="ignore"):
        if rank == 0:
            emp = print_empirical_rates(eng.n_spec, eng.n_exti, eng.DT)
        else:
            emp = (eng.n_spec / eng.DT, eng.n_exti / eng.DT)
    eng.init()
    stem = "%s_%s%s" % (os.path.splitext(args.d)[0], seed, model_suffix(args.m_birth, args.m_death))
    paths = [stem + ("" if args.chains == 1 else "_c%d" % (offset + c)) + ".log" for c in range(n_local)]
    # every rank writes the logs of its own chains, window by window while the next window runs (the reference writes,
    # flushes and fsyncs every sample: DD:225-238 / trend_rate.py:183-195)
    from literate_amd.engine import TraceStreamer
    streamer = TraceStreamer(eng, gather=False)
    for path in paths:
        eng.start_log(path)

    def flush_window():
        rows, snap, (s0, s1, its) = streamer.collect()
        with torch.cuda.stream(streamer.side):          # the per-bin log columns are recomputed on the side stream
            eng.append_logs(paths, rows, emp)
        if rank == 0:
            print(its, snap["likA"][0], snap["L"][0][:8])
            sys.stdout.flush()

    t_start, done = time.time(), 0
    block = args.block if args.block > 0 else args.p * max(1, 50000 // max(args.p, 1))
    while done < args.n:
        n = min(block, args.n - done)
        eng.steps(n)
        streamer.mark()
        done += n
        if len(streamer.pending) > 1:
            flush_window()
    while streamer.pending:
        flush_window()
    torch.cuda.synchronize()
    eng.check_status()
    if rank == 0 and args.n > 0:
        el = time.time() - t_start
        print("%d iterations x %d chains in %.2f s (%.0f iterations/s/chain)" % (args.n, args.chains, el, args.n / el))
    if args.ess != -1.0:
        from literate_amd.logs import write_run_ess
        write_run_ess(eng, n_local, args.chains, world, rank, args.ess, args.s, stem)
    if args.summary != -1.0:
        from literate_amd.logs import write_run_summary
        write_run_summary(eng, n_local, args.chains, world, rank, args.summary, stem)
    if args.ppc != -1.0 and n_samples:
        from literate_amd.ppc import write_run_ppc_dd
        write_run_ppc_dd(eng, n_local, args.chains, world, rank, args.ppc, args.ppc_draws, args.ppc_scale, seed, stem,
                         start_bin=args.ppc_start_bin if args.ppc_start_bin >= 0 else None)
    if args.ppc_age != -1.0 and n_samples:
        from literate_amd import ppc_age
        ppc_age.write_run(eng, n_local, args.chains, world, rank, args.ppc_age, args.ppc_age_draws, seed, stem)
    if args.ade != -1.0 and n_samples:
        from literate_amd import ade
        ade.write_run(eng, n_local, args.chains, world, rank, args.ade, args.ade_draws, stem)
    if args.ade_joint != -1.0:
        from literate_amd import ade_joint
        ade_joint.write_run(eng, args.chains, rank, args.ade_joint, args.ade_joint_n or args.n, args.ade_joint_s or args.s,
                            args.ade_joint_win, seed, stem)
    if args.mlik != -1.0:
        from literate_amd import mlik
        mlik.write_run(eng, rank, args.mlik, args.mlik_temps, args.mlik_reps, args.mlik_n or args.n, args.mlik_s or args.s,
                       args.mlik_alpha, args.mlik_widen, seed, stem, init_death=args.fix_death)
    if args.waic != -1.0 and n_samples:
        from literate_amd import waic
        waic.write_run(eng, n_local, args.chains, world, rank, args.waic, args.waic_draws, stem)
    if args.loo != -1.0 and n_samples:
        from literate_amd import loo
        loo.write_run(eng, n_local, args.chains, world, rank, args.loo, args.loo_draws, stem)
    eng.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
