#!/usr/bin/env python3
"""MultiTrendRate.py - the joint covariate model on MI355X GPUs through literate_amd: every birth and death rate is
log-linear in several columns of the trend file at once, and an indicator per covariate and side says whether it matters once
the others are in the model (Bayesian variable selection).

    python MultiTrendRate.py -d data.tsv -trend_data trend.tsv --columns all --with_diversity --chains 256 -n 1000000 -s 1000 --summary 0.2

The data and the trend file are trend_rate.py's (-d, -trend_data, -rm_first_bin, -TBP, -const_B, -const_D, -no_death, -seed);
--columns picks the columns (all, or i,j,k), each standardised over the bins in use; --with_diversity adds the clade's own
diversity as one more column.  -bvs 1 -pI 0.1 -slab_sd 1: selection, the prior probability of an indicator and the sd of the
Normal prior on a coefficient; --tune 0.1: the share of the run the two coefficient windows are tuned in; --bvs_from N: the
first iteration an indicator may flip at (default: the end of the tuning).  Logs: one per chain,
<data>_<seed><model suffix>_joint[_c<k>].multitrend.log; after the run, with --summary F (the burn-in fraction dropped, chains
pooled): <data>_joint_MT.tsv (P(I = 1), 2 ln BF, the coefficient given inclusion, the model-averaged effect with ESS and split
R-hat, acceptance, windows), <data>_joint_MT_models.tsv (the 20 most visited indicator patterns) and <data>_joint_MT_rates.tsv
(birth and death rate per bin).  trend_rate.py's other extensions are refused with their reason.
"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def build_parser():
    from literate_amd.literate_library import core_arguments
    p = core_arguments()
    p.add_argument('-trend_data', metavar='<path to trend file>', type=str,
                   help='Input trend file should be columns tab-separated with headers. No missing values.', default="")
    p.add_argument('--columns', type=str, default='all', help='covariates: all (every column of the trend file) or a '
                   'comma-separated list of column indices; each standardised over the bins in use')
    p.add_argument('--with_diversity', action='store_true', help='append the clade\'s own diversity (lineage-time per bin), '
                   'standardised, as the covariate `diversity`')
    p.add_argument('-const_B', type=bool, help='F) birth rates vary with the covariates T) constant', default=False, metavar=False)
    p.add_argument('-const_D', type=bool, help='F) death rates vary with the covariates T) constant', default=False, metavar=False)
    p.add_argument('-no_death', type=bool, help='F) Calculate death rate T) Likelihood based on births only', default=False, metavar=False)
    p.add_argument('-bvs', type=int, default=1, help='1) Bayesian variable selection 0) every covariate is in the model')
    p.add_argument('-pI', type=float, default=0.1, help='prior probability of an indicator')
    p.add_argument('-slab_sd', type=float, default=1.0, help='sd of the Normal prior on a coefficient (the Bayes factors depend on it)')
    p.add_argument('--bvs_from', type=int, default=-1, help='the first iteration an indicator may flip at (default: the end of the tuning)')
    p.add_argument('--tune', type=float, default=0.1, help='share of the run in which the two coefficient windows are tuned towards 30 %% acceptance')
    p.add_argument('--chains', type=int, default=1, help='number of independent chains')
    p.add_argument('--block', type=int, default=0, help='iterations per launch: logs are written and flushed once per launch')
    p.add_argument('--summary', type=float, default=-1.0, help='after the run, write <data>_joint_MT.tsv, _MT_models.tsv and _MT_rates.tsv '
                   'with this burn-in fraction dropped, chains pooled')
    p.add_argument('--ess', type=float, default=-1.0, help='after the run, write <data>_joint_MT_ESS.tsv and _ESS_chains.tsv')
    # trend_rate.py's extensions that the joint model does not take: refused with their reason (literate_amd/multitrend.py)
    p.add_argument('--replicates', type=str, default='', help='refused')
    for flag in ('--mlik', '--ppc', '--ppc_age', '--ade', '--ade_joint', '--waic', '--loo'):
        p.add_argument(flag, type=float, default=-1.0, help='refused')
    p.add_argument('--mc3', type=int, default=0, help='refused')
    return p


def main(argv=None):
    from literate_amd import multitrend
    args = build_parser().parse_args(argv)
    err = multitrend.arg_error(args, int(os.environ.get("WORLD_SIZE", "1")))
    if err:
        raise SystemExit(err)
    if args.ess != -1.0:
        from literate_amd.logs import ess_arg_error
        err = ess_arg_error(args.ess, args.n, args.s)
        if err:
            raise SystemExit(err)
    print("\n\n             LiteRate - joint covariate model (MI355X engine)\n")
    return multitrend.run(args)


if __name__ == "__main__":
    main()
