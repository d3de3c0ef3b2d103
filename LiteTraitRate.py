#!/usr/bin/env python
"""LiteTraitRate.py - trait-dependent birth and death rates (the model of the reference's other/LiteTraitRate.py) on MI355X GPUs
through literate_amd: the RJ skylines of LiteRateForward.py, every lineage's rates multiplied by a logistic function of one
static real trait,

    lambda_i(t) = lambda(t) / (1 + exp(-kappa_l (x_i - x0_l))),      mu_i(t) = mu(t) / (1 + exp(-kappa_m (x_i - x0_m))).

Flags: core_arguments() of literate_library, the RJ flags of LiteRateForward.py and --chains; -trait_data FILE (tab-separated, a
header row, then `lineage_name value` rows, matched to -d by the name in its first column), -trait_raw (do not standardise),
--trait_every K (a trait move every K iterations), --trait_win_x0 / --trait_win_kappa (the sliding windows, the reference's
d_win), --trait_tune F (tune the windows during the first F of -n; 0 keeps them).  Logs, in the reference's format, under
literate_mcmc_logs/: <stem>_trait_mcmc.log, _trait_sp_rates.log, _trait_ex_rates.log (_c<k> with several chains); after the run
<stem>_trait_effect.tsv and <stem>_trait_curves.tsv; --rtt and --ess as LiteRateForward.py (the baseline skylines: the rates at
multiplier s = 1).  Only the Keiding likelihood (-model_BDI 2, the default here) is built.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    from literate_amd.literate_library import core_arguments
    p = core_arguments()
    p.add_argument('-const_rates', type=int, help="set to: 1 for constant baseline B and D rates", default=0, metavar=0)
    p.add_argument('-const_death_rate', type=int, help="set to: 1 for a constant baseline D rate", default=0, metavar=0)
    p.add_argument('-model_BDI', type=int, help='2: birth-death (Keiding likelihood), the only one built here', default=2, metavar=2)
    p.add_argument('-use_rate_HP', type=int, help='0: no hyper-prior on rates, 1: hyper-prior on rates', default=1, metavar=1)
    p.add_argument('-Poisson_prior', type=float, help='0: use hyper-prior on n. shifts, >0:  fixed prior on n. shifts', default=0, metavar=0)
    p.add_argument('-update_fraction', type=float, help='', default=0.75, metavar=0.75)
    p.add_argument('-out', type=str, help='output tag', default="", metavar="")
    p.add_argument('-trait_data', type=str, default="", metavar="", help='trait file: tab-separated, a header row, then '
                   '`lineage_name value` rows; matched to -d by name')
    p.add_argument('-trait_raw', default=False, action='store_true', help='use the trait values as given (default: standardised '
                   'to mean 0, sd 1; the mean and sd are written to the log header)')
    p.add_argument('--chains', type=int, default=1, help='number of independent chains')
    p.add_argument('--trait_every', type=int, default=10, help='a trait move every this many iterations (0: never)')
    p.add_argument('--trait_win_x0', type=float, default=0.5, help='sliding window of the midpoints x0')
    p.add_argument('--trait_win_kappa', type=float, default=0.1, help='sliding window of the steepnesses kappa')
    p.add_argument('--trait_tune', type=float, default=0.1, help='fraction of -n during which the trait windows are tuned per side '
                   'towards 30 %% acceptance (0: keep the given windows); its rows are logged but left out of the summary')
    p.add_argument('--block', type=int, default=0, help='iterations per device window: logs are written and flushed once per window')
    p.add_argument('--rtt', type=float, default=-1.0, help='after the run, write <stem>_trait_RTT.tsv: the BASELINE rates through '
                   'time (the rates at multiplier s = 1), pooled over all chains with this burn-in fraction dropped')
    p.add_argument('--ess', type=float, default=-1.0, help='after the run, write <stem>_trait_ESS.tsv and _ESS_chains.tsv')
    # flags of LiteRateForward.py that this sampler refuses by name (literate_amd.traitrate.REFUSED)
    p.add_argument('--replicates', type=str, default="")
    p.add_argument('--mc3', type=int, default=1)
    for flag in ("ppc", "ppc_age", "ade", "ade_joint", "waic", "loo"):
        p.add_argument('--' + flag, type=float, default=-1.0)
    return p


def main(argv=None):
    from literate_amd import traitrate
    args = build_parser().parse_args(argv)
    err = traitrate.arg_error(args, int(os.environ.get("WORLD_SIZE", "1")))
    if err:
        raise SystemExit(err)
    if args.ess != -1.0:
        from literate_amd.logs import ess_arg_error
        err = ess_arg_error(args.ess, args.n, args.s)
        if err:
            raise SystemExit(err)
    print("\n\n             LiteRate - trait-dependent rates (MI355X engine)\n")
    return traitrate.run(args)


if __name__ == "__main__":
    main()
