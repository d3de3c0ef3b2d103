#!/usr/bin/env python
"""MTEmodel.py - multi-trait extinction with Bayesian variable selection (the model of the reference's other/MTEmodel.py) on
MI355X GPUs through literate_amd: every lineage carries several categorical traits, its extinction rate is a mean rate times
the sum of one softmax multiplier per trait, and an indicator per trait says whether the trait matters at all.

    python MTEmodel.py -d table.txt --slice_edges 23,8,0 --chains 16 -n 100000 -s 100 --summary 0.2

Flags of the reference: -d -n -s -p -t0 -t1 -seed -mu_species -traits -const -out -bvs -pI (-A 1 is refused: marginal likelihoods
of this model are not built).  New: --chains (per slice), --slices 'a-b,c-d,...' or --slice_edges e0,e1,... (all slices in one
launch; without either the one slice of -t0 / -t1), --bvs_from (the first iteration an indicator may flip at), --block,
--ess F, --summary F.  Logs: the reference's file per slice (`_c<k>` with several chains) with its header; after the run
<stem>_MTE.tsv (P(I = 1) and 2 ln BF per trait, mean and 95 % HPD of every multiplier, of m, sd and beta_hp, the acceptance
per move kind) with the burn-in fraction --summary dropped, the chains of a slice pooled.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    import argparse
    p = argparse.ArgumentParser()
    p.add_argument('-A', type=int, help='marginal likelihood: not built (refused)', default=0, metavar=0)
    p.add_argument('-d', type=str, help='input file', default="", metavar="<inputfile.txt>")
    p.add_argument('-n', type=int, help='mcmc generations', default=100000, metavar=100000)
    p.add_argument('-s', type=int, help='sample freq.', default=100, metavar=100)
    p.add_argument('-p', type=int, help='print freq.', default=1000, metavar=1000)
    p.add_argument('-t0', type=float, help='max age time slice', default=np.inf, metavar=np.inf)
    p.add_argument('-t1', type=float, help='min age time slice', default=0, metavar=0)
    p.add_argument('-seed', type=int, help='seed (if -1 -> random)', default=-1, metavar=-1)
    p.add_argument('-mu_species', type=int, help='set to 1 to save extinction rates for each trait combination', default=0, metavar=0)
    p.add_argument('-traits', type=int, help="index trait(s)", metavar='', nargs='+', default=[])
    p.add_argument('-const', type=int, help="if set to 1: trait independent rate", metavar=0, default=0)
    p.add_argument('-out', type=str, help='output string', default="", metavar="")
    p.add_argument('-bvs', type=int, help='use Bayesian Variable Selection', default=1, metavar=1)
    p.add_argument('-pI', type=float, help='prior on indicators', default=0.05, metavar=0.05)
    p.add_argument('--chains', type=int, default=1, help='number of independent chains per slice')
    p.add_argument('--slices', type=str, default="", help="time slices 'a-b,c-d,...' (older age first), all in one launch")
    p.add_argument('--slice_edges', type=str, default="", help="edges 'e0,e1,...' of consecutive time slices, all in one launch")
    p.add_argument('--bvs_from', type=int, default=1001, help='the first iteration an indicator may flip at')
    p.add_argument('--block', type=int, default=0, help='iterations per launch: logs are written and flushed once per launch')
    p.add_argument('--ess', type=float, default=-1.0, help='after the run, write <stem>_ESS.tsv and _ESS_chains.tsv per slice')
    p.add_argument('--summary', type=float, default=-1.0, help='after the run, write <stem>_MTE.tsv with this burn-in fraction dropped')
    return p


def main(argv=None):
    from literate_amd import mte
    args = build_parser().parse_args(argv)
    err = mte.arg_error(args, int(os.environ.get("WORLD_SIZE", "1")))
    if err:
        raise SystemExit(err)
    if args.ess != -1.0:
        from literate_amd.logs import ess_arg_error
        err = ess_arg_error(args.ess, args.n, args.s)
        if err:
            raise SystemExit(err)
    print("\n\n             LiteRate - multi-trait extinction (MI355X engine)\n")
    return mte.run(args)


if __name__ == "__main__":
    main()
