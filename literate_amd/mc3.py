"""The Metropolis-coupled RJ sampler (include/literate_hip_rjmc3.h, csrc/lr_rjmc3.hip): LiteRateForward.py --mc3 T.

In runMCMC the number and the position of the rate shifts change through the reversible-jump moves alone, a fifth of the
iterations and rarely accepted.  Beside every cold chain --mc3 runs a ladder of T - 1 heated chains on L^beta * prior
(incremental heating, beta_j = 1 / (1 + dt j), as MrBayes and PyRate), which cross between shift configurations more easily
and hand their states down by swaps.  Only the cold chains are logged and summarised.

    ladder_betas      the temperatures
    TemperedEngine    ReplicateEngine's surface on lr_rjmc3_*: n_chains, trace, logs and summaries see the cold chains
    run               the command line: the replicate path (literate_amd/replicates.py) with this engine, on -d FILE (a
                      replicate set of one) or --replicates, and <stem>_MC3.tsv beside its pooled outputs
"""
import os

import numpy as np

from . import _hip
from .replicates import ReplicateEngine

MAX_TEMPS, WIDE_MAX_BINS = _hip.LR_RJMC3_MAX_TEMPS, _hip.LR_RJMC3_WIDE_MAX_BINS
WIDE_SENTENCE = ("a ladder of more than 4 temperatures holds at most %d time bins (eight bins to a lane do not fit into the registers "
                 "that a workgroup of more than four waves leaves each wave)" % WIDE_MAX_BINS)
# flags of the lineage engines' run path: (attribute, the value that leaves it off, why)
NOT_WITH_MC3 = [(name, -1.0, "--%s works on the lineages of one run of the lineage engines, and --mc3 samples on binned statistics "
                 "through the replicate path: not with --mc3" % name) for name in ("ppc", "ppc_age", "ade", "ade_joint", "waic", "loo")]


def ladder_betas(T, dt):
    """Incremental heating: beta_j = 1 / (1 + dt j), j = 0 .. T - 1; beta_0 = 1 by construction"""
    T, dt = int(T), float(dt)
    if T < 1 or T > MAX_TEMPS:
        raise ValueError("a ladder holds 1 to %d temperatures, not %d" % (MAX_TEMPS, T))
    if not dt > 0.0 or not np.isfinite(dt):
        raise ValueError("the heating increment must be a positive number, not %r" % dt)
    return [1.0 / (1.0 + dt * j) for j in range(T)]


def arg_error(args, world=1):
    """Why LiteRateForward.py --mc3 cannot run with these flags (None when it can), one sentence each"""
    if args.mc3 < 1 or args.mc3 > MAX_TEMPS:
        return "--mc3 takes 1 to %d temperatures per ladder" % MAX_TEMPS
    if not args.mc3_dt > 0.0:
        return "--mc3_dt, the heating increment of --mc3, must be positive"
    if args.mc3_every < 0:
        return "--mc3_every, the iterations between the swap rounds of --mc3, must not be negative (0: never)"
    if not args.d and not args.replicates:
        return "--mc3 needs a data file (-d) or --replicates"
    if args.d and args.replicates:
        return "--mc3 runs on -d FILE or on --replicates, not on both"
    for name, off, why in NOT_WITH_MC3:
        if getattr(args, name, off) != off:
            return why
    if getattr(args, "checkpoint", ""):
        return "--checkpoint saves one engine's workspace, which the tempered sampler does not have: not with --mc3"
    if getattr(args, "init_shifts", 0):
        return "--init_shifts builds the start of one chain, and the replicas of a ladder start from the command line's own draw: not with --mc3"
    if world > 1:
        return "--mc3 runs on one GPU (WORLD_SIZE is %d): a ladder is one workgroup, all ladders one launch" % world
    if getattr(args, "rm_first_bin", 0):
        return ("-rm_first_bin 1 makes the reference's own sampler fail with IndexError at the first K>=2 proposal "
                "(SURVEY.md section 8a A13); not supported with --mc3")
    if args.chains < 1:
        return "--chains, the number of cold chains of --mc3, must be at least 1"
    return None


class TemperedEngine(ReplicateEngine):
    """n_chains ladders of T = len(betas) replicas each: ladder g samples replicate g // chains_per_rep, and everything of
    ReplicateEngine's surface - n_chains, trace, the logs, rtt_summary, ess_summary - sees its cold chain, the replica that
    holds position 0 in the sampled iteration.  ladder [n_trace_slots, G, T, 4]: per position the replica there, its likA,
    K_l, K_m; swaps [G, T - 1, 2]: (proposed, accepted) per adjacent pair."""

    def __init__(self, reps, n_chains, betas=(1.0,), swap_every=100, **kw):
        from . import ops
        self.betas, self.swap_every = [float(b) for b in betas], int(swap_every)
        self.T = len(self.betas)
        if self.T > 4 and reps.n_bins > WIDE_MAX_BINS:
            raise ValueError("%d time bins: %s" % (reps.n_bins, WIDE_SENTENCE))
        super().__init__(reps, n_chains, **kw)
        import torch
        self.ladder = ops.alloc_output((self.n_trace_slots, self.n_chains, self.T, _hip.LR_RJMC3_LADDER_W), torch.float64, self.device, zero=True)
        self.swaps = None

    def init(self, L=None, M=None, tL=None, tM=None):
        """Initial state: the CLI's for every replica, each drawn from its own Philox key.  Given states are not taken here: a
        ladder needs one per replica, which ops.rjmc3_init(init=...) takes."""
        from . import ops
        if L is not None:
            raise ValueError("TemperedEngine.init starts every replica from the command line's own draw; pass per-replica states to ops.rjmc3_init")
        self.data.warn.zero_()
        self.state, self.swaps = ops.rjmc3_init(self.data, self.seed, self.betas, self.settings, self.chain_offset)
        self.iterations = 0

    def steps(self, n):
        from . import ops
        if self.state is None:
            raise _hip.HipLibraryError("TemperedEngine.steps before init")
        n = int(n)
        due = ops.rows_due(self.iterations, n, self.s_freq) if n > 0 else 0
        slot0 = (self.iterations + self.s_freq - 1) // self.s_freq
        if slot0 + due > self.n_trace_slots:
            raise ValueError("the trace holds %d samples; %d iterations from %d on sample up to row %d" %
                             (self.n_trace_slots, n, self.iterations, slot0 + due))
        ops.rjmc3_steps(self.data, self.state, self.swaps, self.iterations, n, self.s_freq, self.seed, self.betas, self.swap_every,
                        self.settings, self.chain_offset, rows=self.trace, ladder=self.ladder, slot0=slot0)
        self.iterations += n

    def positions(self):
        """[G, T]: the position every replica holds now"""
        S = self.state.cpu().numpy().reshape(self.n_chains, self.T, -1, _hip.LR_ROW)
        return S[:, :, _hip.LR_RJBIN_STATE_W // _hip.LR_ROW - 1, _hip.LR_RJMC3_S_POS].astype(int)

    def snapshot(self):
        """the accepted state of every cold chain - the replica at position 0 now - as ReplicateEngine.snapshot gives it"""
        from .ops import RJBIN_ROWS as R, RJBIN_SCALARS as X
        G = self.n_chains
        cold = np.argmin(self.positions(), axis=1)
        S = self.state.cpu().numpy().reshape(G, self.T, -1, _hip.LR_ROW)[np.arange(G), cold]
        sc = S[:, R["scalars"]]
        KL, KM = sc[:, X["K_l"]].astype(int), sc[:, X["K_m"]].astype(int)
        return dict(L=[S[c, R["L"], :KL[c]] for c in range(G)], M=[S[c, R["M"], :KM[c]] for c in range(G)],
                    tL=[S[c, R["tL"], :KL[c] + 1] for c in range(G)], tM=[S[c, R["tM"], :KM[c] + 1] for c in range(G)],
                    likA=sc[:, X["likA"]], priorA=sc[:, X["priorA"]], accepted=sc[:, X["accepted"]].astype(np.int64))

    def swap_table(self):
        """Per adjacent pair of positions, pooled over the ladders: dict(pair, beta_cold, beta_hot, proposed, accepted, rate)
        of arrays [T - 1] (rate: NaN where nothing was proposed)"""
        self.check_status()
        tot = self.swaps.sum(dim=0).cpu().numpy().reshape(self.T - 1, 2) if self.swaps is not None else np.zeros((self.T - 1, 2), dtype=np.int64)
        with np.errstate(all="ignore"):
            rate = np.where(tot[:, 0] > 0, tot[:, 1] / np.maximum(tot[:, 0], 1), np.nan)
        return dict(pair=np.arange(self.T - 1), beta_cold=np.array(self.betas[:-1]), beta_hot=np.array(self.betas[1:]),
                    proposed=tot[:, 0].astype(np.int64), accepted=tot[:, 1].astype(np.int64), rate=rate)

    def round_trips(self):
        """[G]: how often a replica of the ladder travelled from position 0 to position T - 1 and back, as the sampled
        iterations of the ladder buffer show it (a visit between two samples is not seen)"""
        self.check_status()
        return round_trips(self.ladder[:self.samples_done()].cpu().numpy())

    def close(self):
        super().close()
        self.ladder = self.swaps = None


def round_trips(ladder):
    """ladder [S, G, T, 4] -> [G] completed round trips 0 -> T - 1 -> 0 of the ladder's replicas"""
    ladder = np.asarray(ladder)
    S, G, T = ladder.shape[:3]
    trips = np.zeros(G, dtype=np.int64)
    if T < 2:
        return trips
    who = ladder[:, :, :, 0].astype(int)
    leg = np.zeros((G, T), dtype=np.int8)          # per replica: 1 = has been cold and not hot since, 2 = hot since then
    rows = np.arange(G)
    for s in range(S):
        top, bottom = who[s, :, 0], who[s, :, T - 1]
        trips += leg[rows, top] == 2
        leg[rows, top] = 1
        leg[rows, bottom] = np.where(leg[rows, bottom] == 1, 2, leg[rows, bottom])
    return trips


def write_mc3_table(path, eng):
    """<stem>_MC3.tsv: the ladder and the swap rate of every adjacent pair, then the round trips of every ladder"""
    tab, trips = eng.swap_table(), eng.round_trips()
    with open(path, "w") as f:
        f.write("# %d ladders of %d temperatures, a swap round every %d iterations\n" % (eng.n_chains, eng.T, eng.swap_every))
        f.write("pair\tbeta_cold\tbeta_hot\tproposed\taccepted\trate\n")
        for j in range(eng.T - 1):
            f.write("%d\t%r\t%r\t%d\t%d\t%r\n" % (j, float(tab["beta_cold"][j]), float(tab["beta_hot"][j]), tab["proposed"][j],
                                                   tab["accepted"][j], float(tab["rate"][j])))
        f.write("# round trips (position 0 to %d and back) seen in the sampled iterations\n" % (eng.T - 1))
        f.write("ladder\tround_trips\n")
        for g, n in enumerate(trips):
            f.write("%d\t%d\n" % (g, n))


def run(args, parse=None):
    """LiteRateForward.py --mc3 T: the replicate path (replicates.run) on tempered ladders.  -d FILE is a replicate set of one
    and its pooled outputs carry the data file's stem; --chains stays the number of cold chains."""
    from . import logs, replicates
    err = arg_error(args, int(os.environ.get("WORLD_SIZE", "1")))
    if err:
        raise SystemExit(err)
    try:
        files = [args.d] if args.d else replicates.expand_pattern(args.replicates)
        betas = ladder_betas(args.mc3, args.mc3_dt)
    except ValueError as e:
        raise SystemExit(str(e))
    name = None
    if args.d:
        name = os.path.splitext(os.path.basename(args.d))[0] + logs.SUFFIX[args.model_BDI] + args.out

    def engine(reps, n_chains, **kw):
        try:
            eng = TemperedEngine(reps, n_chains, betas=betas, swap_every=args.mc3_every, **kw)
        except ValueError as e:
            raise SystemExit(str(e))
        print("--mc3: %d temperatures, betas %s, a swap round every %d iterations" % (eng.T, " ".join("%.4g" % b for b in betas), eng.swap_every))
        return eng

    def finish(eng, stem):
        write_mc3_table(stem + "_MC3.tsv", eng)
        tab = eng.swap_table()
        print("swap rates per pair: %s; round trips per ladder: mean %.2f (%s_MC3.tsv)" %
              (" ".join("%.3f" % r for r in tab["rate"]), float(np.mean(eng.round_trips())), stem))
    return replicates.run(args, parse, files=files, name=name, engine=engine, finish=finish)
