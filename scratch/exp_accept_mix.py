"""How often does a chain's ACCEPTED STATE change per iteration on cfg4-sized data?  (CPU, oracle loop on binned
statistics = the same trajectory as the device's.)  What the reject-speculation of the four-chain kernel rides on.

    python scratch/exp_accept_mix.py [lineages]
    python scratch/exp_accept_mix.py draws [chains]    the share of iterations in which the four-chain kernel's lean draw
                                                       duty (lr_spec_draw_lean) skips the multiplier part, on cfg4"""
import sys, os
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from literate_amd import synth
from oracle import literate_oracle as lo, mcmc_oracle as mo



class RecordingDraws(mo.PhiloxDraws):
    """PhiloxDraws that keeps what the lean duty's test reads: the move selectors of every iteration, and by how much the
    proposal of an iteration changes the number of rates of which process"""

    def __init__(self, seed, chain):
        super().__init__(seed, chain)
        self.r, self.side, self.dk, self.mult = {}, {}, {}, set()

    def move(self, it):
        self.r[it] = super().move(it)
        return self.r[it]

    def multiplier(self, it, K, f):
        self.mult.add(it)
        return super().multiplier(it, K, f)

    def rj_select(self, it):
        q = super().rj_select(it)
        self.side[it] = 0 if q[0] > 0.5 else 1
        return q

    def rj_add(self, it, times):
        self.dk[it] = 1
        return super().rj_add(it, times)

    def rj_remove(self, it, K):
        self.dk[it] = -1
        return super().rj_remove(it, K)


def skipped_share(n_chains):
    """lr_spec_draw_lean's test for the draws of iteration j, made while proposal j - 1 is pending: r_a < 0.8 and (r_b < .5
    or the process r_a selects holds ONE rate in the accepted state or in the pending proposal)."""
    ts, te, _ = synth.make_lineages(100_000, n_bins=128, n_shifts=20, seed=0)          # bench.py's cfg4
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    stats = dict(sp=sp, ex=ex, br=br)
    n_it = 5000
    windows = ((200, 2200), (3000, 5000))
    made = {w: [0, 0, 0] for w in windows}          # iterations, multiplier parts made, multiplier moves proposed
    for chain in range(n_chains):
        d = RecordingDraws(2026, chain)
        with np.errstate(all="ignore"):
            out = mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=0), d, n_it, 1, k_max=32)
        K = np.vstack([[1, 1], np.array(out["mcmc"])[:, 6:8].astype(int)])          # K[j]: accepted before iteration j
        for w in windows:
            for j in range(*w):
                acc = K[j - 1]                                   # the state proposal j - 1 was made from
                pend = acc.copy()
                if j - 1 in d.dk:
                    pend[d.side[j - 1]] += d.dk[j - 1]
                r_a, r_b = d.r[j]
                p = 0 if r_a < 0.4 else 1
                need = r_a < 0.8 and (r_b < .5 or acc[p] == 1 or pend[p] == 1)
                assert need or j not in d.mult, (chain, j)       # never skipped where the move reads the draws
                made[w][0] += 1
                made[w][1] += bool(need)
                made[w][2] += j in d.mult
    for w in windows:
        n, m, used = made[w]
        print("iterations %d..%d of %d chains: multiplier part skipped in %.1f %% of the iterations (made %.1f %%, read by the "
              "move %.1f %%)" % (w[0], w[1], n_chains, 100.0 * (n - m) / n, 100.0 * m / n, 100.0 * used / n))


if len(sys.argv) > 1 and sys.argv[1] == "draws":
    skipped_share(int(sys.argv[2]) if len(sys.argv) > 2 else 8)
    sys.exit(0)

n_lin = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
ts, te, _ = synth.make_lineages(n_lin, n_bins=128, n_shifts=20, seed=0)
t0, sp, ex, br = lo.bin_events_cli(ts, te)
stats = dict(sp=sp, ex=ex, br=br)
for chain in range(3):
    n_it = 30000
    with np.errstate(all="ignore"):
        out = mo.run_mcmc(stats, ts.min(), te.max(), mo.Settings(model_BDI=0), mo.PhiloxDraws(2026, chain), n_it, 1, k_max=32)
    rows = np.array(out["mcmc"])
    for a, b in ((0, 3000), (3000, 10000), (10000, 30000)):
        r = rows[a:b]
        changed = (np.diff(r[:, 2]) != 0) | (np.diff(r[:, 6]) != 0) | (np.diff(r[:, 7]) != 0)
        gibbs = (np.diff(r[:, 10]) != 0) | (np.diff(r[:, 12]) != 0)
        print("chain %d iterations %5d..%5d: state changed %.3f, gibbs %.4f, K_l %.1f K_m %.1f" % (
            chain, a, b, changed.mean(), gibbs.mean(), r[:, 6].mean(), r[:, 7].mean()))
