"""The GPU cases of tests/test_hip_dd_sim_batch.py, each run in a child process of its own (under the test's time limit):

    python tests/helpers/dd_sim_cases.py CASE [ARGS...]

A case prints its figures, asserts, and exits 0 - or raises.  Yardsticks: ops.simulate_bd_batch (m_birth 0, m_death 0:
exact, no condition), tests/helpers/dd_sim_ref.py (the numpy restatement), oracle/sim_oracle.py and ops.simulate_bd in
mode 1.  Every simulator output is an integer and every comparison is np.array_equal.

When the device and the restatement may differ.  The device forms x ** nu as exp(nu * lr_log x), numpy calls pow, so the
two sets of thresholds differ in their last bits, and a draw that falls between them decides differently.  Every
comparison with the restatement (or with the mode-1 simulators, whose rates are l0 - l0 D / K without a power) therefore
carries one condition, asserted on the CPU side BEFORE the comparison: the restatement's smallest distance between any
draw and either threshold is at least FLOOR = 1e-11.  The floor is a condition, not a measurement.  What the two
evaluations can differ by is bounded by tests/helpers/math_edges.rate_bound, the bound tests/test_hip_math_edges.py holds
lr_dd_rates to against the long-double evaluation: 2 (scale p (e_y + 3 eps) + eps rate) with e_y = |nu| (e_frac + 1.2 eps
|log frac|) + eps |nu log frac|, e_frac = (2 |k (x - x0)| + 5) eps.  In the cases below |k (x - x0)| <= 30, |log frac| <=
9, |nu| <= 2 and scale p <= 1.3, so e_y <= 170 eps and a rate is within 450 eps = 5e-14 of the long-double value; numpy's
evaluation (pow within an ulp, the same other operations) lies within the same bound, the two are at most 1e-13 apart, and
a threshold - a rate over steps_per_bin >= 8, or the sum of two - at most 2.5e-14.  FLOOR is 400 times that."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import dd_sim_ref  # noqa: E402
from helpers.sim_batch_cases import NB, SPB, header_int, mixed_rates, same  # noqa: E402

FLOOR = 1e-11
X = np.arange(NB, dtype=float)

# `created` of the twelve replicates of case_branches, from tests/helpers/dd_sim_ref.py (the issue's figures)
CREATED_2 = {(2, 2): [1913, 2266, 2233, 2991, 3144, 840, 4263, 646, 1681, 1765, 2969, 3048],
             (1, 1): [2693, 2768, 2380, 4816, 4665, 980, 7237, 740, 2452, 3170, 3165, 6253],
             (1, 0): [2003, 1958, 1799, 3814, 3471, 765, 5485, 633, 1859, 2308, 2727, 5140],
             (2, -1): [1526, 1580, 1706, 2625, 2604, 696, 3687, 556, 1414, 1493, 2601, 3027],
             (2, 1): [1871, 2206, 2233, 3042, 3113, 836, 4216, 639, 1645, 1754, 2966, 3126]}
MODE1 = dict(par=[.5, 1, 0, 50, 450, .1, 1, 1], n_start=40, seed=300, created=[1332, 1373, 1296, 1352], living=[340, 332, 330, 333])
ABOVE = dict(par=[.3, 1, 0, 20, 80, .2, 1, 1], n_start=400, seed=50, created=[522, 547, 490], living=[29, 22, 14])
LDS = dict(par=[.6, 1, 0, 1000, 39000, .05, 1, 1], n_bins=32, spb=100, n_start=20, seed=7, created=89381, living=33901, peak=33941)


def branch_params():
    rng = np.random.default_rng(17)
    return np.array([[rng.uniform(.4, .9), rng.uniform(.3, 1.5), rng.uniform(4, 16), rng.uniform(5, 40), rng.uniform(300, 3000),
                      rng.uniform(.03, .15), rng.uniform(.5, 2), rng.uniform(.5, 2)] for _ in range(12)])


def const_params(l_max, m_max, n):
    """n rows whose rates under (0, 0) are l_max, m_max; the other six parameters are not read"""
    p = np.tile([0., 1., 5., 10., 100., 0., 1., 1.], (n, 1))
    p[:, 0], p[:, 5] = l_max, m_max
    return p


def dd_batch(par, x, spb, n_start, seed, mb, md, capacity=None):
    from literate_amd import ops
    counts, totals = ops.simulate_dd_batch(par, x, spb, n_start, seed, mb, md, capacity=capacity)
    return counts.cpu().numpy(), totals.cpu().numpy()


def clear_of_thresholds(what, closest):
    """the condition every comparison with the restatement carries"""
    print("%s: smallest distance between a draw and a threshold in the restatement %.3g (floor %.0e)" % (what, closest, FLOOR))
    sys.stdout.flush()
    assert closest >= FLOOR, (what, closest)


def against_restatement(what, counts, totals, par, x, spb, n_start, seed, mb, md, reps, capacity=None):
    """replicates `reps` of a device batch against the restatement, one by one"""
    par, x = np.atleast_2d(par), np.asarray(x, dtype=float)
    n0 = np.full(len(par), n_start) if np.ndim(n_start) == 0 else np.asarray(n_start)
    cap = capacity or max(64 * int(n0.max()), 1 << 20)
    for r in reps:
        rc, rt, closest = dd_sim_ref.simulate_one(par[r], x if x.ndim == 1 else x[r], spb, n0[r], seed + r, mb, md, cap)
        clear_of_thresholds("%s replicate %d" % (what, r), closest)
        same("%s replicate %d counts vs the restatement" % (what, r), counts[r], rc)
        same("%s replicate %d totals vs the restatement" % (what, r), totals[r], rt)


def case_exact():
    """m_birth 0, m_death 0: the thresholds are l_max / spb and m_max / spb, the existing kernel's own - no condition"""
    from literate_amd import ops
    la, mu = mixed_rates()
    par = const_params(la[:, 0], mu[:, 0], 12)
    counts, totals = dd_batch(par, X, SPB, 300, 1000, 0, 0)
    bc, bt = ops.simulate_bd_batch(np.repeat(la[:, :1], NB, 1), np.repeat(mu[:, :1], NB, 1), SPB, 300, 1000)
    print("created", totals[:, 0].tolist())
    assert totals[:, 0].min() > 300 and not totals[:, 2].any()
    same("constant rates: counts vs simulate_bd_batch", counts, bc.cpu().numpy())
    same("constant rates: totals vs simulate_bd_batch", totals, bt.cpu().numpy())
    counts, totals = dd_batch(const_params(.02, .6, 3), X, SPB, 50, 3, 0, 0)
    bc, bt = ops.simulate_bd_batch(np.full((3, NB), .02), np.full((3, NB), .6), SPB, 50, 3)
    print("first empty step", totals[:, 3].tolist())
    same("first empty step", totals[:, 3], np.array([59, 77, 46]))
    same("extinction: counts vs simulate_bd_batch", counts, bc.cpu().numpy())
    same("extinction: totals vs simulate_bd_batch", totals, bt.cpu().numpy())


def case_branches(mb, md):
    """every branch of the rate map: constant / fixed niche / logistic niche on either side; under (2, 1) the death side
    recomputes the niche"""
    mb, md = int(mb), int(md)
    par = branch_params()
    counts, totals = dd_batch(par, X, SPB, 30, 2000, mb, md)
    print("created", totals[:, 0].tolist(), "most alive at a bin start", int(counts[:, 2].max()))
    assert not totals[:, 2].any()                                       # nothing overflows at the default capacity
    same("created vs the pinned figures", totals[:, 0], np.array(CREATED_2[(mb, md)]))
    if (mb, md) == (2, 2):
        assert int(counts[:, 2].max()) == 2204
    against_restatement("(%d, %d)" % (mb, md), counts, totals, par, X, SPB, 30, 2000, mb, md, range(12))


def case_mode1():
    """the fixed niche with both exponents 1 is notebook 4's diversity dependence: l0 - l0 D / K, m0 + m0 D / K, K = L + div_0"""
    from oracle import sim_oracle
    from literate_amd import ops
    from helpers.sim_batch_cases import counts_from_run
    c = MODE1
    par = np.tile(c["par"], (4, 1))
    counts, totals = dd_batch(par, X, SPB, c["n_start"], c["seed"], 1, 1)
    print("created", totals[:, 0].tolist(), "living at the end", totals[:, 1].tolist(), "(K (l - m) / (l + m) = 333)")
    same("created", totals[:, 0], np.array(c["created"]))
    same("living at the end", totals[:, 1], np.array(c["living"]))
    against_restatement("mode 1", counts, totals, par, X, SPB, c["n_start"], c["seed"], 1, 1, range(4))
    for r in range(4):
        ts, te, trace = sim_oracle.simulate_bd(c["n_start"], NB * SPB, c["seed"] + r, mode=1, l0=.5, m0=.1, K=500., scale=float(SPB))
        oc, ot = counts_from_run(ts, te, trace, c["n_start"], NB, SPB)
        same("replicate %d counts vs sim_oracle mode 1" % r, counts[r], oc)
        same("replicate %d totals vs sim_oracle mode 1" % r, totals[r], ot)
        ts, te, trace = ops.simulate_bd(c["n_start"], NB * SPB, c["seed"] + r, mode=1, l0=.5, m0=.1, K=500., scale=float(SPB))
        sc, st = counts_from_run(ts.cpu().numpy(), te.cpu().numpy(), trace.cpu().numpy(), c["n_start"], NB, SPB)
        same("replicate %d counts vs simulate_bd mode 1" % r, counts[r], sc)
        same("replicate %d totals vs simulate_bd mode 1" % r, totals[r], st)


def case_above_niche():
    """a start above the niche: the birth rate sits on the 1e-15 floor while frac > 1"""
    c = ABOVE
    par = np.tile(c["par"], (3, 1))
    counts, totals = dd_batch(par, X, SPB, c["n_start"], c["seed"], 1, 1)
    print("created", totals[:, 0].tolist(), "living at the end", totals[:, 1].tolist(), "births in bin 0", counts[:, 0, 0].tolist())
    same("created", totals[:, 0], np.array(c["created"]))
    same("living at the end", totals[:, 1], np.array(c["living"]))
    against_restatement("above the niche", counts, totals, par, X, SPB, c["n_start"], c["seed"], 1, 1, range(3))


def case_beyond_lds():
    """a list that outgrows LDS in mid-run while the feedback levels it off at the niche"""
    c = LDS
    par = np.tile(c["par"], (2, 1))
    x = np.arange(c["n_bins"], dtype=float)
    counts, totals = dd_batch(par, x, c["spb"], c["n_start"], c["seed"], 1, 1)
    lds = header_int("LR_SIMBATCH_LDS_SLOTS")
    print("created", totals[:, 0].tolist(), "living at the end", totals[:, 1].tolist(), "peak at a bin start",
          counts[:, 2].max(1).tolist(), "list positions in LDS", lds)
    assert (totals[0, 0], totals[0, 1], counts[0, 2].max()) == (c["created"], c["living"], c["peak"])
    assert counts[0, 2].max() > lds > c["n_start"]                      # starts inside LDS, outgrows it in mid-run
    against_restatement("beyond LDS", counts, totals, par, x, c["spb"], c["n_start"], c["seed"], 1, 1, range(2))
    c2, t2 = dd_batch(par, x, c["spb"], c["n_start"], c["seed"], 1, 1, capacity=100000)
    same("capacity 100000 counts", c2, counts)
    same("capacity 100000 totals", t2, totals)
    c3, t3 = dd_batch(par, x, c["spb"], c["n_start"], c["seed"], 1, 1, capacity=50000)
    print("capacity 50000: overflow flags", t3[:, 2].tolist())
    same("capacity 50000 flags", t3[:, 2], np.array([1, 1]))


def case_batch():
    """more replicates than workgroups, per-replicate starts, refused starts, a second call, the shared x_bins form"""
    groups = header_int("LR_SIMBATCH_GROUPS")
    P = branch_params()
    c1, t1 = dd_batch(P, X, SPB, 30, 2000, 2, 2)
    R = 600
    assert R > groups
    rng = np.random.default_rng(11)
    par = np.tile(P, (R // 12, 1))
    n0 = np.concatenate([np.full(12, 30), rng.integers(1, 9, R - 12)])
    counts, totals = dd_batch(par, X, SPB, n0, 2000, 2, 2)
    print("%d replicates on at most %d workgroups" % (R, groups))
    same("first twelve: counts", counts[:12], c1)
    same("first twelve: totals", totals[:12], t1)
    assert not totals[:, 2].any()
    against_restatement("600", counts, totals, par, X, SPB, n0, 2000, 2, 2, (groups - 1, groups, R - 1))
    c2, t2 = dd_batch(par, X, SPB, n0, 2000, 2, 2)
    same("second call: counts", c2, counts)
    same("second call: totals", t2, totals)
    c3, t3 = dd_batch(par, np.tile(X, (R, 1)), SPB, n0, 2000, 2, 2)
    same("x_bins tiled: counts", c3, counts)
    same("x_bins tiled: totals", t3, totals)
    # per-replicate starts with one refused (0) and one above the capacity
    n1 = 10 + 5 * np.arange(12)
    cg, tg = dd_batch(P, X, SPB, n1, 2000, 2, 2, capacity=50000)
    assert not tg[:, 2].any()
    against_restatement("starts", cg, tg, P, X, SPB, n1, 2000, 2, 2, range(12), capacity=50000)
    bad = n1.copy()
    bad[3], bad[9] = 0, 50001
    cb, tb = dd_batch(P, X, SPB, bad, 2000, 2, 2, capacity=50000)
    print("overflow flags", tb[:, 2].tolist())
    same("flags", tb[:, 2], np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0]))
    same("refused starts report nothing else", tb[[3, 9]], np.array([[0, 0, 1, -1]] * 2))
    assert not cb[[3, 9]].any()
    keep = tb[:, 2] == 0
    same("the other ten: counts", cb[keep], cg[keep])
    same("the other ten: totals", tb[keep], tg[keep])


def case_arguments():
    """every argument error returns before anything is launched"""
    import torch
    from literate_amd import _hip
    lib = _hip.load()
    P = _hip.ptr
    par = torch.tensor(const_params(.1, .1, 3), device="cuda")
    x = torch.zeros((3, 5), dtype=torch.float64, device="cuda")
    n0 = torch.full((3,), 10, dtype=torch.int64, device="cuda")
    cnt = torch.zeros((3, 4, 5), dtype=torch.int64, device="cuda")
    tot = torch.zeros((3, 4), dtype=torch.int64, device="cuda")
    q = lib.lr_simulate_dd_batch_workspace_bytes
    need = q(3, 5, 4, 1000)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(par=par, x=x, mb=2, md=2, R=3, nb=5, spb=4, start=n0, cap=1000, counts=cnt, totals=tot, work=ws, nbytes=need):
        return lib.lr_simulate_dd_batch(P(par), P(x), mb, md, R, nb, spb, P(start), cap, 1, P(counts), P(totals), P(work), nbytes, None)

    for kw in (dict(par=None), dict(x=None), dict(start=None), dict(counts=None), dict(totals=None), dict(work=None)):
        assert call(**kw) == _hip.LR_ERR_NULL, kw
    for kw in (dict(R=0), dict(nb=0), dict(spb=0), dict(nb=_hip.LR_MAX_BINS + 1), dict(cap=0), dict(cap=1 << 31)):
        assert call(**kw) == _hip.LR_ERR_SIZE, kw
    for kw in (dict(mb=-1), dict(mb=3), dict(md=-3), dict(md=3)):
        assert call(**kw) == _hip.LR_ERR_MODEL, kw
    assert call(nbytes=need - 1) == _hip.LR_ERR_WORKSPACE
    assert q(3, 5, 4, 100000) > need and call(cap=100000) == _hip.LR_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert not cnt.any() and not tot.any()                   # nothing was launched
    for mb, md in ((0, -2), (2, 2)):
        assert call(mb=mb, md=md) == 0
    torch.cuda.synchronize()
    assert tot[:, 0].min() >= 10


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
