"""The GPU cases of tests/test_hip_sim_batch.py, each run in a child process of its own (under the test's time limit):

    python tests/helpers/sim_batch_cases.py CASE

A case prints its figures, asserts, and exits 0 - or raises.  Yardsticks: oracle/sim_oracle.py and ops.simulate_bd, one
run per replicate; every comparison is np.array_equal on integers."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

NB, SPB = 24, 8            # the geometry of case 1


def header_int(name):
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, f.read()).group(1))


def counts_from_run(ts, te, trace, n_start, n_bins, spb):
    """(counts [4, n_bins], totals [4]) of ONE run's birth steps, death steps and living count per step"""
    ts, te, trace = np.asarray(ts), np.asarray(te), np.asarray(trace)
    n_steps = n_bins * spb
    births = np.bincount((ts // spb).astype(np.int64), minlength=n_bins)
    births[0] -= n_start
    deaths = np.bincount((te[te < n_steps] // spb).astype(np.int64), minlength=n_bins)
    counts = np.stack([births, deaths, trace[::spb], trace.reshape(n_bins, spb).sum(1)]).astype(np.int64)
    empty = np.nonzero(trace == 0)[0]
    totals = np.array([len(ts), int(np.sum(te == n_steps)), 0, empty[0] if len(empty) else -1], dtype=np.int64)
    return counts, totals


def steps(rate_bins, spb):
    return np.repeat(np.asarray(rate_bins, float), spb) / spb


def oracle_run(la, mu, spb, n_start, seed):
    from oracle import sim_oracle
    n_bins = len(la)
    ts, te, trace = sim_oracle.simulate_bd(n_start, n_bins * spb, seed, steps(la, spb), steps(mu, spb))
    return counts_from_run(ts, te, trace, n_start, n_bins, spb)


def single_run(la, mu, spb, n_start, seed):
    from literate_amd import ops
    n_bins = len(la)
    ts, te, trace = ops.simulate_bd(n_start, n_bins * spb, seed, steps(la, spb), steps(mu, spb))
    return counts_from_run(ts.cpu().numpy(), te.cpu().numpy(), trace.cpu().numpy(), n_start, n_bins, spb)


def batch(la, mu, spb, n_start, seed, capacity=None):
    from literate_amd import ops
    counts, totals = ops.simulate_bd_batch(la, mu, spb, n_start, seed, capacity=capacity)
    return counts.cpu().numpy(), totals.cpu().numpy()


def mixed_rates():
    rng = np.random.default_rng(5)
    la, mu = np.empty((12, NB)), np.empty((12, NB))
    for r in range(12):
        la[r] = rng.uniform(.05, .35, NB)
        mu[r] = rng.uniform(.02, .25, NB)
    return la, mu


CREATED_1 = [3646, 2864, 3146, 4228, 2753, 3085, 2682, 5014, 3381, 4033, 3989, 1615]


def same(what, got, want):
    ok = np.array_equal(got, want)
    print("%s: %s" % (what, "identical" if ok else "DIFFER"))
    sys.stdout.flush()
    assert ok, (what, got, want)


def case_mixed():
    la, mu = mixed_rates()
    counts, totals = batch(la, mu, SPB, 300, 1000)
    print("created", totals[:, 0].tolist(), "most alive at a bin start", int(counts[:, 2].max()))
    same("created vs the issue's figures", totals[:, 0], np.array(CREATED_1))
    for r in range(12):
        oc, ot = oracle_run(la[r], mu[r], SPB, 300, 1000 + r)
        same("replicate %d counts vs oracle" % r, counts[r], oc)
        same("replicate %d totals vs oracle" % r, totals[r], ot)
        sc, st = single_run(la[r], mu[r], SPB, 300, 1000 + r)
        same("replicate %d counts vs simulate_bd" % r, counts[r], sc)
        same("replicate %d totals vs simulate_bd" % r, totals[r], st)


def case_overflow():
    la, mu = mixed_rates()
    counts, totals = batch(la, mu, SPB, 300, 1000)
    c2, t2 = batch(la, mu, SPB, 300, 1000, capacity=4500)
    print("overflow flags", t2[:, 2].tolist())
    same("flags", t2[:, 2], np.array([0] * 7 + [1] + [0] * 4))
    assert int(t2[:, 2].sum()) == 1
    keep = np.arange(12) != 7
    same("the other eleven: counts", c2[keep], counts[keep])
    same("the other eleven: totals", t2[keep], totals[keep])


def case_beyond_lds():
    la = np.array([[.45] * 10 + [.35] * 12 + [.2] * 10] * 3)
    mu = np.full((3, 32), .1)
    counts, totals = batch(la, mu, 100, 20, 7)
    lds = header_int("LR_SIMBATCH_LDS_SLOTS")
    print("created", totals[:, 0].tolist(), "peak at a bin start", counts[:, 2].max(1).tolist(), "list positions in LDS", lds)
    assert totals[0, 0] == 67054 and counts[0, 2].max() > lds > 20      # starts inside LDS, outgrows it in mid-run
    for r in range(3):
        sc, st = single_run(la[r], mu[r], 100, 20, 7 + r)
        same("replicate %d counts vs simulate_bd" % r, counts[r], sc)
        same("replicate %d totals vs simulate_bd" % r, totals[r], st)
    oc, ot = oracle_run(la[0], mu[0], 100, 20, 7)
    same("replicate 0 counts vs oracle", counts[0], oc)
    same("replicate 0 totals vs oracle", totals[0], ot)
    # another capacity (smaller slices of the workspace behind the same LDS part) changes nothing
    c2, t2 = batch(la, mu, 100, 20, 7, capacity=70000)
    same("capacity 70000 counts", c2, counts)
    same("capacity 70000 totals", t2, totals)


def case_extinction():
    la, mu = np.full((3, NB), .02), np.full((3, NB), .6)
    counts, totals = batch(la, mu, SPB, 50, 3)
    print("first empty step", totals[:, 3].tolist())
    same("first empty step", totals[:, 3], np.array([59, 77, 46]))
    for r in range(3):
        oc, ot = oracle_run(la[r], mu[r], SPB, 50, 3 + r)
        same("replicate %d counts vs oracle" % r, counts[r], oc)
        same("replicate %d totals vs oracle" % r, totals[r], ot)
        b = int(totals[r, 3]) // SPB + 1
        assert not counts[r, :, b:].any() and totals[r, 1] == 0


def case_starts():
    la, mu = mixed_rates()
    n0 = 100 + 50 * np.arange(12)
    counts, totals = batch(la, mu, SPB, n0, 1000)
    for r in range(12):
        oc, ot = oracle_run(la[r], mu[r], SPB, int(n0[r]), 1000 + r)
        same("replicate %d counts vs oracle" % r, counts[r], oc)
        same("replicate %d totals vs oracle" % r, totals[r], ot)
    bad = n0.copy()
    bad[3], bad[9] = 0, 50001
    c2, t2 = batch(la, mu, SPB, bad, 1000, capacity=50000)
    print("overflow flags", t2[:, 2].tolist())
    same("flags", t2[:, 2], np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0]))
    keep = t2[:, 2] == 0
    same("the other ten: counts", c2[keep], counts[keep])
    same("the other ten: totals", t2[keep], totals[keep])


def case_independence():
    groups = header_int("LR_SIMBATCH_GROUPS")
    la, mu = mixed_rates()
    c1, t1 = batch(la, mu, SPB, 300, 1000)
    R = groups + 88
    rng = np.random.default_rng(11)
    la_all = np.concatenate([la, rng.uniform(.05, .2, (R - 12, NB))])
    mu_all = np.concatenate([mu, rng.uniform(.05, .2, (R - 12, NB))])
    n0 = np.concatenate([np.full(12, 300), rng.integers(1, 9, R - 12)])
    counts, totals = batch(la_all, mu_all, SPB, n0, 1000)
    print("%d replicates on at most %d workgroups" % (R, groups))
    same("first twelve: counts", counts[:12], c1)
    same("first twelve: totals", totals[:12], t1)
    assert not totals[:, 2].any()
    for r in (12, groups - 1, groups, R - 1):
        oc, ot = oracle_run(la_all[r], mu_all[r], SPB, int(n0[r]), 1000 + r)
        same("replicate %d counts vs oracle" % r, counts[r], oc)
        same("replicate %d totals vs oracle" % r, totals[r], ot)
    c2, t2 = batch(la_all, mu_all, SPB, n0, 1000)
    same("second call: counts", c2, counts)
    same("second call: totals", t2, totals)


def case_expectation():
    R = 2000
    counts, totals = batch(np.full((R, NB), .25), np.full((R, NB), .1), SPB, 100, 77)
    assert not totals[:, 2].any()
    alive = counts[:, 2].astype(float)
    want = 100 * (1 + .15 / 8) ** (8 * np.arange(NB))
    se = alive.std(0, ddof=1) / np.sqrt(R)
    z = np.zeros(NB)
    z[1:] = (alive.mean(0)[1:] - want[1:]) / se[1:]
    print("largest |z| %.3f" % np.abs(z).max(), "means", np.round(alive.mean(0), 2).tolist())
    assert np.all(alive[:, 0] == 100)
    assert np.all(np.abs(z) < 5), z


def case_arguments():
    import torch
    from literate_amd import _hip
    lib = _hip.load()
    P = _hip.ptr
    ra = torch.full((3, 5), .1, dtype=torch.float64, device="cuda")
    n0 = torch.full((3,), 10, dtype=torch.int64, device="cuda")
    cnt = torch.zeros((3, 4, 5), dtype=torch.int64, device="cuda")
    tot = torch.zeros((3, 4), dtype=torch.int64, device="cuda")
    q = lib.lr_simulate_bd_batch_workspace_bytes
    need = q(3, 5, 4, 1000)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def call(lam=ra, mu=ra, R=3, nb=5, spb=4, start=n0, cap=1000, counts=cnt, totals=tot, work=ws, nbytes=need):
        return lib.lr_simulate_bd_batch(P(lam), P(mu), R, nb, spb, P(start), cap, 1, P(counts), P(totals), P(work), nbytes, None)

    for kw in (dict(lam=None), dict(mu=None), dict(start=None), dict(counts=None), dict(totals=None), dict(work=None)):
        assert call(**kw) == _hip.LR_ERR_NULL, kw
    for kw in (dict(R=0), dict(nb=0), dict(spb=0), dict(nb=_hip.LR_MAX_BINS + 1), dict(cap=0), dict(cap=1 << 31)):
        assert call(**kw) == _hip.LR_ERR_SIZE, kw
    for a in ((0, 5, 4, 1000), (3, 0, 4, 1000), (3, 5, 0, 1000), (3, _hip.LR_MAX_BINS + 1, 4, 1000), (3, 5, 4, 0),
              (3, 5, 4, 1 << 31)):
        assert q(*a) == _hip.LR_ERR_SIZE, a
    assert q(3, 5, 4, (1 << 31) - 1) > 0
    assert call(nbytes=need - 1) == _hip.LR_ERR_WORKSPACE
    big = q(3, 5, 4, 100000)
    assert big > need and call(cap=100000) == _hip.LR_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert not cnt.any() and not tot.any()                   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert tot[:, 0].min() >= 10


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]]()
    print("case %s ok" % " ".join(sys.argv[1:]))
