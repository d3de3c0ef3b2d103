"""The restatement of the ABC simulator and driver (tests/helpers/abc_ref.py, from include/literate_hip_abc.h) and the host side
of literate_amd/abc.py, no GPU:
  1. the restated binomial against exact binomial moments;
  2. the restated count-level simulation against the per-lineage scheme it replaces;
  3. prior parsing, the refusals, and the rounds of the driver on the restated simulator."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import abc_ref as R          # noqa: E402
from literate_amd import abc              # noqa: E402

DRAWS = 20000


def draw_many(n, p, seed):
    chunks = int(R.binomial_given([n], [p], np.zeros((1, 1)))[1][0]) or 1
    u = np.random.default_rng(seed).random((DRAWS, chunks))
    x, used = R.binomial_given(np.full(DRAWS, n), np.full(DRAWS, p), u)
    assert (x >= 0).all() and (x <= n).all() and (used == chunks).all()
    return x.astype(np.float64), u


# ---- 1. the binomial ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,seed", [(5, 0.3, 1), (1000, 0.004, 2), (20000, 0.006, 3), (50, 0.9, 4), (7, 0.5, 6)])
def test_1_the_binomial_has_the_exact_mean_and_variance(n, p, seed):
    """20 000 draws: |z| of the mean < 4, the sample variance within 5 % of n p (1 - p).  (20000, 0.006) takes 8 chunks of 2666
    and one of 1338 trials, (50, 0.9) the flipped draw, (7, 0.5) the largest unflipped p.)"""
    x, _ = draw_many(n, p, seed)
    mean, var = n * p, n * p * (1.0 - p)
    z = (x.mean() - mean) / math.sqrt(var / DRAWS)
    ratio = x.var(ddof=1) / var
    print("n %d p %g: z %.3f, variance ratio %.4f" % (n, p, z, ratio))
    assert abs(z) < 4.0
    assert abs(ratio - 1.0) < 0.05


def test_1_the_binomial_at_a_tiny_probability():
    """(3, 1e-9): the mean is held to |z| < 4 as the others.  The variance ratio is not estimable here by ANY sampler, an exact one
    included: 20 000 draws hold a non-zero one with probability 6e-5, so the sample variance is 0 (ratio 0) or at least 5e-5
    (ratio 16 000).  In its place: every uniform below the first cdf step (1 - p)^3 gives 0 - all 20 000 do - and the uniforms
    on either side of the first two steps give 0 | 1 and 1 | 3 (the steps to 2 and 3 are 3e-18 and 1e-27 wide, far below the
    spacing of doubles near 1: a uniform above the second step is above them all)."""
    n, p = 3, 1e-9
    x, u = draw_many(n, p, 5)
    z = (x.mean() - n * p) / math.sqrt(n * p * (1.0 - p) / DRAWS)
    print("n 3 p 1e-9: z %.4f" % z)
    assert abs(z) < 4.0
    f0 = (1.0 - p) * (1.0 - p) * (1.0 - p)
    assert u.max() < f0 and (x == 0).all()
    f1 = f0 * ((p / (1.0 - p)) * (3.0 / 1.0))
    c1 = f0 + f1
    # (the second step is where fl(u - f0) reaches f1, an ulp or two of 1 beside fl(f0 + f1): 8 ulp to either side)
    edges = np.array([[np.nextafter(f0, 0.0)], [f0], [c1 - 2.0 ** -50], [c1 + 2.0 ** -50]])
    got, used = R.binomial_given(np.full(4, n), np.full(4, p), edges)
    assert got.tolist() == [0, 1, 1, 3] and used.tolist() == [1, 1, 1, 1]


def test_1_the_edges_of_the_binomial():
    u = np.array([[0.0, 0.5], [1.0 - 2.0 ** -53, 0.5]])
    for n, p, want in ((0, 0.3, [0, 0]), (4, 0.0, [0, 0]), (4, 1.0, [4, 4]), (4, -1.0, [0, 0]), (4, 2.0, [4, 4])):
        x, used = R.binomial_given([n, n], [p, p], u)
        assert x.tolist() == want and used.tolist() == [0, 0], (n, p)
    x, used = R.binomial_given([1, 1, -1, (1 << 24) + 1, 5, 100], [0.25, 0.25, 0.5, 0.5, np.nan, 0.5], np.array([[0.7499, 0.0], [0.75, 0.0]] * 3))
    assert x.tolist() == [0, 1, -1, -1, -1, -1] and used.tolist() == [1, 1, 0, 0, 0, 4]          # (100 at 0.5: chunks of 32, 4 > n_u)
    # a uniform next to 1 stops at the search cap, not at m
    x, used = R.binomial_given([250], [0.05], [[1.0 - 2.0 ** -53]])
    assert x.tolist() == [R.SEARCH_CAP] and used.tolist() == [1]


# ---- 2. counts against lineages ---------------------------------------------------------------------------------------------------
def test_2_the_count_level_simulation_matches_the_per_lineage_scheme():
    """8 bins x 20 steps from 5 lineages under theta = (0.5, 0.2, 30, 400, 0.7, 0.2), 1500 runs each: every per-bin mean of the four
    counts within |z| < 4 (Welch).  A run that dies out is zero from the bin where it stopped, in both."""
    nb, spb, runs = 8, 20, 1500
    theta = np.tile([0.5, 0.2, 30.0, 400.0, 0.7, 0.2], (runs, 1))
    tab = np.zeros((3, nb))
    a = R.simulate(11, np.arange(runs), theta, 5, nb, spb, 1 << 20, tab, tab)
    b = R.simulate(11, np.arange(runs), theta, 5, nb, spb, 1 << 20, tab, tab, per_lineage_rng=np.random.default_rng(12))
    assert not ((a[1] | b[1]) & ~R.FLAG_EXTINCT).any() and (a[0][a[1] == 0] == 0.0).all()
    ca, cb = a[2].astype(np.float64), b[2].astype(np.float64)
    se = np.sqrt(ca.var(0, ddof=1) / runs + cb.var(0, ddof=1) / runs)
    z = (ca.mean(0) - cb.mean(0)) / np.where(se > 0, se, 1.0)
    print("extinct %d | %d; max |z| %.3f" % ((a[1] != 0).sum(), (b[1] != 0).sum(), np.abs(z).max()))
    assert (ca[a[1] == 0, 2, 0] == 5).all() and (cb[b[1] == 0, 2, 0] == 5).all()
    assert np.abs(z).max() < 4.0
    assert ca[:, 2, -1].mean() > 20          # (the niche grew: K0 = 30 alone would hold the diversity near 13)


def test_2_one_simulation_is_the_batch_row():
    theta = np.array([[0.5, 0.2, 30.0, 400.0, 0.7, 0.2], [0.9, 0.1, 10.0, 50.0, 0.0, 0.0], [0.4, 0.3, 8.0, 20.0, 0.1, 0.9]])
    obs = np.array([[0.4, 0.5, 0.3], [0.2, 0.1, 0.2], [5.0, 6.0, 7.0]])
    w = R.mean_relative_weights(obs, rows=(0, 1, 2))
    dist, flags, counts, K = R.simulate(3 << 33 | 5, [7, 1 << 31, 9], theta, [5, 3, 4], 3, 4, 64, obs, w)
    for i, sid in enumerate([7, 1 << 31, 9]):
        one = R.simulate_one(3 << 33 | 5, sid, theta[i], [5, 3, 4][i], 3, 4, 64, obs, w)
        assert one[0] == dist[i] and one[1] == flags[i] and np.array_equal(one[2], counts[i]) and one[3] == K[i]


# ---- 3. the driver ----------------------------------------------------------------------------------------------------------------
def test_3_priors_are_parsed_and_refused(tmp_path):
    base = abc.default_priors(5, 80, "niche")
    assert base[2] == ("uniform", 5.0, 80.0) and base[3] == ("loguniform", 80.0, 1600.0) and base[4] == ("uniform", 0.0, 1.0)
    assert abc.default_priors(5, 80, "fixed")[4:] == [("fixed", 0.0, 0.0)] * 2
    path = tmp_path / "priors.tsv"
    path.write_text("param\tdist\ta\tb\n# a comment\nl0\tuniform\t0.1\t2\nKmax\tfixed\t300\ng\tloguniform\t0.01\t1\n")
    pr = abc.read_priors(str(path), base)
    assert pr[0] == ("uniform", 0.1, 2.0) and pr[3] == ("fixed", 300.0, 300.0) and pr[4] == ("loguniform", 0.01, 1.0) and pr[1] == base[1]
    assert np.allclose(abc.prior_mean(pr)[[0, 3, 4]], [1.05, 300.0, 0.99 / math.log(100.0)])
    for text, why in (("lambda\tuniform\t0\t1\n", "unknown parameter 'lambda'"), ("l0\tuniform\t2\t2\n", r"support \[2.0, 2.0\] is empty"),
                      ("l0\tuniform\t3\t1\n", "is empty"), ("l0\tloguniform\t0\t1\n", "positive lower bound"),
                      ("l0\tgamma\t1\t1\n", "unknown distribution 'gamma'"), ("l0\tuniform\t1\n", "expected `param dist a b`")):
        path.write_text(text)
        with pytest.raises(ValueError, match=why):
            abc.read_priors(str(path), base)
    th = abc.prior_transform(pr, np.random.default_rng(0).random((500, 6)))
    assert abc.in_support(pr, th).all() and (th[:, 3] == 300.0).all()
    assert not abc.in_support(pr, th + np.array([0, 0, 0, 0, 5.0, 0])).any()
    # the density integrates to one over the support of a free pair (midpoint rule on a 400 x 400 grid)
    two = [("uniform", 0.5, 2.5), ("loguniform", 0.1, 3.0)] + [("fixed", 1.0, 1.0)] * 4
    g0, g1 = (np.arange(400) + 0.5) / 400 * 2.0 + 0.5, (np.arange(400) + 0.5) / 400 * 2.9 + 0.1
    grid = np.ones((160000, 6))
    grid[:, 0], grid[:, 1] = np.repeat(g0, 400), np.tile(g1, 400)
    assert abs(np.exp(abc.log_prior(two, grid)).sum() * (2.0 / 400) * (2.9 / 400) - 1.0) < 1e-3


def test_3_too_few_bins_and_no_finite_distance_are_refused():
    sp, ex, DT = np.array([6, 2, 3]), np.array([0, 1, 1]), np.array([3.0, 6.5, 8.0])
    with pytest.raises(ValueError, match="1 bin after the start bin 2: at least 2 are needed"):
        abc.Observed(sp, ex, DT, start_bin=2)
    ob = abc.Observed(sp, ex, DT)
    assert (ob.b0, ob.n_bins, ob.n_start, ob.max_div) == (1, 2, 6, 9) and ob.default_max_living() == 144
    assert np.array_equal(ob.obs, [[2 / 6.5, 3 / 8.0], [1 / 6.5, 1 / 8.0], [0.0, 0.0]]) and (ob.weight[2] == 0).all()
    assert np.allclose((ob.weight * ob.obs).sum(), 1.0)
    assert np.count_nonzero(abc.Observed(sp, ex, DT, stats="rates+div").weight) == 6
    with pytest.raises(ValueError, match="no simulation of round 0 has a finite distance"):
        abc.fit(lambda th, ids: (np.full(len(th), np.inf), np.full(len(th), 2, dtype=np.int32)), abc.default_priors(5, 80), 64, 0.1, 2, 1)


NB, SPB, N0, MAXL, SEED = 6, 8, 20, 4096, 2024
TRUE = np.array([0.9, 0.2, 60.0, 400.0, 0.8, 0.3])


def driver_case():
    """the data: simulation 0 under TRUE (its own seed); scored on the rates, the mean relative deviation"""
    tab = np.zeros((3, NB))
    _, flags, counts, _ = R.simulate(77, [0], [TRUE], N0, NB, SPB, MAXL, tab, tab)
    assert flags[0] == 0
    obs = R.statistics(counts[0], SPB)
    weight = R.mean_relative_weights(obs)
    max_div = int(max(counts[0, 2].max(), counts[0, 2, -1] + counts[0, 0, -1] - counts[0, 1, -1]))
    priors = abc.default_priors(N0, max_div, "niche")

    def simulate(theta, ids):
        return R.simulate(SEED, ids, theta, N0, NB, SPB, MAXL, obs, weight)[:2]
    return obs, weight, priors, simulate


@pytest.fixture(scope="module")
def driver_run():
    obs, weight, priors, simulate = driver_case()
    return priors, simulate, R.run_rounds(simulate, priors, 4096, 0.05, 3, SEED)


def test_3_the_rounds_of_the_driver(driver_run):
    priors, simulate, run = driver_run
    assert run["stopped"] is None and len(run["eps"]) == 3 and run["kept"] == [205] * 3
    assert abs(run["weights"].sum() - 1.0) < 1e-12 and (run["weights"] > 0).all()
    assert all(b <= a for a, b in zip(run["eps"], run["eps"][1:])), run["eps"]
    assert (run["dist"] <= run["eps"][-1]).all() and (np.diff(run["dist"]) >= 0).all()
    assert (run["ids"] >= 2 * 4096).all() and (run["ids"] < 3 * 4096).all() and len(set(run["ids"])) == len(run["ids"])
    again = simulate(run["theta"], run["ids"])[0]
    assert np.array_equal(again, run["dist"])          # the id rule: the kept ids alone give the kept distances
    post, prior = (run["weights"][:, None] * run["theta"]).sum(0), abc.prior_mean(priors)
    print("eps", run["eps"], "posterior means", post, "prior means", prior)
    for d in (0, 1):
        assert abs(post[d] - TRUE[d]) < abs(prior[d] - TRUE[d]), (abc.PARAMS[d], post[d], prior[d])


def test_3_the_module_runs_the_restated_rounds(driver_run):
    """literate_amd.abc.fit on the restated simulator, its weights by the restated sum: the same population"""
    priors, simulate, run = driver_run
    res = abc.fit(simulate, priors, 4096, 0.05, 3, SEED, log_weights=lambda new, lp, old, w, var2, moved: R.log_weights(new, priors, old, w, var2, moved))
    assert np.array_equal(res.ids, run["ids"]) and np.array_equal(res.dist, run["dist"]) and np.array_equal(res.theta, run["theta"])
    assert np.array_equal(res.weights, run["weights"]) and [r["eps"] for r in res.rounds] == run["eps"]
    assert [r["kept"] for r in res.rounds] == run["kept"] and res.rounds[0]["in_support"] == 4096 and res.rounds[1]["in_support"] < 4096
    assert abs(res.rounds[-1]["ess"] - 1.0 / np.sum(run["weights"] ** 2)) < 1e-9 and res.rounds[0]["ess"] == pytest.approx(205.0)
    text = abc.params_table(res).splitlines()
    assert text[0].split("\t") == ["param", "prior_mean", "mean", "q2.5", "q50", "q97.5", "fixed"] and len(text) == 7
    q = [float(v) for v in text[1].split("\t")[3:6]]
    assert q[0] <= q[1] <= q[2] and res.theta[:, 0].min() <= q[0] and q[2] <= res.theta[:, 0].max()
    assert abc.rounds_table(res).splitlines()[0].split("\t") == abc.ROUND_COLS


def test_3_a_round_that_keeps_one_particle_stops():
    priors = abc.default_priors(5, 80, "fixed")

    def simulate(theta, ids):          # round 0: distances 1, 2, 3, ...; afterwards one finite distance below eps
        d = np.arange(1.0, len(ids) + 1.0) if ids[0] == 0 else np.where(np.arange(len(ids)) == 3, 0.5, np.inf)
        return d, np.zeros(len(ids), dtype=np.int32)
    res = abc.fit(simulate, priors, 100, 0.1, 3, 4, log_weights=None)
    assert res.stopped == 1 and len(res.rounds) == 2 and res.rounds[1]["kept"] == 1 and res.dist.tolist() == list(np.arange(1.0, 11.0))
    assert "round 1 kept fewer than 2" in abc.rounds_table(res)
