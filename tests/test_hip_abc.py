"""The count-level ABC simulator on the device (include/literate_hip_abc.h, csrc/lr_abc.hip, literate_amd/abc.py) against
tests/helpers/abc_ref.py:
  1. lr_abc_binomial: equal integers and equal uniforms consumed, at the chunk edges, the cdf steps and the search cap;
  2. lr_abc_simulate bit for bit on counts, flags, k_end and dist, at the wave and block edges and on both table paths;
  3. identity: a simulation is its (seed, id), wherever it stands;   4. pinned on the reference's own simulator;
  5. the buffer and stream contracts and the refusals;   6. the driver end to end.
max_living <= 4096 throughout."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import abc_ref as R          # noqa: E402

pytestmark = pytest.mark.gpu

TOP = 1.0 - 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")


def host(*ts):
    return [t.cpu().numpy() for t in ts]


# ---- 1. the binomial ------------------------------------------------------------------------------------------------------------
def binomial_cases():
    """rows (n, p, u [N_U]): for every (n, p) the first chunk's uniform at 0, next to 1, on either side of the first two cdf
    steps and at a random place; the later chunks random"""
    n_u = 12
    rng = np.random.default_rng(5)
    pairs = [(65, 0.25), (64, 0.25), (63, 0.25),          # the chunk length floor(16 / p) = 64 is n - 1, n, n + 1
             (54, 0.3), (53, 0.3), (52, 0.3),            # ... 53
             (10, 0.0), (10, 1.0), (10, np.nextafter(0.5, 1.0)), (10, np.nextafter(0.5, 0.0)), (10, 0.5), (300, 0.9),
             (4096, 1e-12), (0, 0.3), (1, 0.3), (1, 0.7), (250, 0.05), (4096, 0.05), (4096, 0.004)]
    rows = []
    for n, p in pairs:
        first = [0.0, TOP, rng.random()]
        if n > 0 and 0.0 < p < 1.0:
            q = 1.0 - p if p > 0.5 else p
            m = np.array([min(n, int(R.chunk_len(np.array([n]), np.array([q]))[0]))])
            f0 = float(R.powi(np.array([1.0 - q]), m)[0])
            c1 = f0 + f0 * ((q / (1.0 - q)) * (float(m[0]) / 1.0))
            first += [np.nextafter(f0, 0.0), f0, c1 - 2.0 ** -50, c1 + 2.0 ** -50]
        for u0 in first:
            rows.append((n, p, np.concatenate([[u0], rng.random(n_u - 1)])))
    for _ in range(1500):          # and anywhere
        rows.append((int(rng.integers(0, 4097)), float(np.exp(rng.uniform(np.log(1e-4), 0.0))), rng.random(n_u)))
    rows += [(-1, 0.5, rng.random(n_u)), ((1 << 24) + 1, 0.5, rng.random(n_u)), (5, np.nan, rng.random(n_u)),
             (4096, 0.5, rng.random(n_u))]          # (the last: 128 chunks, more than n_u)
    return (np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows]), np.stack([r[2] for r in rows]))


def test_1_the_binomial_is_the_restatement():
    from literate_amd import ops
    n, p, u = binomial_cases()
    x, used = host(*ops.abc_binomial(n, p, u))
    rx, rused = R.binomial_given(n, p, u)
    assert np.array_equal(x, rx) and np.array_equal(used, rused), np.nonzero((x != rx) | (used != rused))[0][:10]
    assert x[-1] == -1 and used[-1] == 128 and (x[-4:-1] == -1).all() and (used[-4:-1] == 0).all()
    cap = (n == 250) & (u[:, 0] == TOP)
    assert cap.sum() == 1 and x[cap][0] == R.SEARCH_CAP          # the search cap, below m = 250
    assert used.max() > 8 and (x[(p == 1.0)] == n[p == 1.0]).all() and (x[p == 0.0] == 0).all()


# ---- 2. the simulation ------------------------------------------------------------------------------------------------------------
MAXL = 4096


def sim_rows(n_sims, spb, seed, only=None):
    """theta [n_sims, 6] and n_start [n_sims], cycling through the kinds of row the header tells apart (only: through these)"""
    s = float(spb)
    nan, inf = np.nan, np.inf
    kinds = [((0.5, 0.2, 30.0, 400.0, 0.7, 0.2), 5),                     # the niche grows
             ((3.5 * s, 0.1, 1e6, 1e6, 0.0, 0.0), 2),                    # lt >= 1: everybody spawns, then past max_living
             ((0.6 * s, 0.7 * s, 1e6, 1e6, 0.0, 0.0), 40),               # lt + mt > 1, lt < 1
             ((0.5, -0.5, 10.0, 10.0, 0.0, 0.0), 10),                    # lt = 0: n >= K
             ((0.5, 0.2, 200.0, 200.0, 0.0, 0.0), 150),                  # g = h = 0, the fixed niche
             ((0.01, 0.9 * s, 30.0, 30.0, 0.1, 0.1), 1),                 # dies out inside a bin
             ((0.9 * s, 0.0, 1e5, 1e5, 0.0, 0.0), 4000),                 # past max_living inside a bin
             ((0.5, 0.2, 30.0, 400.0, 0.7, 0.2), 0), ((0.5, 0.2, 30.0, 400.0, 0.7, 0.2), MAXL + 1),          # refused
             ((0.5, nan, 30.0, 400.0, 0.7, 0.2), 5), ((0.5, 0.2, 30.0, inf, 0.7, 0.2), 5), ((0.5, 0.2, 30.0, 0.0, 0.7, 0.2), 5),
             ((0.3 * s, 0.3 * s, 1e6, 1e6, 0.0, 0.0), 3000),             # many chunks per draw
             ((0.7 * s, 0.25 * s, 1e6, 1e6, 0.0, 0.0), 100),             # pb > 0.5: the flipped draw
             ((0.5, 0.2, 1.0, 5000.0, 2.0, 0.5), 30)]                    # K0 below n_start: the clamp
    kinds = kinds if only is None else [kinds[k] for k in only]
    rng = np.random.default_rng(seed)
    theta = np.array([kinds[i % len(kinds)][0] for i in range(n_sims)])
    jitter = np.where(np.isfinite(theta) & (np.arange(n_sims)[:, None] >= len(kinds)), rng.uniform(0.9, 1.1, theta.shape), 1.0)
    return theta * jitter, np.array([kinds[i % len(kinds)][1] for i in range(n_sims)], dtype=np.int32)


def tables(n_bins, pattern, seed):
    """obs and weight; pattern 0: every entry counts, 1: the death row counts for nothing, 2: the first bin is skipped.  An
    entry that does not count holds a NaN: it is not evaluated."""
    rng = np.random.default_rng(seed)
    obs = np.stack([rng.uniform(0.1, 0.8, n_bins), rng.uniform(0.05, 0.5, n_bins), rng.uniform(5.0, 300.0, n_bins)])
    counted = np.ones((3, n_bins), dtype=bool)
    if pattern == 1:
        counted[1] = False
    if pattern == 2:
        counted[:, 0] = False
    weight = np.where(counted, 1.0 / (obs * max(counted.sum(), 1)), 0.0)
    return np.where(counted, obs, np.nan), weight


def check_parity(n_sims, n_bins, spb, pattern, seed=9, id0=1000, only=None):
    from literate_amd import ops
    theta, n0 = sim_rows(n_sims, spb, seed, only)
    obs, weight = tables(n_bins, pattern, seed)
    got = ops.abc_simulate(theta, n0, obs, weight, spb, MAXL, seed, id0=id0, counts=True, k_end=True)
    dist, flags, counts, k_end = host(got.dist, got.flags, got.counts, got.k_end)
    rd, rf, rc, rk = R.simulate(seed, id0 + np.arange(n_sims), theta, n0, n_bins, spb, MAXL, obs, weight)
    assert np.array_equal(flags, rf), np.nonzero(flags != rf)[0][:10]
    assert np.array_equal(counts, rc), np.nonzero((counts != rc).any((1, 2)))[0][:10]
    assert np.array_equal(k_end, rk), np.nonzero(k_end != rk)[0][:10]
    assert np.array_equal(dist, rd), np.nonzero(dist != rd)[0][:10]
    assert not np.isnan(dist).any() and (np.isinf(dist) == (flags != 0)).all()
    return flags


@pytest.mark.parametrize("spb", [1, 3])
@pytest.mark.parametrize("n_bins", [1, 2, 5])
@pytest.mark.parametrize("n_sims", [1, 63, 64, 65, 257])
def test_2_bit_parity(n_sims, n_bins, spb):
    flags = check_parity(n_sims, n_bins, spb, pattern=(n_sims + n_bins + spb) % 3)
    if n_sims >= 63:
        assert (flags[7:12] == 4).all() and flags[1] in (0, 1) and flags[0] == 0


def test_2_every_kind_of_stop_is_met():
    """at 5 bins x 3 steps: the rows that overflow, die out and are refused do, the others do not"""
    flags = check_parity(15, 5, 3, pattern=0)
    assert flags.tolist() == [0, 1, 0, 0, 0, 2, 1, 4, 4, 4, 4, 4, 0, 1, 0]


@pytest.mark.parametrize("over", [0, 1])
def test_2_the_tables_at_and_beyond_lds(over):
    """n_bins above LR_ABC_LDS_BINS: obs and weight are read from HBM; at it: the largest tables LDS holds.  (The rows of small
    populations: the restatement walks a thousand steps.)"""
    from literate_amd import _hip
    flags = check_parity(70, _hip.LR_ABC_LDS_BINS + over, 1, pattern=2 - over, only=[0, 3, 4, 5, 7, 9])
    assert flags[:6].tolist() == [0, 0, 0, 2, 4, 4]


# ---- 3. identity ------------------------------------------------------------------------------------------------------------------
def test_3_a_simulation_is_its_seed_and_id():
    import torch
    from literate_amd import ops
    n_sims, nb, spb, seed = 300, 4, 3, (5 << 32) | 17
    theta, n0 = sim_rows(n_sims, spb, 3)
    obs, weight = tables(nb, 0, 3)
    base = ops.abc_simulate(theta, n0, obs, weight, spb, MAXL, seed, id0=50, counts=True, k_end=True)
    perm = np.random.default_rng(1).permutation(n_sims)
    moved = ops.abc_simulate(theta[perm], n0[perm], obs, weight, spb, MAXL, seed, sim_id=50 + perm, counts=True, k_end=True)
    at = torch.as_tensor(perm, device="cuda")
    for a, b in zip(base, moved):
        assert torch.equal(a[at], b)
    some = perm[:37]
    part = ops.abc_simulate(theta[some], n0[some], obs, weight, spb, MAXL, seed, sim_id=50 + some)
    assert part.counts is None and part.k_end is None
    assert torch.equal(part.dist, base.dist[at[:37]]) and torch.equal(part.flags, base.flags[at[:37]])
    other = ops.abc_simulate(theta, n0, obs, weight, spb, MAXL, seed + 1, id0=50)
    high = ops.abc_simulate(theta, n0, obs, weight, spb, MAXL, seed + (1 << 32), id0=50)          # the high word counts too
    fin = torch.isfinite(base.dist) & torch.isfinite(other.dist) & torch.isfinite(high.dist)
    assert int(fin.sum()) > 100 and int((base.dist[fin] != other.dist[fin]).sum()) > 90 and int((base.dist[fin] != high.dist[fin]).sum()) > 90
    ids = np.array([-1, 1 << 32, (1 << 32) - 1, 0])
    edge = ops.abc_simulate(theta[:4] * 0 + theta[0], 5, obs, weight, spb, MAXL, seed, sim_id=ids)
    assert edge.flags.tolist() == [4, 4, 0, 0]


# ---- 4. pinned on the reference ---------------------------------------------------------------------------------------------------
def test_4_the_reference_simulators_diversity():
    """tests/golden/abc_sim.npz: mean and variance of the living count at the start of each bin over 4000 passes of the
    Simulator class of simulateRateABC.v2.py (fixed niche K 200, l0 0.5, m0 0.2, 5 founders, 4 bins x scale 100), made by
    tests/golden/make_abc_sim_golden.py.  4000 device simulations of the same settings: the means at the start of bins 1 - 3 within
    |z| < 4 (Welch).  The script does not register a death at step 0 (te = 0 means alive), which moves its mean up by about 0.2
    %, a sixth of the standard error.  A device run that died out is zero from the bin where it stopped; the script records what
    lived at the start of that bin, which the counts of the bin before give back."""
    from literate_amd import ops
    g = np.load(os.path.join(ROOT, "tests", "golden", "abc_sim.npz"))
    l0, m0, K, founders, nb, scale = g["settings"]
    nb, scale, runs = int(nb), int(scale), int(g["runs"])
    theta = np.tile([l0, m0, K, K, 0.0, 0.0], (runs, 1))
    tab = np.zeros((3, nb))
    res = ops.abc_simulate(theta, int(founders), tab, tab, scale, MAXL, 4, counts=True)
    flags, counts = host(res.flags, res.counts)
    assert not (flags & ~2).any()
    div = golden_diversity(flags, counts)
    z = (div.mean(0)[1:] - g["mean"][1:]) / np.sqrt(div.var(0, ddof=1)[1:] / runs + g["var"][1:] / runs)
    print("device mean", div.mean(0), "reference mean", g["mean"], "z of bins 1 - 3", z)
    assert (div[:, 0] == founders).all() and g["mean"][0] == founders
    assert np.abs(z).max() < 4.0


def golden_diversity(flags, counts):
    div = counts[:, 2].astype(np.float64)
    for i in np.nonzero(flags)[0]:
        b = int(np.nonzero(counts[i, 3] == 0)[0][0])          # the bin in which it stopped
        div[i, b] = div[i, 0] if b == 0 else counts[i, 2, b - 1] + counts[i, 0, b - 1] - counts[i, 1, b - 1]
    return div


# ---- 5. contracts -----------------------------------------------------------------------------------------------------------------
def test_5_the_outputs_do_not_depend_on_what_the_buffers_held():
    import torch
    from helpers.abi_cases import contract
    from literate_amd import ops
    theta, n0 = sim_rows(130, 3, 2)
    obs, weight = tables(5, 2, 2)
    for counts in (True, False):
        out = contract(ops, torch, lambda: ops.abc_simulate(theta, n0, obs, weight, 3, MAXL, 8, id0=3, counts=counts, k_end=counts),
                       label="abc_simulate")
        assert (out.counts is None) == (not counts)
    n, p, u = binomial_cases()
    contract(ops, torch, lambda: ops.abc_binomial(n, p, u), label="abc_binomial")


def test_5_the_stream_contract_on_a_busy_side_stream():
    """both entry points take the stream in their descriptor: the library handed to TorchRuntime is an adapter with the stream
    last, as tests/test_hip_score.py does for lr_rtt_score"""
    import torch
    from helpers import stream_cases as S
    from literate_amd import _hip, ops
    lib = _hip.load()

    def simulate(prob, stream):
        prob.stream = stream
        return lib.lr_abc_simulate(C.byref(prob))

    def binomial(prob, stream):
        prob.stream = stream
        return lib.lr_abc_binomial(C.byref(prob))
    adapters = types.SimpleNamespace(lr_abc_simulate=simulate, lr_abc_binomial=binomial)
    rt = S.TorchRuntime(library=(adapters, ["lr_abc_simulate", "lr_abc_binomial"]))
    N, nb, spb = 200, 4, 3

    def make(seed):
        theta, n0 = sim_rows(N, spb, seed)
        obs, weight = tables(nb, 0, seed)
        return theta, n0, obs, weight

    def call(theta, n0, obs, weight):
        out = dict(dist=ops.alloc_output(N, torch.float64, "cuda"), flags=ops.alloc_output(N, torch.int32, "cuda"),
                   counts=ops.alloc_output((N, 4, nb), torch.int64, "cuda"), k_end=ops.alloc_output(N, torch.float64, "cuda"))
        prob = _hip.AbcProblem(_hip.ptr(theta), _hip.ptr(n0), None, _hip.ptr(obs), _hip.ptr(weight), _hip.ptr(out["dist"]),
                               _hip.ptr(out["flags"]), _hip.ptr(out["counts"]), _hip.ptr(out["k_end"]), N, 7, nb, spb, MAXL, 0, 21, None)
        assert adapters.lr_abc_simulate(prob, rt.current_stream_arg()) == 0
        return out
    a_in, b_in = [S.dev(torch, x) for x in make(60)], [S.dev(torch, x) for x in make(61)]
    bufs = [torch.empty_like(x) for x in a_in]
    want, table = S.ordered(rt, lambda: call(*bufs), a_in, b_in, bufs, "abc_simulate")
    assert table["lr_abc_simulate"]["calls"] == 1
    ref = ops.abc_simulate(a_in[0], a_in[1], a_in[2], a_in[3], spb, MAXL, 21, id0=7, counts=True)
    assert np.array_equal(np.frombuffer(want["dist"]), ref.dist.cpu().numpy())
    assert np.array_equal(np.frombuffer(want["counts"], dtype=np.int64).reshape(N, 4, nb), ref.counts.cpu().numpy())

    n, p, u = binomial_cases()
    M, n_u = len(n), u.shape[1]

    def call_b(n_, p_, u_):
        out = dict(x=ops.alloc_output(M, torch.int32, "cuda"), used=ops.alloc_output(M, torch.int32, "cuda"))
        prob = _hip.AbcBinomialProblem(_hip.ptr(n_), _hip.ptr(p_), _hip.ptr(u_), _hip.ptr(out["x"]), _hip.ptr(out["used"]), M, n_u, 0, None)
        assert adapters.lr_abc_binomial(prob, rt.current_stream_arg()) == 0
        return out
    a_in = [S.dev(torch, x) for x in (n, p, u)]
    b_in = [S.dev(torch, x) for x in (n[::-1].copy(), p[::-1].copy(), u[::-1].copy())]
    bufs = [torch.empty_like(x) for x in a_in]
    want, table = S.ordered(rt, lambda: call_b(*bufs), a_in, b_in, bufs, "abc_binomial")
    assert table["lr_abc_binomial"]["calls"] == 1
    assert np.array_equal(np.frombuffer(want["x"], dtype=np.int32), R.binomial_given(n, p, u)[0])


def test_5_refusals_leave_every_output_byte_as_it_was():
    import torch
    from helpers.abi_cases import refuses
    from literate_amd import _hip, ops
    theta, n0 = sim_rows(20, 3, 2)
    obs, weight = tables(5, 0, 2)
    wide = np.ones((3, _hip.LR_MAX_BINS + 1))
    for what, call in (
            ("no step", lambda: ops.abc_simulate(theta, n0, obs, weight, 0, MAXL, 1, counts=True, k_end=True)),
            ("max_living 0", lambda: ops.abc_simulate(theta, n0, obs, weight, 3, 0, 1, counts=True)),
            ("max_living 2^24 + 1", lambda: ops.abc_simulate(theta, n0, obs, weight, 3, (1 << 24) + 1, 1)),
            ("2^31 steps", lambda: ops.abc_simulate(theta, n0, obs, weight, (1 << 31) // 5 + 1, MAXL, 1, k_end=True)),
            ("LR_MAX_BINS + 1 bins", lambda: ops.abc_simulate(theta, n0, wide, wide, 1, MAXL, 1, counts=True)),
            ("a negative id0", lambda: ops.abc_simulate(theta, n0, obs, weight, 3, MAXL, 1, id0=-1)),
            ("ids past 2^32", lambda: ops.abc_simulate(theta, n0, obs, weight, 3, MAXL, 1, id0=(1 << 32) - 19))):
        refuses(ops, torch, call, "LR_ERR_SIZE", label=what, entry="lr_abc_simulate")
    ok = ops.abc_simulate(theta, n0, obs, weight, 3, MAXL, 1, id0=(1 << 32) - 20)          # the last id there is is served
    assert ok.flags.tolist() == ops.abc_simulate(theta, n0, obs, weight, 3, MAXL, 1, sim_id=(1 << 32) - 20 + np.arange(20)).flags.tolist()
    with pytest.raises(ValueError, match="theta must be"):
        ops.abc_simulate(theta[:, :5], n0, obs, weight, 3, MAXL, 1)
    with pytest.raises(ValueError, match="obs and weight"):
        ops.abc_simulate(theta, n0, obs, weight[:2], 3, MAXL, 1)


# ---- 6. the driver ----------------------------------------------------------------------------------------------------------------
NB, SPB, N0, SEED = 6, 8, 20, 2024
TRUE = np.array([0.9, 0.2, 60.0, 400.0, 0.8, 0.3])


def test_6_the_driver_end_to_end(tmp_path):
    """the host test's shape (6 bins x 8 steps, 4096 simulations, keep 0.05, 3 rounds, data simulated under TRUE): the kept ids,
    distances and eps of the device run are the restated driver's exactly, its log-weights within 1e-11 (a fixed-order sum of
    at most 4096 positive terms, each a few ulp off); the four files are written and the re-run of the kept ids alone gave the
    kept distances bit for bit (run() raises otherwise; checked again here from the npz)."""
    from literate_amd import abc, ops
    tab = np.zeros((3, NB))
    _, flags, counts, _ = R.simulate(77, [0], [TRUE], N0, NB, SPB, MAXL, tab, tab)
    assert flags[0] == 0
    c = counts[0]
    # create_bins' statistics of such a data set: a bin in front in which the founders appear, then the simulated bins
    n_spec, n_exti = np.concatenate([[N0], c[0]]), np.concatenate([[0], c[1]])
    DT = np.concatenate([[N0 / 2.0], c[3] / float(SPB)])
    stem = str(tmp_path / "run")
    observed, res, sims = abc.run(n_spec, n_exti, DT, "niche", None, 4096, 0.05, 3, SPB, None, MAXL, "rates", SEED, out=stem)
    assert (observed.b0, observed.n_bins, observed.n_start) == (1, NB, N0)
    assert np.array_equal(observed.obs[:2], R.statistics(c, SPB)[:2]) and np.array_equal(observed.weight, R.mean_relative_weights(R.statistics(c, SPB)))
    ref = R.run_rounds(lambda th, ids: R.simulate(SEED, ids, th, N0, NB, SPB, MAXL, observed.obs, observed.weight)[:2],
                       abc.default_priors(N0, observed.max_div), 4096, 0.05, 3, SEED)
    assert res.stopped is None and ref["stopped"] is None
    assert np.array_equal(res.ids, ref["ids"]) and np.array_equal(res.dist, ref["dist"]) and np.array_equal(res.theta, ref["theta"])
    assert [r["eps"] for r in res.rounds] == ref["eps"] and [r["kept"] for r in res.rounds] == ref["kept"]
    err = np.abs(np.log(res.weights) - ref["log_weights"]).max()
    print("log-weights off by at most", err)
    assert err < 1e-11 and abs(res.weights.sum() - 1.0) < 1e-12
    for suffix in ("_ABC.tsv", "_ABC_rounds.tsv", "_ABC_fit.tsv", "_ABC.npz"):
        assert os.path.getsize(stem + suffix) > 0, suffix
    z = np.load(stem + "_ABC.npz")
    again = ops.abc_simulate(z["theta"], N0, observed.obs, observed.weight, SPB, MAXL, SEED, sim_id=z["ids"], counts=True)
    assert np.array_equal(again.dist.cpu().numpy(), z["dist"]) and np.array_equal(z["dist"], ref["dist"])
    assert np.array_equal(abc.fit_stats(again.counts.cpu().numpy(), SPB), z["sims"]) and z["sims"].shape == (len(ref["ids"]), 3, NB)
    fit = open(stem + "_ABC_fit.tsv").read().splitlines()
    assert len(fit) == 1 + 3 * NB and fit[1].split("\t")[:2] == ["birth_rate", "1"]
    post = (res.weights[:, None] * res.theta).sum(0)
    prior = abc.prior_mean(res.priors)
    assert abs(post[0] - TRUE[0]) < abs(prior[0] - TRUE[0]) and abs(post[1] - TRUE[1]) < abs(prior[1] - TRUE[1])
