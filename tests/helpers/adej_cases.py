"""The case tables of the joint sampler of (death-rate skyline, Weibull shape), shared by tests/test_adej_host.py (the
restatement against what is known exactly) and tests/test_hip_adej.py, whose GPU cases run here, each in a child process of
its own (under the test's time limit):

    python tests/helpers/adej_cases.py CASE [ARGS...]

A case prints its figures, asserts, and exits 0 - or raises.  The yardstick is tests/helpers/adej_ref.py.

Statistical bounds (the exact posterior at one rate, the number of rates under the prior alone): a pooled mean lies within
5 sd_exact / sqrt(ESS) of the exact expectation, ESS being Tracer's, summed over the chains, and at least ESS_FLOOR - a
condition of the test, asserted."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import ade_ref  # noqa: E402
from helpers import adej_ref as ref  # noqa: E402

LL_TOL = 1e-9
ESS_FLOOR = 400.0
N_SIGMA = 5.0
# the exact posterior at one rate: host (the restatement, Philox in Python) and device
EXACT_SEED, EXACT_ITERS, EXACT_S, EXACT_BURN, EXACT_CHAINS_HOST = 11, 12000, 4, 250, 6
EXACT_CHAINS_DEV, EXACT_ITERS_DEV, EXACT_S_DEV, EXACT_BURN_DEV = 256, 4000, 10, 100
# the number of rates under the prior alone (the rates start near 0.4 and drift to the prior's 2 at +-10 % a move: until
# they are there a second rate is unlikely, so the burn-in is thousands of iterations)
PRIOR_SEED, PRIOR_ITERS, PRIOR_S, PRIOR_BURN, PRIOR_CHAINS_HOST = 12, 12000, 4, 750, 6
PRIOR_CHAINS_DEV, PRIOR_ITERS_DEV, PRIOR_S_DEV, PRIOR_BURN_DEV = 256, 12000, 20, 200


def say(*a):
    print(*a)
    sys.stdout.flush()


def table(name):
    """(dead, cens) of a named data set"""
    if name == "a12":                      # 480 lineages, 250 deaths, 71 classes
        ts, te = ade_ref.simulate(np.random.default_rng(5), 12, 40, np.repeat([0.10, 0.25], 6), 0.7, 1.0)
        return ade_ref.classes(ts, te, 0.0, 12)[:2]
    if name == "a40":                      # 1e5 lineages born uniformly over 40 bins, lifespans of mean 5 bins: 783 classes
        rng = np.random.default_rng(7)
        ts = 5.0 + rng.random(100000) * 40
        return ade_ref.classes(ts, ts + 0.001 + rng.exponential(5.0, 100000), 5.0, 40)[:2]
    if name in ("a1", "a2", "a64", "a65", "a128"):
        from helpers import ppc_age_cases as P
        A = int(name[1:])
        ts, te = P.lineages(np.random.default_rng(400 + A), {1: 50, 2: 200}.get(A, 6000), A, "year" if A % 2 == 0 else "continuous")
        return ade_ref.classes(ts, te, P.T0, A)[:2]
    if name == "full40":                   # a class in every cell
        A = 40
        dead = np.zeros((A, A), dtype=np.int64)
        for jb in range(A):
            dead[jb, :A - jb] = 1 + (np.arange(A - jb) * 7 + jb) % 5
        return dead, np.arange(A, dtype=np.int64) % 3
    if name == "one40":                    # a single class
        A = 40
        dead = np.zeros((A, A), dtype=np.int64)
        dead[3, 17] = 9
        return dead, np.zeros(A, dtype=np.int64)
    if name == "few128":                   # few data on many bins: the prior decides, K grows to the cap
        A = 128
        dead = np.zeros((A, A), dtype=np.int64)
        dead[0, 5], dead[60, 2] = 1, 1
        cens = np.zeros(A, dtype=np.int64)
        cens[100] = 1
        return dead, cens
    raise KeyError(name)


def rates(rng, S, n_bins, scale=1.0):
    return np.exp(rng.normal(size=(S, n_bins)) * 0.7 - 1.5) * scale


def _bound(what, mean, want, sd, ess):
    bound = N_SIGMA * sd / math.sqrt(ess) if ess > 0 else float("nan")
    say("   %s: mean %.6f, exact %.6f (sd %.6f), ESS %.0f, |difference| %.3g, bound %.3g" % (what, mean, want, sd, ess, abs(mean - want), bound))
    assert ess >= ESS_FLOOR, (what, ess)
    assert abs(mean - want) <= bound, (what, mean, want, bound)


def check_exact(rows, exact, pooled):
    """rows [C, n, ROW_W] (kept) of runs with const = 1, use_rate_hp = 0 on `a12`; exact: ref.grid_posterior;
    pooled(series [C, n]) -> (mean, ESS)"""
    rows = np.asarray(rows)
    g, m = rows[:, :, ref.COL["log_shape"]], rows[:, :, ref.COL["mean_rate"]]
    assert (rows[:, :, ref.COL["K"]] == 1).all()
    for what, f in (("g", g), ("g2", g * g), ("logm", np.log(m))):
        mean, ess = pooled(f)
        _bound(what, mean, exact[what][0], exact[what][1], ess)


def check_prior_k(rows, p, pooled):
    """rows [C, n, ROW_W] (kept) of prior-only runs; p: ref.k_prior_pmf"""
    Kc = np.asarray(rows)[:, :, ref.COL["K"]]
    for k in range(1, 5):
        mean, ess = pooled((Kc == k).astype(np.float64))
        _bound("P(K = %d)" % k, mean, p[k - 1], math.sqrt(p[k - 1] * (1.0 - p[k - 1])), ess)


# ------------------------------------------------------------------------------------------------
# trajectories: name -> (table, settings, seed, iterations, the chains compared); the seeds were picked on the CPU so that
# the restatement's smallest decision margin over the compared iterations is at least MARGIN_FLOOR (asserted again here)
# ------------------------------------------------------------------------------------------------
MARGIN_FLOOR = 1e-6
TRAJ_CHAINS, TRAJ_ITERS, TRAJ_COMPARED = 130, 400, (0, 64, 129)
TRAJ = {
    "a12": ("a12", dict(), 1, TRAJ_ITERS, TRAJ_COMPARED),
    "a40": ("a40", dict(), 1, TRAJ_ITERS, TRAJ_COMPARED),
    "a128": ("a128", dict(), 1, TRAJ_ITERS, TRAJ_COMPARED),
    "a12_const": ("a12", dict(const=1), 1, TRAJ_ITERS, TRAJ_COMPARED),
    "big12": ("big12", dict(), 1, TRAJ_ITERS, (0, 129)),          # counts beyond 32 bits: R and the classes through L2
    "cap128": ("few128", dict(poisson_prior=2000.0), 1, 1500, (0,)),      # K reaches LR_KMAX and an add is refused
}
RTOL = ATOL = 1e-9


def traj_table(name):
    if name == "big12":
        dead, cens = table("a12")
        dead, cens = dead * (1 << 28), cens * (1 << 28)
        # (the name's condition: a birth bin with more lineages than 32 bits hold, so FITS32 is 0 and the chain kernel reads
        # the doubles of R and of the class list from the workspace)
        assert int((cens + dead.sum(axis=1)).max()) > 2 ** 31 - 1
        return dead, cens
    return table(name)


def traj_reference(name):
    """the restatement's runs of the compared chains -> {chain: run dict}, and the smallest decision margin"""
    tab, kw, seed, n_it, chains = TRAJ[name]
    data = ref.Data(*traj_table(tab))
    st = ref.Settings(**kw)
    runs = {c: ref.run(data, 0.0, st, ref.PhiloxDraws(seed, c), n_it, 1) for c in chains}
    return runs, min(float(r["margin"].min()) for r in runs.values())


# ------------------------------------------------------------------------------------------------
# the GPU cases
# ------------------------------------------------------------------------------------------------
def same(what, got, want_):
    ok = got == want_ if isinstance(got, (list, bytes)) else np.array_equal(np.asarray(got), np.asarray(want_))
    say("%s: %s" % (what, "identical" if ok else "DIFFER"))
    assert ok, what


def bits(ts):
    return [np.ascontiguousarray(t.cpu().numpy()).tobytes() for t in ts]


def dev_data(dead, cens):
    import torch
    from literate_amd import ops
    return ops.adej_prepare(torch.as_tensor(dead, device="cuda"), torch.as_tensor(cens, device="cuda"))


def settings(**kw):
    from literate_amd import ops
    return ops.AdejSettings(**kw)


LOGLIK_TABLES = ("a1", "a2", "a40", "a64", "a65", "a128", "full40", "one40", "big12")
LOGLIK_SHAPES = (0.125, 1.0, 8.0)
LOGLIK_SCALES = (1.0, 1e-12, 1e6)


def loglik_inputs(name):
    dead, cens = traj_table(name)
    A = len(cens)
    rng = np.random.default_rng(500 + A)
    base = rates(rng, 2, A)
    mu = np.concatenate([base[i % 2][None, :] * f for i, f in enumerate(LOGLIK_SCALES) for _ in LOGLIK_SHAPES])
    return dead, cens, mu, np.tile(LOGLIK_SHAPES, len(LOGLIK_SCALES))


def case_loglik():
    """lr_adej_loglik against the restatement within LL_TOL sum n |class term|, and the same bits from a second call on
    the dirty outputs"""
    import torch
    from literate_amd import ops
    for name in LOGLIK_TABLES:
        dead, cens, mu, sh = loglik_inputs(name)
        want, wflag, mag = ref.loglik_rows(dead, cens, mu, sh)
        data = dev_data(dead, cens)
        out = ops.adej_loglik(data, mu, sh)
        ll, flag = (t.cpu().numpy() for t in out)
        assert not wflag.any() and np.array_equal(flag, wflag), (name, flag)
        err, bound = np.abs(ll - want), LL_TOL * mag
        say("%s: %d classes, %d rows, worst |dl| / bound %.3g" % (name, int((np.asarray(dead) > 0).sum()), len(sh), float(np.max(err / np.where(bound > 0, bound, 1.0)))))
        assert (err <= bound).all(), (name, err, bound)
        first = bits(out)
        out[0].fill_(123.0), out[1].fill_(123)
        same(name + " again on dirty outputs", bits(ops.adej_loglik(data, mu, sh, out=out)), first)
        data2 = ops.adej_prepare(torch.as_tensor(dead, device="cuda"), torch.as_tensor(cens, device="cuda"), out=data)
        same(name + " after a second prepare into the dirty workspace", bits(ops.adej_loglik(data2, mu, sh)), first)


def case_flags():
    """flagged rows beside good ones leave the good ones bit-identical"""
    from literate_amd import ops
    dead, cens, mu, sh = loglik_inputs("a40")
    data = dev_data(dead, cens)
    good = bits(ops.adej_loglik(data, mu, sh))
    ll0 = np.frombuffer(good[0])
    A = mu.shape[1]
    je = int(np.nonzero(ref.Data(dead, cens).je >= 0)[0][0] * 0 + ref.Data(dead, cens).je[0])
    quiet = [b for b in range(A) if b not in set(ref.Data(dead, cens).je.tolist())]
    mu2, sh2 = mu.copy(), sh.copy()
    mu2[0, 3], mu2[2, 5], mu2[4, A - 1], mu2[6, je] = np.nan, -1.0, np.inf, 0.0
    sh2[1], sh2[3], sh2[5], sh2[7] = 0.0, -2.0, np.nan, np.inf
    if quiet:
        mu2[8, quiet[0]] = 0.0                                     # zero where no death was observed: a good row
    want, wflag, _ = ref.loglik_rows(dead, cens, mu2, sh2)
    ll, flag = (t.cpu().numpy() for t in ops.adej_loglik(data, mu2, sh2))
    say("flags %s" % flag.tolist())
    assert np.array_equal(flag, wflag) and flag[:8].tolist() == [1, 2, 1, 2, 1, 2, 1, 2] and flag[8] == 0
    assert np.isnan(ll[:8]).all() and np.isfinite(ll[8])
    if not quiet:
        assert ll[8].tobytes() == ll0[8].tobytes()
    solo = ops.adej_loglik(data, mu2[8:9], sh2[8:9])[0].cpu().numpy()
    assert solo.tobytes() == ll[8:9].tobytes()


def case_arguments():
    """every refusal returns its code, in the documented order, and leaves the buffers untouched"""
    import torch
    from literate_amd import _hip
    lib = _hip.load()
    E, P_ = _hip, _hip.ptr
    A, S, C = 20, 4, 3
    dev = torch.device("cuda")
    dead = torch.zeros((A, A), dtype=torch.int64, device=dev)
    dead[2, 3] = 5
    cens = torch.ones(A, dtype=torch.int64, device=dev)
    need = lib.lr_adej_workspace_bytes(A)
    assert need > 0 and lib.lr_adej_workspace_bytes(0) == E.LR_ERR_SIZE and lib.lr_adej_workspace_bytes(129) == E.LR_ERR_SIZE
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=dev)

    def prepare(**kw):
        a = dict(dead=P_(dead), cens=P_(cens), nb=A, ws=P_(ws), wsb=need)
        a.update(kw)
        return _hip.launch(lib.lr_adej_prepare, dev, a["dead"], a["cens"], a["nb"], a["ws"], a["wsb"])

    for kw, code in ((dict(dead=None), E.LR_ERR_NULL), (dict(cens=None), E.LR_ERR_NULL), (dict(ws=None), E.LR_ERR_NULL),
                     (dict(nb=0), E.LR_ERR_SIZE), (dict(nb=129), E.LR_ERR_SIZE), (dict(wsb=need - 1), E.LR_ERR_WORKSPACE),
                     (dict(dead=None, nb=0, wsb=0), E.LR_ERR_NULL), (dict(nb=0, wsb=0), E.LR_ERR_SIZE)):
        rc = prepare(**kw)
        say("lr_adej_prepare %s -> %d" % (sorted(kw), rc))
        assert rc == code, (kw, rc, code)
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all())
    assert prepare() == 0

    mu = torch.rand(S, A, dtype=torch.float64, device=dev) + 0.1
    sh = torch.ones(S, dtype=torch.float64, device=dev)
    ll = torch.full((S,), 123.0, dtype=torch.float64, device=dev)
    flag = torch.full((S,), 123, dtype=torch.int32, device=dev)

    def loglik(**kw):
        a = dict(ws=P_(ws), wsb=need, nb=A, mu=P_(mu), sh=P_(sh), S=S, ll=P_(ll), flag=P_(flag))
        a.update(kw)
        return _hip.launch(lib.lr_adej_loglik, dev, a["ws"], a["wsb"], a["nb"], a["mu"], a["sh"], a["S"], a["ll"], a["flag"])

    for kw, code in ((dict(ws=None), E.LR_ERR_NULL), (dict(mu=None), E.LR_ERR_NULL), (dict(sh=None), E.LR_ERR_NULL),
                     (dict(ll=None), E.LR_ERR_NULL), (dict(flag=None), E.LR_ERR_NULL), (dict(S=0), E.LR_ERR_SIZE),
                     (dict(nb=0), E.LR_ERR_SIZE), (dict(nb=129), E.LR_ERR_SIZE), (dict(wsb=need - 1), E.LR_ERR_WORKSPACE),
                     (dict(ll=None, S=0, wsb=0), E.LR_ERR_NULL), (dict(S=0, wsb=0), E.LR_ERR_SIZE)):
        rc = loglik(**kw)
        say("lr_adej_loglik %s -> %d" % (sorted(kw), rc))
        assert rc == code, (kw, rc, code)
    torch.cuda.synchronize()
    assert bool((ll == 123.0).all()) and bool((flag == 123).all())
    assert loglik() == 0

    state = torch.full((C, E.LR_ADEJ_STATE_W), 123.0, dtype=torch.float64, device=dev)
    rows = torch.full((10, C, E.LR_ADEJ_ROW_W), 123.0, dtype=torch.float64, device=dev)

    def chain(steps, **kw):
        a = dict(ws=P_(ws), wsb=need, nb=A, t0=0.0, const=0, hp=1, poi=0.0, win=0.4, seed=5, c0=0, C=C, state=P_(state), it0=0,
                 n=10, s=1, rows=P_(rows), nr=10)
        a.update(kw)
        head = (a["ws"], a["wsb"], a["nb"], a["t0"], a["const"], a["hp"], a["poi"], a["win"], a["seed"], a["c0"], a["C"], a["state"])
        if steps:
            return _hip.launch(lib.lr_adej_steps, dev, *head, a["it0"], a["n"], a["s"], a["rows"], a["nr"])
        return _hip.launch(lib.lr_adej_init, dev, *head)

    both = ((dict(ws=None), E.LR_ERR_NULL), (dict(state=None), E.LR_ERR_NULL), (dict(nb=0), E.LR_ERR_SIZE),
            (dict(nb=129), E.LR_ERR_SIZE), (dict(C=0), E.LR_ERR_SIZE), (dict(c0=-1), E.LR_ERR_SIZE), (dict(win=0.0), E.LR_ERR_MODEL),
            (dict(win=float("nan")), E.LR_ERR_MODEL), (dict(poi=-1.0), E.LR_ERR_MODEL), (dict(poi=float("inf")), E.LR_ERR_MODEL),
            (dict(t0=0.5), E.LR_ERR_T0), (dict(t0=float("nan")), E.LR_ERR_T0), (dict(wsb=need - 1), E.LR_ERR_WORKSPACE),
            (dict(state=None, C=0, win=0.0, t0=0.5, wsb=0), E.LR_ERR_NULL), (dict(C=0, win=0.0, t0=0.5, wsb=0), E.LR_ERR_SIZE),
            (dict(win=0.0, t0=0.5, wsb=0), E.LR_ERR_MODEL), (dict(t0=0.5, wsb=0), E.LR_ERR_T0))
    only_steps = ((dict(rows=None), E.LR_ERR_NULL), (dict(it0=-1), E.LR_ERR_SIZE), (dict(n=-1), E.LR_ERR_SIZE),
                  (dict(s=0), E.LR_ERR_SIZE), (dict(nr=9), E.LR_ERR_SIZE), (dict(it0=3, n=10, s=3, nr=3), E.LR_ERR_SIZE))
    for steps, table_ in ((False, both), (True, both + only_steps)):
        for kw, code in table_:
            rc = chain(steps, **kw)
            say("%s %s -> %d" % ("lr_adej_steps" if steps else "lr_adej_init", sorted(kw), rc))
            assert rc == code, (steps, kw, rc, code)
    torch.cuda.synchronize()
    assert bool((state == 123.0).all()) and bool((rows == 123.0).all())
    assert chain(False) == 0 and chain(True, it0=3, n=10, s=3, nr=4) == 0 and chain(True, n=0, rows=None, nr=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(state).all()) and bool((rows[:4, :, 0] == torch.tensor([3.0, 6.0, 9.0, 12.0], device=dev)[:, None]).all())
    assert bool((rows[4:] == 123.0).all())


def compare_run(label, rows, state, runs, chains):
    """device rows [n, C, W] and state [C, W] against the restatement's runs of `chains`"""
    from literate_amd import ops
    worst = 0.0
    for c in chains:
        r = runs[c]
        got, want = rows[:, c], r["rows"]
        assert got.shape == want.shape, (label, got.shape, want.shape)
        assert np.array_equal(got[:, ref.COL["K"]], want[:, ref.COL["K"]]), (label, c, "K")
        assert np.array_equal(np.isnan(got), np.isnan(want)), (label, c, "unused slots")
        s = r["state"]
        sp = state[c, ops.ADEJ_STATE["proposed"]:ops.ADEJ_STATE["proposed"] + 5]
        sa = state[c, ops.ADEJ_STATE["accepted"]:ops.ADEJ_STATE["accepted"] + 5]
        assert np.array_equal(sp, s.proposed) and np.array_equal(sa, s.accepted), (label, c, sp, s.proposed, sa, s.accepted)
        # which proposals were accepted: the posterior column changes exactly where the restatement accepted a change
        used = ~np.isnan(want)
        err = np.abs(got[used] - want[used]) / (ATOL + RTOL * np.abs(want[used]))
        worst = max(worst, float(err.max()))
        assert np.allclose(got[used], want[used], rtol=RTOL, atol=ATOL), (label, c, float(err.max()))
        K = len(s.m)
        assert state[c, 0] == K and np.allclose(state[c, 16:16 + K], s.m, rtol=RTOL, atol=ATOL)
        assert np.allclose(state[c, 48:48 + K + 1], s.times, rtol=RTOL, atol=ATOL) and (state[c, 16 + K:48] == 0).all()
        assert np.allclose(state[c, 1:6], [s.g, s.rate_hp, s.poi_hp, s.lik, s.prior], rtol=RTOL, atol=ATOL)
    say("%s: chains %s equal the restatement, worst error / tolerance %.3g" % (label, list(chains), worst))


def case_trajectory(name):
    """chains of a 130-chain run against the restatement, iteration by iteration"""
    from literate_amd import ops
    tab, kw, seed, n_it, chains = TRAJ[name]
    runs, margin = traj_reference(name)
    r0 = runs[chains[0]]
    say("%s: smallest decision margin %.3g; moves proposed %s, accepted %s, largest K %d, adds refused at the cap %d"
        % (name, margin, r0["state"].proposed.tolist(), r0["state"].accepted.tolist(), int(r0["K"].max()), r0["forced"]))
    assert margin >= MARGIN_FLOOR, margin
    if name == "cap128":
        assert r0["K"].max() == ref.KMAX and r0["forced"] >= 1
    else:
        assert (r0["kind"] == ref.SHAPE).any() and (r0["accepted"] & (r0["kind"] == ref.MULT)).any()
        if not kw.get("const"):
            assert max(int(r["K"].max()) for r in runs.values()) > 1
    data = dev_data(*traj_table(tab))
    C = TRAJ_CHAINS if len(chains) > 1 else 1
    rows, state = ops.adej_run(data, 0.0, C, n_it, 1, seed, settings(**kw))
    compare_run(name, rows.cpu().numpy(), state.cpu().numpy(), runs, chains)


def case_function():
    """the run is a function of its arguments: one launch against two, a chain alone against the chain among 130, dirty
    state and row buffers on entry"""
    import torch
    from literate_amd import ops
    for tab, n_a in (("a12", 150), ("a128", 151)):
        data = dev_data(*table(tab))
        st = settings()
        C, n_it, seed, s = 130, 400, 3, 3
        rows, state = ops.adej_run(data, 0.0, C, n_it, s, seed, st)
        state2 = torch.full_like(state, 123.0)
        ops.adej_init(data, 0.0, C, seed, st, out=(state2,))
        dirty = torch.full((ops.rows_due(0, n_a, s), C, rows.shape[2]), 123.0, dtype=torch.float64, device="cuda")
        ra = ops.adej_steps(data, 0.0, state2, 0, n_a, s, seed, st, out=(dirty,))
        rb = ops.adej_steps(data, 0.0, state2, n_a, n_it - n_a, s, seed, st)
        same("%s: %d + %d iterations against %d, rows" % (tab, n_a, n_it - n_a, n_it), bits([torch.cat([ra, rb])]), bits([rows]))
        same("%s: the state after them" % tab, bits([state2]), bits([state]))
        for c in (0, 77, 129):
            r1, s1 = ops.adej_run(data, 0.0, 1, n_it, s, seed, st, chain0=c)
            same("%s: chain %d alone" % (tab, c), bits([r1[:, 0], s1[0]]), bits([rows[:, c], state[c]]))


def case_contract():
    """exact-size guarded buffers (helpers.abi_cases.contract / refuses): workspace, outputs, state and rows"""
    import torch
    from literate_amd import ops
    from helpers.abi_cases import contract, refuses
    for tab, C in (("a1", 1), ("a40", 3), ("a65", 2), ("a128", 2)):
        dead, cens = table(tab)
        dead_d, cens_d = torch.as_tensor(dead, device="cuda"), torch.as_tensor(cens, device="cuda")
        A = len(cens)
        mu = torch.as_tensor(rates(np.random.default_rng(3), 2, A), device="cuda")
        sh = torch.as_tensor([0.7, 2.0], device="cuda")

        def whole():
            data = ops.adej_prepare(dead_d, cens_d)
            ll, flag = ops.adej_loglik(data, mu, sh)
            rows, state = ops.adej_run(data, 0.0, C, 40, 3, 9)
            return ll, flag, rows, state

        contract(ops, torch, whole, label="adej bins %d" % A)
        refuses(ops, torch, lambda: ops.adej_prepare(dead_d, cens_d), "LR_ERR_WORKSPACE", short=1, label=tab, entry="lr_adej_prepare")
        say("adej bins %d: contract kept" % A)


def _dev_pooled(torch, ops):
    def pooled(series):
        x = torch.as_tensor(np.ascontiguousarray(np.asarray(series).T), device="cuda")[:, :, None].contiguous()   # [n, C, 1]
        es = ops.ess_summary(x, x.shape[0], [0], burnin=0.0)
        return float(es.pooled_mean[0]), float(es.pooled_ess[0])
    return pooled


def case_exact():
    """the exact posterior at one rate, on the device"""
    import torch
    from literate_amd import ops
    dead, cens = table("a12")
    exact = ref.grid_posterior(ref.Data(dead, cens))
    rows, _ = ops.adej_run(dev_data(dead, cens), 0.0, EXACT_CHAINS_DEV, EXACT_ITERS_DEV, EXACT_S_DEV, EXACT_SEED,
                           settings(const=1, use_rate_hp=0))
    kept = rows[EXACT_BURN_DEV:].permute(1, 0, 2).cpu().numpy()
    check_exact(kept, exact, _dev_pooled(torch, ops))


def case_prior_k():
    """the number of rates under the prior alone, on the device"""
    import torch
    from literate_amd import ops
    A = 12
    rows, _ = ops.adej_run(dev_data(np.zeros((A, A), dtype=np.int64), np.zeros(A, dtype=np.int64)), 0.0, PRIOR_CHAINS_DEV,
                           PRIOR_ITERS_DEV, PRIOR_S_DEV, PRIOR_SEED, settings(poisson_prior=2.0, use_rate_hp=0))
    kept = rows[PRIOR_BURN_DEV:].permute(1, 0, 2).cpu().numpy()
    check_prior_k(kept, ref.k_prior_pmf(A, 2.0), _dev_pooled(torch, ops))


REC_BINS, REC_BIRTHS, REC_SEED = 30, 100, 20261019
REC_MU = np.repeat([0.05, 0.15, 0.3], 10)


def case_recovery():
    """three rate levels and k = 0.7: the 95 % HPD of the shape holds 0.7 and that of K values above 1; k = 1: it holds 1"""
    from literate_amd import ade_joint
    for k in (0.7, 1.0):
        ts, te = ade_ref.simulate(np.random.default_rng(REC_SEED), REC_BINS, REC_BIRTHS, REC_MU, k, 1.0)
        res = ade_joint.run(ts, te, 0.0, REC_BINS, 64, 6000, 10, 17)
        f = res.fit
        say("k = %s: shape %.4f (%.4f - %.4f), K mean %.2f (%g - %g), ESS of log shape %.0f, R-hat %.4f, acceptance %s"
            % (k, f["shape_mean"], f["shape_hpd_low"], f["shape_hpd_high"], f["K_mean"], f["K_hpd_low"], f["K_hpd_high"],
               f["log_shape_ess"], f["log_shape_rhat"], [round(f["accept_" + m], 3) for m in ade_joint.MOVES]))
        assert f["shape_hpd_low"] <= k <= f["shape_hpd_high"]
        assert f["K_hpd_high"] > 1
        assert f["deaths"] + f["censored"] == f["lineages_used"] == REC_BINS * REC_BIRTHS
        rates_ = np.array(res.rates)
        assert rates_.shape == (REC_BINS, 4) and (rates_[:, 2] <= rates_[:, 1]).all() and (rates_[:, 1] <= rates_[:, 3]).all()


# ------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------
N_IT, S_FREQ, CH = 2000, 10, 4
OTHER = ["--ade", "0.2", "--ade_draws", "20", "--ess", "0.2"]
OTHER_FILES = ("_ADE.tsv", "_ADE_shape.tsv", "_ESS.tsv", "_ESS_chains.tsv")
JOINT_FILES = ("_ADE_joint.tsv", "_ADE_joint_rates.tsv", "_ADE_joint_draws.npz")


def _cli(script, data, extra, joint=("--ade_joint", "0.2"), check=True):
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, script), "-d", data, "-TBP", "-n", str(N_IT), "-s", str(S_FREQ), "-p", "1000",
           "-seed", "31", "--chains", str(CH)] + list(joint) + extra
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_PPC_AGE_SLICES", "LR_WAIC_SLICES"):
        env.pop(k, None)
    return subprocess.run(cmd, check=check, capture_output=True, text=True, timeout=280, env=env)


def _check_files(stem, n_lineages, n_bins):
    from literate_amd import ade_joint
    fit, rates_, draws = ade_joint.read_tables(stem)
    say("fit row: %s" % fit)
    kept = N_IT // S_FREQ - int(0.2 * (N_IT // S_FREQ))
    assert list(fit) == ade_joint.FIT_HEAD and all(np.isfinite(v) for v in fit.values())
    assert fit["chains"] == CH and fit["iterations"] == N_IT and fit["samples_kept"] == kept and fit["bins"] == n_bins
    assert fit["lineages"] == n_lineages and fit["deaths"] + fit["censored"] == fit["lineages_used"] and fit["deaths"] > 0
    assert 0.125 <= fit["shape_hpd_low"] <= fit["shape_median"] <= fit["shape_hpd_high"] <= 8.0 and 0.0 <= fit["p_shape_lt_1"] <= 1.0
    assert len(rates_) == n_bins and [r[0] for r in rates_] == list(range(n_bins)) and all(r[2] <= r[1] <= r[3] for r in rates_)
    assert all(draws[k].shape == (kept, CH) for k in ade_joint.DRAW_KEYS) and np.isfinite(draws["lik"]).all()


def _with_and_without(script, data, stem, extra, n_lineages, n_bins):
    out = _cli(script, data, extra + OTHER).stdout
    line = [l for l in out.splitlines() if l.startswith("ADE joint:")]
    say(line)
    assert len(line) == 1 and "_ADE_joint.tsv" in line[0]
    _check_files(stem, n_lineages, n_bins)
    beside = {k: open(stem + k, "rb").read() for k in OTHER_FILES}
    for k in OTHER_FILES + JOINT_FILES:
        os.remove(stem + k)
    out = _cli(script, data, extra + OTHER, joint=()).stdout
    assert "ADE joint:" not in out and not any(os.path.exists(stem + k) for k in JOINT_FILES)
    for k in OTHER_FILES:
        same("%s beside --ade_joint and without it" % k, beside[k], open(stem + k, "rb").read())
    for joint, word in ((("--ade_joint", "1.5"), "burn-in"), (("--ade_joint", "0.2", "--ade_joint_win", "0"), "--ade_joint_win"),
                        (("--ade_joint", "0.2", "--ade_joint_n", "10"), "samples")):
        r = _cli(script, data, extra, joint=joint, check=False)
        say("%s -> exit %d: %s" % (joint, r.returncode, (r.stderr.strip().splitlines() or [""])[-1][:160]))
        assert r.returncode != 0 and word in r.stderr


def case_cli_lrf():
    import tempfile
    from helpers import waic_cases as W
    from literate_amd import logs
    with tempfile.TemporaryDirectory() as tmp:
        data = W._data(tmp)
        ts = W._lrf_lineages(data)[0]
        stem = logs.log_paths(data, 2)[1]["div"][:-len("_div.log")]
        r = _cli("LiteRateForward.py", data, ["-model_BDI", "3"], check=False)
        assert r.returncode != 0 and "-model_BDI 3" in r.stderr
        _with_and_without("LiteRateForward.py", data, stem, ["-model_BDI", "2"], len(ts), W._dd_setup(data)[3])


def case_cli_dd():
    import tempfile
    from helpers import waic_cases as W
    from literate_amd.ddrate import model_suffix
    with tempfile.TemporaryDirectory() as tmp:
        data = W._data(tmp)
        setup = W._dd_setup(data)
        _with_and_without("DDRate.py", data, os.path.join(tmp, "example_31" + model_suffix(2, 2)), ["-m_birth", "2", "-m_death", "2"],
                          len(setup[0]), setup[3])


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
