"""The GPU cases of tests/test_hip_waic.py, each run in a child process of its own (under the test's time limit):

    python tests/helpers/waic_cases.py CASE [ARGS...]

A case prints its figures, asserts, and exits 0 - or raises.  The yardstick is tests/helpers/waic_ref.py: the full
[lineages, draws] matrix in np.longdouble and the defining formulas.

The bound.  Errors are counted in units of u_i = eps A_i for lppd_i and mean_i and of u_i max(spread_i, u_i) for var_i
(A_i = max_s(|logB[js]| + |logD[je]| + sum_b R[s, b]), spread_i = max_s l - min_s l: the table's cumulative sums set the
scale, not |l|).  A case first measures the worst count of the FLOAT64 restatement against the longdouble one over its own
configurations; the device may show 16 times that, and at least 8: it differs from numpy in lr_log (<= 1.2 ulp), fma
contraction, the order of the sums and the online forms (running maximum, Welford / Chan), and in nothing larger.

Worst counts measured on an MI355X (lppd, mean, var), float64 restatement | device, in the cases recorded so far
(profiles/EXPERIMENTS.md, section "Pointwise WAIC", holds the list and the command):
    against 2 a   1.70 1.15 2.12 | 1.79 3.48 1.59        against 3 d   2.85 2.09 4.79 | 3.65 3.20 6.84
    against 0 b   1.80 1.50 3.01 | 0.89 0.81 1.58        12th digit    0.46 0.61 0.13 | 0.27 2.51 0.83
    slices (400 draws; 1, 2, 7 and the plan's 8 or 16 slices)    0.23 0.42 0.02 | 0.40 2.55 0.07 (mean: one slice)
The device's mean is the Welford form, whose error grows with the draws of a slice; the sums of numpy are pairwise."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import waic_ref  # noqa: E402

EPS = waic_ref.EPS
T0 = 5.0
N_BINS_GROUPS = {"a": (1, 38), "b": (39, 134), "c": (135, 262), "d": (263, None)}      # None: the largest accepted
NS = (1, 2, 257, 1031)
KINDS = ("continuous", "year", "integer")


def say(*a):
    print(*a)
    sys.stdout.flush()


def largest_bins(model):
    return 2398 if model == 3 else 4094


def lineages(rng, n, n_bins, kind):
    """n lineages around the window [T0, T0 + n_bins), some born before it or dead after it; with more than two of them the
    first lies wholly before the window and the second wholly after it"""
    span = n_bins + 3.0
    ts = T0 - 2.0 + rng.random(n) * span
    te = ts + 0.01 + rng.random(n) * np.minimum(span * 0.5, 40.0)
    if kind == "year":
        ts = np.floor(ts)
        te = np.floor(te) + 0.5
        te = np.where(te <= ts, ts + 0.5, te)
    elif kind == "integer":
        ts = np.floor(ts)
        te = np.maximum(np.floor(te), ts + 1.0)
    if n > 2:
        ts[0], te[0] = (T0 - 3.75, T0 - 1.25) if kind == "continuous" else (T0 - 4.0, T0 - 1.0 if kind == "integer" else T0 - 1.5)
    if n > 2:
        ts[1], te[1] = T0 + n_bins + 1.0, T0 + n_bins + (3.0 if kind == "integer" else 2.5)
    return ts, te


def rates(rng, S, n_bins):
    return np.exp(rng.normal(size=(S, n_bins)) * 0.7 - 1.5), np.exp(rng.normal(size=(S, n_bins)) * 0.7 - 1.5)


def model_inputs(rng, model, n_bins, te):
    br = None
    if model == 0:
        br = rng.random(n_bins) * 50.0
        br[rng.random(n_bins) < 0.2] = 0.0              # bins nobody lived in: zero terms
    end = float(np.quantile(te, 0.7)) if model == 3 else 0.0
    return br, end


def device(ts, te, lam, mu, model, br, end, offset=False):
    """ops.waic_pointwise -> host (pointwise, totals, plan); offset: ts / te as views one element into a longer tensor"""
    import torch
    from literate_amd import ops
    if offset:
        a = torch.as_tensor(np.concatenate(([0.0], ts)), device="cuda")[1:]
        b = torch.as_tensor(np.concatenate(([0.0], te)), device="cuda")[1:]
        assert a.data_ptr() % 16 == 8 and b.data_ptr() % 16 == 8
    else:
        a, b = torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda")
    pw, tot, plan = ops.waic_pointwise(a, b, T0, lam, mu, model=model, br_length=br, end_time=end)
    return pw.cpu().numpy(), tot.cpu().numpy(), plan


def allowed_counts(worst_f64):
    return np.maximum(16.0 * np.asarray(worst_f64), 8.0)


def check_totals(tot, pw, ld, allowed):
    """the totals against the longdouble restatement: the sums to the pointwise bound summed over the lineages, the
    standard error by the Lipschitz bound of a sample deviation (|sd(x + d) - sd(x)| <= |d|_2 / sqrt(n - 1)), the count
    and the maximum exactly as the device's own pointwise values give them"""
    want, U = ld["totals"], waic_ref.units(ld)
    n = len(pw)
    assert tot[0] == want[0] == n and tot[1] == want[1] == 0
    slack = 4.0 * n * EPS                                     # the rounding of an n-term sum, relative to the sum of |terms|
    for k, cols in ((2, (0,)), (3, (2,)), (4, (0, 2))):
        bound = sum(float(np.sum(allowed[c] * U[:, c])) for c in cols) + slack * sum(float(np.sum(np.abs(pw[:, c]))) for c in cols)
        err = abs(float(tot[k]) - float(want[k]))
        say("   total %s: |error| %.3g, bound %.3g" % (waic_ref.TOTALS[k], err, bound))
        assert err <= bound, (waic_ref.TOTALS[k], tot[k], want[k], bound)
    if n >= 2:
        elpd = pw[:, 0] - pw[:, 2]
        d = allowed[0] * U[:, 0] + allowed[2] * U[:, 2] + 2.0 * EPS * float(np.max(np.abs(elpd)))
        bound = np.sqrt(n / (n - 1.0)) * float(np.sqrt(np.sum(d * d))) + 8.0 * n * EPS * abs(float(want[5]))
        err = abs(float(tot[5]) - float(want[5]))
        say("   total se_elpd: |error| %.3g, bound %.3g" % (err, bound))
        assert err <= bound
    else:
        assert np.isnan(tot[5])
    assert tot[6] == np.sum(pw[:, 2] > 0.4) and tot[7] == pw[:, 2].max()


def run_configs(configs, model):
    """configs: dicts (n, n_bins, S, kind, shuffled, offset, seed).  First the float64 restatement's worst counts against the
    longdouble one over ALL of them, then the device against the bound that follows."""
    prepared, worst = [], np.zeros(3)
    for cfg in configs:
        rng = np.random.default_rng(cfg["seed"])
        ts, te = lineages(rng, cfg["n"], cfg["n_bins"], cfg["kind"])
        if not cfg["shuffled"]:
            o = np.lexsort((te, ts))
            ts, te = ts[o], te[o]
        lam, mu = rates(rng, cfg["S"], cfg["n_bins"])
        br, end = model_inputs(rng, model, cfg["n_bins"], te)
        ld = waic_ref.waic(ts, te, T0, lam, mu, model, br, end, dtype=np.longdouble)
        f64 = waic_ref.waic(ts, te, T0, lam, mu, model, br, end, dtype=np.float64)
        assert not ld["flagged"].any() and not f64["flagged"].any() and f64["totals"][1] == 0
        worst = np.maximum(worst, waic_ref.error_counts(f64["pointwise"], ld))
        prepared.append((cfg, ts, te, lam, mu, br, end, ld))
    allowed = allowed_counts(worst)
    say("float64 restatement, worst counts (lppd, mean, var): %s -> allowed on the device: %s" % (worst, allowed))
    dev_worst = np.zeros(3)
    for cfg, ts, te, lam, mu, br, end, ld in prepared:
        pw, tot, plan = device(ts, te, lam, mu, model, br, end, cfg["offset"])
        c = waic_ref.error_counts(pw, ld)
        dev_worst = np.maximum(dev_worst, c)
        say("model %d %s plan %s: counts %s" % (model, {k: cfg[k] for k in ("n", "n_bins", "S", "kind", "shuffled", "offset")}, plan, c))
        assert (c <= allowed).all(), (cfg, c, allowed)
        assert (pw[:, 2] >= 0).all()
        check_totals(tot, pw, ld, allowed)
    say("device, worst counts (lppd, mean, var): %s" % dev_worst)
    return worst, dev_worst


# Between the groups' bin counts (<= 263: several draws' tables per LDS buffer) and the largest accepted (one table, one
# buffer) lies the walk's middle regime: a draw's table above 16 KiB, two of them in LDS (38,464 B under models 0 and 2,
# 76,928 B under model 3), so the plan's chunk is 1 and the next table lands in the other buffer.
MIDDLE = dict(n=257, n_bins=1200, S=25, kind="continuous", shuffled=True, offset=False, seed=3201)


def case_against(model, group):
    """the device against the restatement at the table-size edges of one group of bin counts, every draw count around the
    LDS chunk, every lineage count, kind of times, order and alignment"""
    from literate_amd import ops
    model = int(model)
    configs, k = [], 0
    for nb in N_BINS_GROUPS[group]:
        nb = largest_bins(model) if nb is None else nb
        chunk = ops.waic_plan(1031, nb, 4096, model)[1]
        draws = sorted({S for S in (2, 3, chunk - 1, chunk, chunk + 1, 3 * chunk + 1) if S >= 2})
        if nb > 1000:
            draws = [S for S in draws if S <= 4]                  # (chunk = 1: 2, 3, 4 are chunk + 1 and 3 chunk + 1)
        for j, S in enumerate(draws):
            for n in (NS if j == 0 else (NS[k % 4],)):
                if nb * S * n > 6e7:                              # (the restatement holds [n, S] longdoubles and walks S tables)
                    n = 257
                configs.append(dict(n=n, n_bins=nb, S=S, kind=KINDS[k % 3], shuffled=bool(k & 1), offset=bool(k & 2), seed=1000 + k))
                k += 1
    run_configs(configs, model)
    if group == "d":                                              # (with a bound of its own: the others' stays what it was)
        assert ops.waic_plan(MIDDLE["n"], MIDDLE["n_bins"], MIDDLE["S"], model)[1] == 1
        run_configs([MIDDLE], model)


def case_exact():
    """identical draws; independence of the other lineages (subset, permutation); identical bits on a repeated call"""
    from literate_amd import ops
    import torch
    rng = np.random.default_rng(7)
    n, nb, S = 1031, 20, 64                                       # (64 draws < two chunks: the plan takes one slice at every n)
    ts, te = lineages(rng, n, nb, "continuous")
    lam, mu = rates(rng, S, nb)
    for model in (0, 2, 3):
        br, end = model_inputs(np.random.default_rng(8), model, nb, te)
        assert ops.waic_plan(n, nb, S, model)[2] == 1 and ops.waic_plan(300, nb, S, model)[2] == 1
        # all draws identical
        lam1, mu1 = np.repeat(lam[:1], S, 0), np.repeat(mu[:1], S, 0)
        pw, tot, _ = device(ts, te, lam1, mu1, model, br, end)
        assert np.array_equal(pw[:, 2], np.zeros(n)) and np.array_equal(pw[:, 0], pw[:, 1])
        ld = waic_ref.waic(ts, te, T0, lam1, mu1, model, br, end, dtype=np.longdouble)
        f64 = waic_ref.waic(ts, te, T0, lam1, mu1, model, br, end)
        allowed = allowed_counts(waic_ref.error_counts(f64["pointwise"], ld))
        batch = float(ops.bd_loglik_batch(torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda"), T0, lam[:1], mu[:1],
                                          model=model, br_length=br, end_time=end).cpu()[0])
        bound = 2.0 * allowed[0] * float(np.sum(waic_ref.units(ld)[:, 0])) + 8.0 * n * EPS * float(np.sum(np.abs(pw[:, 0])))
        say("model %d, identical draws: sum lppd %.17g, bd_loglik_batch %.17g, bound %.3g" % (model, tot[2], batch, bound))
        assert tot[3] == 0.0 and tot[2] == tot[4] and abs(tot[2] - batch) <= bound
        # a lineage's outputs do not depend on the others
        full, tot_full, _ = device(ts, te, lam, mu, model, br, end)
        sub = np.sort(rng.choice(n, 300, replace=False))
        part, _, _ = device(ts[sub], te[sub], lam, mu, model, br, end)
        assert np.array_equal(part, full[sub])
        perm = rng.permutation(n)
        mixed, _, _ = device(ts[perm], te[perm], lam, mu, model, br, end, offset=True)
        assert np.array_equal(mixed, full[perm])
        os.environ["LR_WAIC_SLICES"] = "3"                        # the same under draw slices, at the same slice count
        full3, _, plan3 = device(ts, te, lam, mu, model, br, end)
        part3, _, _ = device(ts[sub], te[sub], lam, mu, model, br, end)
        del os.environ["LR_WAIC_SLICES"]
        assert plan3[2] == 3 and np.array_equal(part3, full3[sub])
        # a repeated call
        again, tot_again, _ = device(ts, te, lam, mu, model, br, end)
        assert np.array_equal(again, full) and np.array_equal(tot_again, tot_full)
        say("model %d: subset, permutation and repetition identical" % model)


def case_slices():
    """the plan's own slice count and 1, 2 and 7 slices through LR_WAIC_SLICES, each within the bound"""
    from literate_amd import ops
    rng = np.random.default_rng(17)
    n, nb, S = 257, 38, 400
    ts, te = lineages(rng, n, nb, "year")
    lam, mu = rates(rng, S, nb)
    for model in (2, 3, 0):
        br, end = model_inputs(np.random.default_rng(18), model, nb, te)
        own = ops.waic_plan(n, nb, S, model)
        assert own[2] > 1, own
        ld = waic_ref.waic(ts, te, T0, lam, mu, model, br, end, dtype=np.longdouble)
        f64 = waic_ref.waic(ts, te, T0, lam, mu, model, br, end)
        worst = waic_ref.error_counts(f64["pointwise"], ld)
        allowed = allowed_counts(worst)
        say("model %d: float64 restatement %s, allowed %s, the plan's own slices %d" % (model, worst, allowed, own[2]))
        for k in (None, 1, 2, 7):
            if k is not None:
                os.environ["LR_WAIC_SLICES"] = str(k)
            pw, tot, plan = device(ts, te, lam, mu, model, br, end)
            os.environ.pop("LR_WAIC_SLICES", None)
            assert plan[2] == (own[2] if k is None else k)
            c = waic_ref.error_counts(pw, ld)
            say("   slices %d: counts %s" % (plan[2], c))
            assert (c <= allowed).all() and (pw[:, 2] >= 0).all()
            check_totals(tot, pw, ld, allowed)


def case_range():
    """draws more than 1500 nats apart (rates of 1e-300 and of 1 on a lineage that lives 1500 bins); draws that differ in
    the 12th digit"""
    nb = 1600
    ts = np.array([T0 + 10.25, T0 + 3.5, T0 + 700.0, T0 + 1590.5, T0 - 1.0])
    te = np.array([T0 + 1510.75, T0 + 4.25, T0 + 900.5, T0 + 1599.0, T0 + 1700.0])
    lam = np.ones((4, nb))
    lam[0], lam[2] = 1e-300, 1e-300
    mu = lam.copy()
    ld = waic_ref.waic(ts, te, T0, lam, mu, 2, dtype=np.longdouble)
    f64 = waic_ref.waic(ts, te, T0, lam, mu, 2)
    assert ld["spread"][0] > 1500 and not ld["flagged"].any()
    allowed = allowed_counts(waic_ref.error_counts(f64["pointwise"], ld))
    for k in (None, 2):
        if k:
            os.environ["LR_WAIC_SLICES"] = str(k)
        pw, tot, plan = device(ts, te, lam, mu, 2, None, 0.0)
        os.environ.pop("LR_WAIC_SLICES", None)
        c = waic_ref.error_counts(pw, ld)
        say("far apart (spread %.1f nats), slices %d: lppd %s, counts %s, allowed %s" % (ld["spread"][0], plan[2], pw[:, 0], c, allowed))
        assert np.isfinite(pw).all() and tot[1] == 0 and (c <= allowed).all()
    # the 12th digit
    rng = np.random.default_rng(27)
    n, nb, S = 257, 39, 33
    ts, te = lineages(rng, n, nb, "continuous")
    lam0, mu0 = rates(rng, 1, nb)
    scale = 1.0 + 1e-12 * np.arange(S)[:, None]
    lam, mu = lam0 * scale, mu0 * scale
    ld = waic_ref.waic(ts, te, T0, lam, mu, 2, dtype=np.longdouble)
    f64 = waic_ref.waic(ts, te, T0, lam, mu, 2)
    worst = waic_ref.error_counts(f64["pointwise"], ld)
    allowed = allowed_counts(worst)
    pw, tot, _ = device(ts, te, lam, mu, 2, None, 0.0)
    c = waic_ref.error_counts(pw, ld)
    say("12th digit: float64 restatement %s, device %s, allowed %s, largest var %.3g" % (worst, c, allowed, pw[:, 2].max()))
    assert (c <= allowed).all() and (pw[:, 2] >= 0).all() and pw[:, 2].max() < 1e-18


def case_flags():
    """one draw with a zero death rate in a bin where exactly k lineages die, one with a nan birth rate in a bin where j are
    born: exactly those are NaN, the counts are exact, every other lineage keeps its bits"""
    rng = np.random.default_rng(37)
    nb, S, k, j, rest = 10, 9, 5, 3, 600
    ts = np.concatenate([T0 + 4.0 + rng.random(k) * 1.5, T0 + 8.0 + rng.random(j) * 0.9, T0 - 1.0 + rng.random(rest) * 4.0])
    te = np.concatenate([T0 + 5.0 + 0.6 + rng.random(k) * 0.4, T0 + 9.0 + rng.random(j) * 0.9, np.zeros(rest)])
    te[k + j:] = ts[k + j:] + rng.random(rest) * (T0 + 3.99 - ts[k + j:])        # the rest: over before bin 4 begins
    assert (te > ts).all() and (te[k + j:] < T0 + 4.0).all()
    o = rng.permutation(len(ts))
    ts, te = ts[o], te[o]
    bad = np.isin(o, np.arange(k + j))
    lam, mu = rates(rng, S, nb)
    good, _, _ = device(ts, te, lam, mu, 2, None, 0.0)
    lam_b, mu_b = lam.copy(), mu.copy()
    mu_b[2, 5] = 0.0
    lam_b[6, 8] = np.nan
    ref = waic_ref.waic(ts, te, T0, lam_b, mu_b, 2)
    assert np.array_equal(ref["flagged"], bad)
    for sl in (None, 4):
        if sl:
            os.environ["LR_WAIC_SLICES"] = str(sl)
        clean, _, _ = device(ts, te, lam, mu, 2, None, 0.0)
        pw, tot, plan = device(ts, te, lam_b, mu_b, 2, None, 0.0)
        os.environ.pop("LR_WAIC_SLICES", None)
        assert np.isnan(pw[bad]).all() and np.isfinite(pw[~bad]).all()
        assert tot[0] == rest and tot[1] == k + j
        assert np.array_equal(pw[~bad], clean[~bad])
        if sl is None:
            assert np.array_equal(clean, good)
        elpd = pw[~bad, 0] - pw[~bad, 2]
        assert np.isclose(tot[4], elpd.sum(), rtol=1e-12) and np.isclose(tot[5], np.sqrt(rest * np.var(elpd, ddof=1)), rtol=1e-9)
        assert tot[7] == pw[~bad, 2].max() and tot[6] == np.sum(pw[~bad, 2] > 0.4)
        say("slices %d: %d flagged, %d used, the others identical" % (plan[2], tot[1], tot[0]))
    # every lineage flagged: no totals but the counts
    pw, tot, _ = device(ts[bad], te[bad], lam_b, mu_b, 2, None, 0.0)
    assert np.isnan(pw).all() and tot[0] == 0 and tot[1] == k + j and tot[2] == 0 and np.isnan(tot[5]) and np.isnan(tot[7])


def case_arguments():
    """every refusal returns its code and leaves the outputs untouched"""
    import torch
    from literate_amd import _hip
    lib = _hip.load()
    n, nb, S = 10, 20, 8
    ts = torch.rand(n, dtype=torch.float64, device="cuda") + T0
    te = ts + 1.0
    lam = torch.rand(S, nb, dtype=torch.float64, device="cuda") + 0.1
    br = torch.ones(nb, dtype=torch.float64, device="cuda")
    pw = torch.full((n, 3), 123.0, dtype=torch.float64, device="cuda")
    tot = torch.full((8,), 123.0, dtype=torch.float64, device="cuda")
    need2 = lib.lr_waic_workspace_bytes(n, nb, S, 2)
    need = max(lib.lr_waic_workspace_bytes(n, nb, S, m) for m in (0, 2, 3))
    assert 0 < need2 <= need
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    P = _hip.ptr

    def call(**kw):
        a = dict(ts=P(ts), te=P(te), n=n, t0=T0, nb=nb, lam=P(lam), mu=P(lam), S=S, model=2, br=None, pw=P(pw), tot=P(tot),
                 ws=P(ws), wsb=need)
        a.update(kw)
        return _hip.launch(lib.lr_waic_pointwise, ts.device, a["ts"], a["te"], a["n"], a["t0"], a["nb"], a["lam"], a["mu"], a["S"],
                           a["model"], a["br"], 0.0, a["pw"], a["tot"], a["ws"], a["wsb"])

    E = _hip
    for kw, code in ((dict(ts=None), E.LR_ERR_NULL), (dict(te=None), E.LR_ERR_NULL), (dict(lam=None), E.LR_ERR_NULL),
                     (dict(mu=None), E.LR_ERR_NULL), (dict(pw=None), E.LR_ERR_NULL), (dict(tot=None), E.LR_ERR_NULL),
                     (dict(ws=None), E.LR_ERR_NULL), (dict(n=0), E.LR_ERR_SIZE), (dict(n=-3), E.LR_ERR_SIZE),
                     (dict(S=1), E.LR_ERR_SIZE), (dict(S=0), E.LR_ERR_SIZE), (dict(nb=0), E.LR_ERR_SIZE),
                     (dict(nb=E.LR_MAX_BINS + 1), E.LR_ERR_SIZE), (dict(model=3, nb=2399), E.LR_ERR_SIZE),
                     (dict(model=1, br=P(br)), E.LR_ERR_MODEL), (dict(model=4), E.LR_ERR_MODEL), (dict(model=-1), E.LR_ERR_MODEL),
                     (dict(model=0), E.LR_ERR_MODEL), (dict(t0=T0 + 0.5), E.LR_ERR_T0), (dict(wsb=need2 - 1), E.LR_ERR_WORKSPACE),
                     (dict(wsb=0), E.LR_ERR_WORKSPACE)):
        rc = call(**kw)
        say("%s -> %d" % (sorted(kw), rc))
        assert rc == code, (kw, rc, code)
    torch.cuda.synchronize()
    assert bool((pw == 123.0).all()) and bool((tot == 123.0).all())              # nothing was launched
    assert call() == 0 and call(model=0, br=P(br)) == 0 and call(model=3) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pw).all()) and float(tot[0]) == n
    from literate_amd import ops
    for bad in (dict(model=1), dict(model=0)):
        try:
            ops.waic_pointwise(ts, te, T0, lam, lam, **bad)
        except ValueError as ex:
            assert "LR_ERR_MODEL" in str(ex)
        else:
            raise AssertionError(bad)


# ------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------
CH, N_IT, S_FREQ, DRAWS = 4, 3000, 10, 64


def _run_cli(script, data, extra):
    cmd = [sys.executable, os.path.join(ROOT, script), "-d", data, "-TBP", "-n", str(N_IT), "-s", str(S_FREQ), "-p", "1000",
           "-seed", "31", "--chains", str(CH), "--waic", "0.2", "--waic_draws", str(DRAWS)] + extra
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_WAIC_SLICES"):
        env.pop(k, None)
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=280, env=env).stdout
    line = [l for l in out.splitlines() if l.startswith("WAIC:")]
    say(line)
    assert len(line) == 1 and "_WAIC.tsv" in line[0] and "_WAIC_pointwise.npz" in line[0] and "%d draws" % DRAWS in line[0]


def _engine_order(ts, te):
    """the order the engines hold the lineages in (stable by te, then stable by the birth bin)"""
    o1 = np.argsort(te, kind="stable")
    return o1[np.argsort(np.floor(ts[o1]), kind="stable")]


def _draw_rows(per_chain):
    S = N_IT // S_FREQ
    assert all(len(r) == S for r in per_chain)
    flat = [per_chain[c][k] for k in range(int(0.2 * S), S) for c in range(CH)]     # sample-major, chain-minor
    return [flat[i] for i in waic_ref.draw_indices(len(flat), DRAWS)]


def _check_files(stem, ts, te, t0, lam, mu, model, br, end):
    """<stem>_WAIC.tsv and _pointwise.npz against the restatement on the rates read back from the logs"""
    from literate_amd import waic
    o = _engine_order(ts, te)
    ts, te = ts[o], te[o]
    ld = waic_ref.waic(ts, te, t0, lam, mu, model, br, end, dtype=np.longdouble)
    f64 = waic_ref.waic(ts, te, t0, lam, mu, model, br, end)
    assert not ld["flagged"].any()
    allowed = allowed_counts(waic_ref.error_counts(f64["pointwise"], ld))
    with open(stem + "_WAIC.tsv") as f:
        head, vals = [l.rstrip("\n").split("\t") for l in f]
    assert head == waic.TSV_HEAD and all("." not in vals[head.index(k)] for k in waic.TSV_INTS)
    row = dict(zip(head, [float(v) for v in vals]))
    z = np.load(stem + "_WAIC_pointwise.npz")
    elpd = z["elpd"]
    n, U, want = len(ts), waic_ref.units(ld), ld["totals"]
    assert (row["draws"], row["lineages"], row["lineages_used"], row["lineages_flagged"]) == (len(lam), n, n, 0)
    assert np.array_equal(z["fingerprint"], waic.fingerprint(ts, te, t0, lam.shape[1], model)) and elpd.shape == (n,)
    want_elpd = (ld["pointwise"][:, 0] - ld["pointwise"][:, 2]).astype(np.float64)
    tol = allowed[0] * U[:, 0] + allowed[2] * U[:, 2] + EPS * np.abs(want_elpd)
    say("%s: pointwise elpd, worst |error| / bound %.3g (allowed counts %s)" % (os.path.basename(stem), np.max(np.abs(elpd - want_elpd) / tol), allowed))
    assert (np.abs(elpd - want_elpd) <= tol).all()
    slack = 4.0 * n * EPS
    for name, k, cols in (("lppd", 2, (0,)), ("p_waic", 3, (2,)), ("elpd_waic", 4, (0, 2))):
        bound = sum(float(np.sum(allowed[c] * U[:, c])) for c in cols) + slack * sum(float(np.sum(np.abs(ld["pointwise"][:, c]))) for c in cols)
        say("   %s %.17g, restatement %.17g, bound %.3g" % (name, row[name], float(want[k]), bound))
        assert abs(row[name] - float(want[k])) <= bound
    d = tol + 2.0 * EPS * float(np.max(np.abs(want_elpd)))
    bound = np.sqrt(n / (n - 1.0)) * float(np.sqrt(np.sum(d * d))) + 8.0 * n * EPS * float(want[5])
    assert abs(row["se_elpd"] - float(want[5])) <= bound
    assert row["waic"] == -2.0 * row["elpd_waic"] and row["se_waic"] == 2.0 * row["se_elpd"]
    assert row["max_var"] >= 0 and row["n_var_gt_0.4"] <= n
    return row, elpd


def _data(tmp):
    from helpers.ppc_cases import _write_example
    data = os.path.join(tmp, "example.tsv")
    _write_example(data)
    return data


def _lrf_lineages(data):
    import argparse
    import LiteRateForward as cli
    ts, te, _ = cli.parse_data(argparse.Namespace(d=data, rev_se=False, TBP=True, first_year=-1, last_year=-1, death_jitter=0.5))
    return ts, te


def _run_lrf(tmp, data, model):
    from literate_amd import logs
    _run_cli("LiteRateForward.py", data, ["-model_BDI", str(model)])
    stem = logs.log_paths(data, model)[1]["div"][:-len("_div.log")]
    return stem


def case_cli_lrf(model):
    """LiteRateForward.py --waic against the restatement fed the rates of the logs the same run wrote"""
    from literate_amd import logs, ops
    model = int(model)
    with tempfile.TemporaryDirectory() as tmp:
        data = _data(tmp)
        stem = _run_lrf(tmp, data, model)
        ts, te = _lrf_lineages(data)
        t0, n_bins = float(int(ts.min())), int(te.max()) - int(ts.min())
        per_chain = []
        for c in range(CH):
            paths = logs.log_paths(data, model, chain=c)[1]
            mc = np.loadtxt(paths["mcmc"], skiprows=1)
            sp_rows = [np.array(l.split(), float) for l in open(paths["sp_rates"])]
            ex_rows = [np.array(l.split(), float) for l in open(paths["ex_rates"])]
            per_chain.append([(logs.rates_per_bin(a[:(len(a) + 1) // 2], a[(len(a) + 1) // 2:], m[8], n_bins),
                               logs.rates_per_bin(b[:(len(b) + 1) // 2], b[(len(b) + 1) // 2:], m[8], n_bins))
                              for m, a, b in zip(mc, sp_rows, ex_rows)])
        drawn = _draw_rows(per_chain)
        lam, mu = np.array([d[0] for d in drawn]), np.array([d[1] for d in drawn])
        br = ops.bin_unit_events(ts, te, t0, n_bins)[2].cpu().numpy() if model == 0 else None
        _check_files(stem, ts, te, t0, lam, mu, model, br, float(te.max()))


def _dd_setup(data):
    from literate_amd.literate_library import create_bins, parse_ts_te
    TS, TE, PRESENT, ORIGIN = parse_ts_te(data, True, -1, -1, .5)
    ts, te = np.asarray(TS, float), np.asarray(TE, float)
    origin, _, n_spec, n_exti, DT, n_bins, x = create_bins(ORIGIN, PRESENT, ts, te, 0)
    return ts, te, float(origin), int(n_bins), np.asarray(DT, float)


def _log_rows(paths):
    return _draw_rows([list(np.loadtxt(p, skiprows=1)) for p in paths])


def case_cli_dd():
    """DDRate.py --waic under two models against the restatement; python -m literate_amd.waic ranks the two and refuses a
    LiteRateForward.py file beside them"""
    from literate_amd import ops
    from literate_amd.ddrate import model_suffix
    with tempfile.TemporaryDirectory() as tmp:
        data = _data(tmp)
        ts, te, origin, n_bins, DT = _dd_setup(data)
        rows, files = {}, {}
        for mb, md in ((2, 2), (0, 0)):
            _run_cli("DDRate.py", data, ["-m_birth", str(mb), "-m_death", str(md)])
            stem = os.path.join(tmp, "example_31" + model_suffix(mb, md))
            par = np.array(_log_rows(["%s_c%d.log" % (stem, c) for c in range(CH)]))[:, 6:14].copy()
            par[:, 2] -= origin                                   # the log holds x0 + ORIGIN and L + div_0
            par[:, 4] -= par[:, 3]
            lam, mu = [v.cpu().numpy() for v in ops.dd_rates(par, DT, mb, md)[:2]]
            rows[(mb, md)], _ = _check_files(stem, ts, te, origin, lam, mu, 2, None, float(te.max()))
            files[(mb, md)] = stem + "_WAIC_pointwise.npz"
        cmd = [sys.executable, "-m", "literate_amd.waic", files[(2, 2)], files[(0, 0)], "-o", os.path.join(tmp, "table.tsv")]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
        say(out.stdout)
        assert out.returncode == 0, out.stderr
        lines = [l.split("\t") for l in out.stdout.splitlines()]
        assert len(lines) == 3 and lines[0][0] == "model" and open(os.path.join(tmp, "table.tsv")).read() == out.stdout
        best, other = lines[1], lines[2]
        e = {files[k]: np.load(files[k])["elpd"] for k in files}
        assert float(best[1]) == float(np.sum(e[best[0]])) >= float(other[1]) == float(np.sum(e[other[0]]))
        assert float(best[3]) == 0.0 and float(other[3]) == float(np.sum(e[other[0]] - e[best[0]]))
        assert abs(float(other[3]) - (float(other[1]) - float(best[1]))) <= 64 * EPS * abs(float(best[1]))
        assert float(best[2]) == rows[(2, 2) if best[0] == files[(2, 2)] else (0, 0)]["p_waic"]
        # a LiteRateForward.py file beside them: another window and model id
        lrf = _run_lrf(tmp, data, 0) + "_WAIC_pointwise.npz"
        out = subprocess.run([sys.executable, "-m", "literate_amd.waic", files[(2, 2)], lrf], capture_output=True, text=True,
                             timeout=120, cwd=ROOT)
        say(out.stderr.strip())
        assert out.returncode != 0 and "fingerprint mismatch" in out.stderr and "not comparable" in out.stderr


def case_cli_trend():
    """trend_rate.py --waic with a synthetic covariate against the restatement on ops.trend_rates of the drawn log rows"""
    from literate_amd import ops
    from literate_amd.trendrate import model_suffix, normalise_trend
    with tempfile.TemporaryDirectory() as tmp:
        data = _data(tmp)
        ts, te, origin, n_bins, DT = _dd_setup(data)
        raw = 3.0 + np.sin(np.arange(n_bins + 1) / 4.0) + np.arange(n_bins + 1) / 10.0
        trend_file = os.path.join(tmp, "trend.tsv")
        with open(trend_file, "w") as f:
            f.write("year\tcovariate\n" + "".join("%d\t%r\n" % (i, float(v)) for i, v in enumerate(raw)))
        _run_cli("trend_rate.py", data, ["-trend_data", trend_file, "-trend_index", "1"])
        stem = os.path.join(tmp, "example_31" + model_suffix(False, False))
        par = np.array(_log_rows(["%s_c%d_1.trendrate.log" % (stem, c) for c in range(CH)]))[:, 6:12]
        lam, mu = [v.cpu().numpy() for v in ops.trend_rates(par, normalise_trend(raw), False, False)]
        _check_files(stem + "_1", ts, te, origin, lam, mu, 2, None, float(te.max()))


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
