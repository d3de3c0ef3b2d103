"""The GPU cases of tests/test_hip_loo.py, each run in a child process of its own (under the test's time limit):

    python tests/helpers/loo_cases.py CASE [ARGS...]

A case prints its figures, asserts, and exits 0 - or raises.  The yardstick is tests/helpers/loo_ref.py: the published
algorithm row by row in np.longdouble.

The bound.  Errors are counted per output (elpd_loo, pareto_k, lppd, n_eff) in units of eps max(1, |value|) times the row's
tail condition x_M / x_1 (capped at 1e6; 1 where nothing is fitted): the fit divides by x_1-sized quantities what was
rounded at x_M's size.  Where the rows come from rates, the term's own unit u_i = eps A_i (waic_ref.units) times the same
condition is added: an error of u_i in every term moves every x_j by up to u_i x_M.  A case first measures the worst
count of the FLOAT64 restatement against the longdouble one over its own inputs; the device may show 16 times that, and
at least 8: it differs from numpy in exp, log, log1p and expm1 (the device library's), fma contraction and the order of
the sums, and in nothing larger.  Tail membership is exact wherever the restatement's gap between the cutoff and the
smallest tail value exceeds 64 u_i (always, for matrices the device and the restatement share bit for bit).

Worst counts measured on an MI355X (elpd_loo, pareto_k, lppd, n_eff), float64 restatement | device
(profiles/EXPERIMENTS.md, section "PSIS-LOO", holds the list and the command):
    rows small  5.40 3.62 1.89 3.33 | 5.40 4.58 1.89 3.07        rates 2  0.21 7.82 0.15 1.98 | 0.17 1.36 0.16 1.31
    rows mid    0.08 0.70 0.23 0.09 | 0.05 0.70 0.13 0.13        rates 0  0.30 9.03 0.15 1.90 | 0.36 5.61 0.30 1.75
    rows cap    0.02 0.29 0.01 0.04 | 0.03 0.26 0.01 0.01        rates 3  0.14 2.09 0.16 1.27 | 0.19 12.7 0.12 1.78"""
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

from helpers import loo_ref, waic_cases, waic_ref  # noqa: E402
from oracle import literate_oracle as lo  # noqa: E402
from helpers.waic_cases import T0, lineages, model_inputs, rates, say  # noqa: E402

EPS = loo_ref.EPS
ROW_GROUPS = {"small": (2, 24, 25, 26, 100), "mid": (225, 226, 1000, 1023, 1024, 1025), "cap": (8192,)}
N_ROWS = (1, 2, 257)
SPREADS = (0.1, 0.5, 2.0, 10.0, 50.0)


def allowed_counts(worst_f64):
    return np.maximum(16.0 * np.asarray(worst_f64), 8.0)


def row_matrix(rng, n_rows, S):
    """rows of log-likelihood terms with distinct entries: normal ratios of spread 0.1 ... 50 nats, a heavy-tailed row
    (ratios Pareto with shape near 1: r = E, E exponential) and a light one (ratios uniform: k < 0)"""
    L = np.empty((n_rows, S))
    for i in range(n_rows):
        kind = i % (len(SPREADS) + 2)
        if kind < len(SPREADS):
            r = SPREADS[kind] * rng.normal(size=S)
        elif kind == len(SPREADS):
            r = 1.0 * rng.exponential(size=S)
        else:
            r = np.log(rng.random(S) + 1e-3)
        L[i] = -r - 3.0 * rng.random()
    if n_rows <= 2:                                           # the two special rows where there is room for nothing else
        L[0] = -(1.0 * rng.exponential(size=S)) - 1.0
        if n_rows == 2:
            L[1] = -np.log(rng.random(S) + 1e-3) - 2.0
    for i in range(n_rows):
        assert len(np.unique(L[i])) == S
    return L


def device_rows(L):
    import torch
    from literate_amd import ops
    pw, tot, tail = ops.psis_loo_rows(torch.as_tensor(L, device="cuda"), return_tail=True)
    return pw.cpu().numpy(), tot.cpu().numpy(), tail.cpu().numpy()


def check_structure(ld, f64, pw, tail, M, exempt=None):
    """M, the tail's draw indices (as sets; in order too where the float64 restatement on the same bits has them), +inf
    and NaN exactly where the restatement has them"""
    n = len(pw)
    assert ld["M"] == M == tail.shape[1], (ld["M"], M, tail.shape)
    for i in range(n):
        if ld["flagged"][i]:
            assert (tail[i] == -1).all()
            continue
        if exempt is not None and exempt[i]:
            continue
        assert set(tail[i].tolist()) == set(ld["tails"][i].tolist()), (i, tail[i], ld["tails"][i])
        if exempt is None:
            assert np.array_equal(tail[i], f64["tails"][i]), (i, tail[i], f64["tails"][i])
    want_k = ld["pointwise"][:, 1].astype(np.float64)
    assert np.array_equal(np.isposinf(pw[:, 1]), np.isposinf(want_k))


def check_totals(tot, pw, ld, allowed, U):
    """the totals against the longdouble restatement: the sums to the pointwise bound summed over the rows, the standard
    error by the Lipschitz bound of a sample deviation, the counts and the maximum exactly as the device's own pointwise
    values give them"""
    want = ld["totals"]
    use = ~ld["flagged"]
    n = int(use.sum())
    assert tot[0] == want[0] == n and tot[1] == want[1] == len(pw) - n
    if n == 0:
        assert np.isnan(tot[[2, 3, 4, 5, 9]]).all() and (tot[6:9] == 0).all()
        return
    P, UU = pw[use], U[use]
    slack = 4.0 * n * EPS
    for k, cols in ((2, (0,)), (5, (2,)), (4, (0, 2))):
        bound = sum(float(np.sum(allowed[c] * UU[:, c])) for c in cols) + slack * sum(float(np.sum(np.abs(P[:, c]))) for c in cols)
        err = abs(float(tot[k]) - float(want[k]))
        say("   total %s: |error| %.3g, bound %.3g" % (loo_ref.TOTALS[k], err, bound))
        assert err <= bound, (loo_ref.TOTALS[k], tot[k], want[k], bound)
    if n >= 2:
        d = allowed[0] * UU[:, 0] + 2.0 * EPS * float(np.max(np.abs(P[:, 0])))
        bound = np.sqrt(n / (n - 1.0)) * float(np.sqrt(np.sum(d * d))) + 8.0 * n * EPS * abs(float(want[3]))
        err = abs(float(tot[3]) - float(want[3]))
        say("   total se_elpd: |error| %.3g, bound %.3g" % (err, bound))
        assert err <= bound
    else:
        assert np.isnan(tot[3])
    k = P[:, 1]
    fin = np.isfinite(k)
    assert tot[6] == np.sum(k[fin] > 0.5) and tot[7] == np.sum(k[fin] > 0.7) and tot[8] == np.sum(~fin)
    assert (tot[9] == k[fin].max()) if fin.any() else np.isnan(tot[9])


def case_rows(group):
    """ops.psis_loo_rows on host-built matrices with distinct entries: structure exactly, values within the bound"""
    from literate_amd import ops
    prepared, worst = [], np.zeros(4)
    for S in ROW_GROUPS[group]:
        for n_rows in N_ROWS:
            rng = np.random.default_rng(100 * S + n_rows)
            L = row_matrix(rng, n_rows, S)
            ld, f64 = loo_ref.psis(L, np.longdouble), loo_ref.psis(L, np.float64)
            worst = np.maximum(worst, loo_ref.error_counts(f64["pointwise"], ld))
            if S >= 1000 and n_rows == 257:                       # the heavy and the light rows are what they are meant to be
                k = ld["pointwise"][:, 1].astype(np.float64)
                assert np.isfinite(k).all() and np.median(k[5::7]) > 0.7 and np.median(k[6::7]) < 0.0
            prepared.append((S, n_rows, L, ld, f64))
    allowed = allowed_counts(worst)
    say("float64 restatement, worst counts (elpd_loo, pareto_k, lppd, n_eff): %s -> allowed on the device: %s" % (worst, allowed))
    dev_worst = np.zeros(4)
    for S, n_rows, L, ld, f64 in prepared:
        pw, tot, tail = device_rows(L)
        M = ops.loo_plan(n_rows, 10, S)[0]
        assert M == loo_ref.tail_length(S)
        check_structure(ld, f64, pw, tail, M)
        c = loo_ref.error_counts(pw, ld)
        dev_worst = np.maximum(dev_worst, c)
        k = pw[:, 1]
        say("S %d rows %d M %d: counts %s; k from %.3f to %.3f, %d unsmoothed" % (S, n_rows, M, c, np.min(k), np.max(k[np.isfinite(k)], initial=-np.inf), np.sum(np.isinf(k))))
        assert (c <= allowed).all(), (S, n_rows, c, allowed)
        assert (pw[:, 3] >= 1.0 - 1e-9).all() and (pw[:, 3] <= S * (1 + 1e-9)).all()
        check_totals(tot, pw, ld, allowed, loo_ref.value_units(ld))
    say("device, worst counts (elpd_loo, pareto_k, lppd, n_eff): %s" % dev_worst)


def case_ties():
    """rows quantised to a quarter of a nat, so that the cutoff ties with tail values and tail values tie with each other:
    the tail's draw indices in the order (r, draw index), and the values of the restatement"""
    prepared, worst = [], np.zeros(4)
    for S in (25, 100, 1000, 1025):
        rng = np.random.default_rng(5000 + S)
        L = -np.round(rng.normal(size=(9, S)) * 2.0 * 4.0) / 4.0 - 1.0
        L[7] = -np.round(rng.random(S))                        # two values only
        L[8, :] = -2.5
        L[8, S // 2] = -3.0                                     # one ratio above a constant rest: x_1 ... x_(M-1) = 0, no finite fit
        ld, f64 = loo_ref.psis(L, np.longdouble), loo_ref.psis(L, np.float64)
        assert sum(len(np.unique(L[i][ld["tails"][i]])) < ld["M"] for i in range(7)) >= 3     # ties inside the tail
        assert sum(float(ld["gap"][i]) == 0.0 for i in range(9)) >= 3                         # ties at the cutoff
        assert np.isposinf(ld["pointwise"][7, 1]) and np.isposinf(ld["pointwise"][8, 1])      # a constant tail; a fit that is not finite
        worst = np.maximum(worst, loo_ref.error_counts(f64["pointwise"], ld))
        prepared.append((S, L, ld, f64))
    allowed = allowed_counts(worst)
    say("float64 restatement %s -> allowed %s" % (worst, allowed))
    for S, L, ld, f64 in prepared:
        pw, tot, tail = device_rows(L)
        check_structure(ld, f64, pw, tail, ld["M"])
        c = loo_ref.error_counts(pw, ld)
        say("S %d: counts %s, k %s" % (S, c, pw[:, 1]))
        assert (c <= allowed).all()
        check_totals(tot, pw, ld, allowed, loo_ref.value_units(ld))


# ------------------------------------------------------------------------------------------------
# from rates
# ------------------------------------------------------------------------------------------------
def device(ts, te, lam, mu, model, br, end, offset=False, terms=False):
    """ops.loo_pointwise -> host (pointwise, totals, plan[, terms]); offset: ts / te as views one element into a longer tensor"""
    import torch
    from literate_amd import ops
    if offset:
        a = torch.as_tensor(np.concatenate(([0.0], ts)), device="cuda")[1:]
        b = torch.as_tensor(np.concatenate(([0.0], te)), device="cuda")[1:]
        assert a.data_ptr() % 16 == 8 and b.data_ptr() % 16 == 8
    else:
        a, b = torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda")
    out = ops.loo_pointwise(a, b, T0, lam, mu, model=model, br_length=br, end_time=end, return_terms=terms)
    return (out[0].cpu().numpy(), out[1].cpu().numpy(), out[2]) + ((out[3],) if terms else ())


# the lineage counts beside the 25-draw configurations (which take all four): every count meets 100 and 400 draws once
OTHER_NS = {(38, 100): (1031,), (38, 400): (257, 2), (39, 100): (257, 1), (39, 400): (1031,)}


# (model, configuration) -> the first t for which seed 3000 + k + 100 t gives no lineage over several unlived bins (see prepare_rates)
SEED_TRIES = {(0, 2): 1, (0, 3): 4, (0, 10): 3, (0, 11): 4}


def rate_configs(model):
    """one bin count from each of waic_cases.N_BINS_GROUPS' first two groups at S = 25, 100, 400 and every lineage count,
    kind of times, order and alignment; the largest accepted bin count at S = 25"""
    configs, k = [], 0
    for nb in (waic_cases.N_BINS_GROUPS["a"][1], waic_cases.N_BINS_GROUPS["b"][0]):
        for j, S in enumerate((25, 100, 400)):
            for n in (waic_cases.NS if j == 0 else OTHER_NS[(nb, S)]):
                configs.append(dict(n=n, n_bins=nb, S=S, kind=waic_cases.KINDS[k % 3], shuffled=bool(k & 1), offset=bool(k & 2),
                                    seed=3000 + k + 100 * SEED_TRIES.get((model, k), 0)))
                k += 1
    configs.append(dict(n=257, n_bins=waic_cases.largest_bins(model), S=25, kind="continuous", shuffled=True, offset=False, seed=3100))
    return configs


def prepare_rates(cfg, model):
    rng = np.random.default_rng(cfg["seed"])
    ts, te = lineages(rng, cfg["n"], cfg["n_bins"], cfg["kind"])
    if not cfg["shuffled"]:
        o = np.lexsort((te, ts))
        ts, te = ts[o], te[o]
    lam, mu = rates(rng, cfg["S"], cfg["n_bins"])
    br, end = model_inputs(rng, model, cfg["n_bins"], te)
    ld = loo_ref.loo(ts, te, T0, lam, mu, model, br, end, dtype=np.longdouble)
    f64 = loo_ref.loo(ts, te, T0, lam, mu, model, br, end, dtype=np.float64)
    assert not ld["flagged"].any() and not f64["flagged"].any()
    u = EPS * ld["A"]
    # ambiguous: the cutoff and the smallest tail value closer than 64 u_i.  A lineage whose term is EXACTLY the same under
    # every draw on the device as in the restatement has no gap at all, but nothing ambiguous either - its tail is the last
    # M draws by the index rule: it is compared exactly like the others.  That holds where birth and death read the same
    # cumulative sum (js == je: a lineage outside the window, or inside one bin nobody lived in under model 0), which then
    # cancels bit for bit.  A lineage that spans SEVERAL bins nobody lived in (model 0, R = 0 in each) is constant in the
    # restatement, whose cumulative sums are sequential, but only up to rounding on the device, whose table builder takes
    # them from a wave scan (another association per bin): it is ambiguous like any other lineage without a gap, and the
    # restatement's k = +inf cannot be asked of it.  No data set has such a lineage (whoever lives in a bin gives it a
    # branch length); model_inputs' random br_length makes them, so the seeds below are chosen on the CPU so that no
    # configuration holds one.
    js, _, je, _ = lo.lineage_bins(ts, te, T0, cfg["n_bins"])
    constant = (ld["L"].max(axis=1) == ld["L"].min(axis=1)) & (f64["L"].max(axis=1) == f64["L"].min(axis=1))
    exempt = ~(ld["gap"] > 64.0 * u) & ~(constant & (js == je))
    return ts, te, lam, mu, br, end, ld, f64, u, exempt


def case_rates(model):
    """ops.loo_pointwise against the restatement fed the same rates; then the walk's middle LDS regime (waic_cases.MIDDLE:
    one batch of all 257 lineages), with a bound of its own"""
    from literate_amd import ops
    model = int(model)
    run_rate_configs(rate_configs(model), model)
    mid = waic_cases.MIDDLE
    assert ops.loo_plan(mid["n"], mid["n_bins"], mid["S"], model)[2:] == (257, 1)
    run_rate_configs([mid], model)


def run_rate_configs(configs, model):
    from literate_amd import ops
    prepared, worst = [], np.zeros(4)
    for cfg in configs:
        ts, te, lam, mu, br, end, ld, f64, u, exempt = prepare_rates(cfg, model)
        share = float(exempt.mean())
        say("model %d %s: %d of %d lineages with an ambiguous tail" % (model, {k: cfg[k] for k in ("n", "n_bins", "S", "kind")}, exempt.sum(), cfg["n"]))
        assert share <= 0.01, (cfg, share)
        worst = np.maximum(worst, loo_ref.error_counts(f64["pointwise"], ld, u))
        prepared.append((cfg, ts, te, lam, mu, br, end, ld, f64, u, exempt))
    allowed = allowed_counts(worst)
    say("float64 restatement, worst counts (elpd_loo, pareto_k, lppd, n_eff): %s -> allowed on the device: %s" % (worst, allowed))
    dev_worst = np.zeros(4)
    for cfg, ts, te, lam, mu, br, end, ld, f64, u, exempt in prepared:
        pw, tot, plan, terms = device(ts, te, lam, mu, model, br, end, cfg["offset"], terms=True)
        assert plan[0] == ld["M"] and plan[3] == 1
        pw2, tot2, tail = ops.psis_loo_rows(terms, return_tail=True)
        assert np.array_equal(pw2.cpu().numpy(), pw, equal_nan=True) and np.array_equal(tot2.cpu().numpy(), tot, equal_nan=True)
        check_structure(ld, f64, pw, tail.cpu().numpy(), plan[0], exempt=exempt)
        # +inf where the restatement has it is part of error_counts; an exempt lineage is held to the values all the same
        c = loo_ref.error_counts(pw, ld, u)
        dev_worst = np.maximum(dev_worst, c)
        say("model %d %s plan %s: counts %s" % (model, {k: cfg[k] for k in ("n", "n_bins", "S", "kind", "shuffled", "offset")}, plan, c))
        assert (c <= allowed).all(), (cfg, c, allowed)
        check_totals(tot, pw, ld, allowed, loo_ref.value_units(ld, u))
    say("device, worst counts (elpd_loo, pareto_k, lppd, n_eff): %s" % dev_worst)


def case_exact():
    """subset, permutation, batches, repetition: identical bits; the two stages apart; lppd beside WAIC's; identical draws"""
    import torch
    from literate_amd import ops
    rng = np.random.default_rng(7)
    n, nb, S = 1031, 20, 64
    ts, te = lineages(rng, n, nb, "continuous")
    lam, mu = rates(rng, S, nb)
    for model in (0, 2, 3):
        br, end = model_inputs(np.random.default_rng(8), model, nb, te)
        assert ops.loo_plan(n, nb, S, model) == (12, 33, n, 1)
        full, tot_full, plan, terms = device(ts, te, lam, mu, model, br, end, terms=True)
        assert np.isfinite(full[:, [0, 2, 3]]).all()
        # the second stage alone on the matrix the first stage wrote
        pw2, tot2 = ops.psis_loo_rows(terms)
        assert np.array_equal(pw2.cpu().numpy(), full) and np.array_equal(tot2.cpu().numpy(), tot_full)
        # a lineage's outputs do not depend on the others, nor on the batches
        sub = np.sort(rng.choice(n, 300, replace=False))
        part, _, _ = device(ts[sub], te[sub], lam, mu, model, br, end)
        assert np.array_equal(part, full[sub])
        perm = rng.permutation(n)
        mixed, tot_mixed, _ = device(ts[perm], te[perm], lam, mu, model, br, end, offset=True)
        assert np.array_equal(mixed, full[perm])
        os.environ["LR_LOO_BATCH"] = "300"
        batched, tot_b, plan_b = device(ts, te, lam, mu, model, br, end)
        del os.environ["LR_LOO_BATCH"]
        assert plan_b[2:] == (300, 4) and np.array_equal(batched, full) and np.array_equal(tot_b, tot_full)
        again, tot_again, _ = device(ts, te, lam, mu, model, br, end)
        assert np.array_equal(again, full) and np.array_equal(tot_again, tot_full)
        # lppd beside WAIC's: both within WAIC's own bound of the longdouble restatement
        ld = waic_ref.waic(ts, te, T0, lam, mu, model, br, end, dtype=np.longdouble)
        f64 = waic_ref.waic(ts, te, T0, lam, mu, model, br, end)
        allowed = waic_cases.allowed_counts(waic_ref.error_counts(f64["pointwise"], ld))
        w_pw = ops.waic_pointwise(torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda"), T0, lam, mu, model=model,
                                  br_length=br, end_time=end)[0].cpu().numpy()
        U = waic_ref.units(ld)[:, 0]
        d_loo = np.abs(full[:, 2] - ld["pointwise"][:, 0].astype(np.float64))
        say("model %d: lppd against the restatement, worst count %.3g (WAIC's: %.3g), allowed %.3g" %
            (model, np.max(d_loo / U), np.max(np.abs(w_pw[:, 0] - ld["pointwise"][:, 0].astype(np.float64)) / U), allowed[0]))
        assert (d_loo <= allowed[0] * U).all() and (np.abs(full[:, 2] - w_pw[:, 0]) <= 2.0 * allowed[0] * U).all()
        # all draws identical
        lam1, mu1 = np.repeat(lam[:1], S, 0), np.repeat(mu[:1], S, 0)
        pw, tot, _ = device(ts, te, lam1, mu1, model, br, end)
        assert np.array_equal(pw[:, 0], pw[:, 2]) and np.isposinf(pw[:, 1]).all() and np.array_equal(pw[:, 3], np.full(n, float(S)))
        assert tot[8] == n and tot[6] == 0 and tot[7] == 0 and np.isnan(tot[9]) and tot[4] == 0.0 and tot[2] == tot[5]
        say("model %d: subset, permutation, batches, repetition and the stages apart identical" % model)


def case_flags():
    """waic_cases.case_flags' construction: exactly the k + j lineages are NaN, the counts exact, the others keep their bits"""
    rng = np.random.default_rng(37)
    nb, S, k, j, rest = 10, 30, 5, 3, 600
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
    ref = loo_ref.loo(ts, te, T0, lam_b, mu_b, 2)
    assert np.array_equal(ref["flagged"], bad)
    for batch in (None, 250):
        if batch:
            os.environ["LR_LOO_BATCH"] = str(batch)
        pw, tot, plan = device(ts, te, lam_b, mu_b, 2, None, 0.0)
        os.environ.pop("LR_LOO_BATCH", None)
        assert np.isnan(pw[bad]).all() and not np.isnan(pw[~bad]).any()
        assert tot[0] == rest and tot[1] == k + j
        assert np.array_equal(pw[~bad], good[~bad])
        elpd, kk = pw[~bad, 0], pw[~bad, 1]
        assert np.isclose(tot[2], elpd.sum(), rtol=1e-12) and np.isclose(tot[3], np.sqrt(rest * np.var(elpd, ddof=1)), rtol=1e-9)
        assert np.isclose(tot[5], pw[~bad, 2].sum(), rtol=1e-12) and np.isclose(tot[4], (pw[~bad, 2] - elpd).sum(), rtol=1e-9, atol=1e-12)
        fin = np.isfinite(kk)
        assert tot[6] == np.sum(kk[fin] > 0.5) and tot[7] == np.sum(kk[fin] > 0.7) and tot[8] == np.sum(~fin) and tot[9] == kk[fin].max()
        say("batches %d: %d flagged, %d used, the others identical" % (plan[3], tot[1], tot[0]))
    pw, tot, _ = device(ts[bad], te[bad], lam_b, mu_b, 2, None, 0.0)
    assert np.isnan(pw).all() and tot[0] == 0 and tot[1] == k + j and np.isnan(tot[[2, 3, 4, 5, 9]]).all() and (tot[6:9] == 0).all()
    # the same through the rows' entry point: a -inf and a nan
    L = ref["L"].copy()
    pw_r, tot_r, tail = device_rows(L)
    assert np.array_equal(np.isnan(pw_r).all(axis=1), bad) and tot_r[1] == k + j and (tail[bad] == -1).all() and (tail[~bad] >= 0).all()


def case_arguments():
    """every refusal of both entry points returns its code and leaves the outputs untouched"""
    import torch
    from literate_amd import _hip, ops
    lib = _hip.load()
    n, nb, S = 10, 20, 30
    ts = torch.rand(n, dtype=torch.float64, device="cuda") + T0
    te = ts + 1.0
    big = 8193
    lam = torch.rand(big, nb, dtype=torch.float64, device="cuda") + 0.1
    br = torch.ones(nb, dtype=torch.float64, device="cuda")
    pw = torch.full((n, 4), 123.0, dtype=torch.float64, device="cuda")
    tot = torch.full((10,), 123.0, dtype=torch.float64, device="cuda")
    need2 = lib.lr_loo_workspace_bytes(n, nb, S, 2)
    need = max(lib.lr_loo_workspace_bytes(n, nb, S, m) for m in (0, 2, 3))
    assert 0 < need2 <= need
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    P, E = _hip.ptr, _hip

    def call(**kw):
        a = dict(ts=P(ts), te=P(te), n=n, t0=T0, nb=nb, lam=P(lam), mu=P(lam), S=S, model=2, br=None, pw=P(pw), tot=P(tot),
                 ws=P(ws), wsb=need)
        a.update(kw)
        return _hip.launch(lib.lr_loo_pointwise, ts.device, a["ts"], a["te"], a["n"], a["t0"], a["nb"], a["lam"], a["mu"], a["S"],
                           a["model"], a["br"], 0.0, a["pw"], a["tot"], a["ws"], a["wsb"])

    for kw, code in ((dict(ts=None), E.LR_ERR_NULL), (dict(te=None), E.LR_ERR_NULL), (dict(lam=None), E.LR_ERR_NULL),
                     (dict(mu=None), E.LR_ERR_NULL), (dict(pw=None), E.LR_ERR_NULL), (dict(tot=None), E.LR_ERR_NULL),
                     (dict(ws=None), E.LR_ERR_NULL), (dict(n=0), E.LR_ERR_SIZE), (dict(n=-3), E.LR_ERR_SIZE),
                     (dict(S=1), E.LR_ERR_SIZE), (dict(S=0), E.LR_ERR_SIZE), (dict(S=big), E.LR_ERR_SIZE), (dict(nb=0), E.LR_ERR_SIZE),
                     (dict(nb=E.LR_MAX_BINS + 1), E.LR_ERR_SIZE), (dict(model=3, nb=2399), E.LR_ERR_SIZE),
                     (dict(model=1, br=P(br)), E.LR_ERR_MODEL), (dict(model=4), E.LR_ERR_MODEL), (dict(model=-1), E.LR_ERR_MODEL),
                     (dict(model=0), E.LR_ERR_MODEL), (dict(t0=T0 + 0.5), E.LR_ERR_T0), (dict(wsb=need2 - 1), E.LR_ERR_WORKSPACE),
                     (dict(wsb=0), E.LR_ERR_WORKSPACE)):
        rc = call(**kw)
        say("lr_loo_pointwise %s -> %d" % (sorted(kw), rc))
        assert rc == code, (kw, rc, code)
    L = torch.rand(n, big, dtype=torch.float64, device="cuda")
    need_r = lib.lr_psis_rows_workspace_bytes(n, S)
    assert need_r > 0

    def rows(**kw):
        a = dict(L=P(L), n=n, S=S, pw=P(pw), tot=P(tot), ws=P(ws), wsb=need_r)
        a.update(kw)
        return _hip.launch(lib.lr_psis_rows, L.device, a["L"], a["n"], a["S"], a["pw"], a["tot"], a["ws"], a["wsb"])

    for kw, code in ((dict(L=None), E.LR_ERR_NULL), (dict(pw=None), E.LR_ERR_NULL), (dict(tot=None), E.LR_ERR_NULL),
                     (dict(ws=None), E.LR_ERR_NULL), (dict(n=0), E.LR_ERR_SIZE), (dict(n=-1), E.LR_ERR_SIZE), (dict(S=1), E.LR_ERR_SIZE),
                     (dict(S=big), E.LR_ERR_SIZE), (dict(wsb=need_r - 1), E.LR_ERR_WORKSPACE), (dict(wsb=0), E.LR_ERR_WORKSPACE)):
        rc = rows(**kw)
        say("lr_psis_rows %s -> %d" % (sorted(kw), rc))
        assert rc == code, (kw, rc, code)
    assert lib.lr_psis_rows_workspace_bytes(0, S) == E.LR_ERR_SIZE and lib.lr_psis_rows_workspace_bytes(n, big) == E.LR_ERR_SIZE
    assert lib.lr_loo_workspace_bytes(n, nb, big, 2) == E.LR_ERR_SIZE and lib.lr_loo_workspace_bytes(n, nb, 1, 2) == E.LR_ERR_SIZE
    torch.cuda.synchronize()
    assert bool((pw == 123.0).all()) and bool((tot == 123.0).all())              # nothing was launched
    assert call() == 0 and call(model=0, br=P(br)) == 0 and call(model=3) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pw[:, [0, 2, 3]]).all()) and float(tot[0]) == n
    pw.fill_(123.0)
    assert rows() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pw[:, [0, 2, 3]]).all()) and float(tot[0]) == n
    for bad in (dict(model=1), dict(model=0)):
        try:
            ops.loo_pointwise(ts, te, T0, lam[:S], lam[:S], **bad)
        except ValueError as ex:
            assert "LR_ERR_MODEL" in str(ex)
        else:
            raise AssertionError(bad)
    for shape in ((n, 1), (n, big)):
        try:
            ops.psis_loo_rows(L[:, :shape[1]])
        except ValueError as ex:
            assert "LR_ERR_SIZE" in str(ex)
        else:
            raise AssertionError(shape)


# ------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------
CH, N_IT, S_FREQ, DRAWS = waic_cases.CH, waic_cases.N_IT, waic_cases.S_FREQ, waic_cases.DRAWS


def _run_cli(script, data, extra, waic_too=False):
    cmd = [sys.executable, os.path.join(ROOT, script), "-d", data, "-TBP", "-n", str(N_IT), "-s", str(S_FREQ), "-p", "1000",
           "-seed", "31", "--chains", str(CH), "--loo", "0.2", "--loo_draws", str(DRAWS)] + extra
    if waic_too:
        cmd += ["--waic", "0.2", "--waic_draws", str(DRAWS)]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_WAIC_SLICES", "LR_LOO_BATCH"):
        env.pop(k, None)
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=280, env=env).stdout
    line = [l for l in out.splitlines() if l.startswith("LOO:")]
    say(line)
    assert len(line) == 1 and "_LOO.tsv" in line[0] and "_LOO_pointwise.npz" in line[0] and "%d draws" % DRAWS in line[0]
    assert "elpd_loo" in line[0] and "p_loo" in line[0] and "lineages with k > 0.7" in line[0]
    assert len([l for l in out.splitlines() if l.startswith("WAIC:")]) == int(waic_too)


def _check_files(stem, ts, te, t0, lam, mu, model, br, end):
    """<stem>_LOO.tsv and _pointwise.npz against the restatement on the rates read back from the logs"""
    from literate_amd import loo, waic
    o = waic_cases._engine_order(ts, te)
    ts, te = ts[o], te[o]
    ld = loo_ref.loo(ts, te, t0, lam, mu, model, br, end, dtype=np.longdouble)
    f64 = loo_ref.loo(ts, te, t0, lam, mu, model, br, end)
    assert not ld["flagged"].any()
    u = EPS * ld["A"]
    allowed = allowed_counts(loo_ref.error_counts(f64["pointwise"], ld, u))
    with open(stem + "_LOO.tsv") as f:
        head, vals = [l.rstrip("\n").split("\t") for l in f]
    assert head == loo.TSV_HEAD and all("." not in vals[head.index(k)] for k in loo.TSV_INTS)
    row = dict(zip(head, [float(v) for v in vals]))
    z = np.load(stem + "_LOO_pointwise.npz")
    elpd, kk = z["elpd"], z["pareto_k"]
    n, U, want = len(ts), loo_ref.value_units(ld, u), ld["totals"]
    assert str(z["method"]) == "psis-loo"
    assert (row["draws"], row["lineages"], row["lineages_used"], row["lineages_flagged"]) == (len(lam), n, n, 0)
    assert np.array_equal(z["fingerprint"], waic.fingerprint(ts, te, t0, lam.shape[1], model)) and elpd.shape == kk.shape == (n,)
    want_pw = ld["pointwise"].astype(np.float64)
    ambiguous = ~(ld["gap"] > 64.0 * u) & ~(ld["L"].max(axis=1) == ld["L"].min(axis=1))
    say("%s: %d of %d lineages with an ambiguous tail" % (os.path.basename(stem), ambiguous.sum(), n))
    for name, got, c in (("elpd", elpd, 0), ("pareto_k", kk, 1)):
        fin = np.isfinite(want_pw[:, c])
        assert np.array_equal(np.isfinite(got), fin)
        ratio = np.abs(got[fin] - want_pw[fin, c]) / (allowed[c] * U[fin, c])
        say("%s: pointwise %s, worst |error| / bound %.3g (allowed counts %s)" % (os.path.basename(stem), name, ratio.max(initial=0.0), allowed))
        assert (ratio <= 1.0).all()
    slack = 4.0 * n * EPS
    for name, k, cols in (("elpd_loo", 2, (0,)), ("lppd", 5, (2,)), ("p_loo", 4, (0, 2))):
        bound = sum(float(np.sum(allowed[c] * U[:, c])) for c in cols) + slack * sum(float(np.sum(np.abs(want_pw[:, c]))) for c in cols)
        say("   %s %.17g, restatement %.17g, bound %.3g" % (name, row[name], float(want[k]), bound))
        assert abs(row[name] - float(want[k])) <= bound
    d = allowed[0] * U[:, 0] + 2.0 * EPS * float(np.max(np.abs(want_pw[:, 0])))
    bound = np.sqrt(n / (n - 1.0)) * float(np.sqrt(np.sum(d * d))) + 8.0 * n * EPS * float(want[3])
    assert abs(row["se_elpd"] - float(want[3])) <= bound
    assert row["looic"] == -2.0 * row["elpd_loo"] and row["se_looic"] == 2.0 * row["se_elpd"]
    fin = np.isfinite(kk)
    assert row["n_k_gt_0.7"] == np.sum(kk[fin] > 0.7) and row["n_k_gt_0.5"] == np.sum(kk[fin] > 0.5) and row["n_unsmoothed"] == np.sum(~fin)
    assert (row["max_k"] == kk[fin].max()) if fin.any() else np.isnan(row["max_k"])
    return row, elpd


def _run_lrf(tmp, data, model, waic_too=False):
    from literate_amd import logs
    _run_cli("LiteRateForward.py", data, ["-model_BDI", str(model)], waic_too)
    return logs.log_paths(data, model)[1]["div"][:-len("_div.log")]


def case_cli_lrf(model):
    """LiteRateForward.py --loo (with --waic beside it: four files) against the restatement fed the rates of the logs"""
    from literate_amd import logs, ops
    model = int(model)
    with tempfile.TemporaryDirectory() as tmp:
        data = waic_cases._data(tmp)
        stem = _run_lrf(tmp, data, model, waic_too=True)
        for suffix in ("_LOO.tsv", "_LOO_pointwise.npz", "_WAIC.tsv", "_WAIC_pointwise.npz"):
            assert os.path.exists(stem + suffix), suffix
        ts, te = waic_cases._lrf_lineages(data)
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
        drawn = waic_cases._draw_rows(per_chain)
        lam, mu = np.array([d[0] for d in drawn]), np.array([d[1] for d in drawn])
        br = ops.bin_unit_events(ts, te, t0, n_bins)[2].cpu().numpy() if model == 0 else None
        _check_files(stem, ts, te, t0, lam, mu, model, br, float(te.max()))


def case_cli_dd():
    """DDRate.py --loo under two models against the restatement; python -m literate_amd.loo ranks the two and refuses a
    LiteRateForward.py file and a WAIC file beside them"""
    from literate_amd import ops
    from literate_amd.ddrate import model_suffix
    with tempfile.TemporaryDirectory() as tmp:
        data = waic_cases._data(tmp)
        ts, te, origin, n_bins, DT = waic_cases._dd_setup(data)
        rows, files = {}, {}
        for mb, md in ((2, 2), (0, 0)):
            _run_cli("DDRate.py", data, ["-m_birth", str(mb), "-m_death", str(md)], waic_too=(mb == 0))
            stem = os.path.join(tmp, "example_31" + model_suffix(mb, md))
            par = np.array(waic_cases._log_rows(["%s_c%d.log" % (stem, c) for c in range(CH)]))[:, 6:14].copy()
            par[:, 2] -= origin                                   # the log holds x0 + ORIGIN and L + div_0
            par[:, 4] -= par[:, 3]
            lam, mu = [v.cpu().numpy() for v in ops.dd_rates(par, DT, mb, md)[:2]]
            rows[(mb, md)], _ = _check_files(stem, ts, te, origin, lam, mu, 2, None, float(te.max()))
            files[(mb, md)] = stem + "_LOO_pointwise.npz"
        cmd = [sys.executable, "-m", "literate_amd.loo", files[(2, 2)], files[(0, 0)], "-o", os.path.join(tmp, "table.tsv")]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
        say(out.stdout)
        assert out.returncode == 0, out.stderr
        lines = [l.split("\t") for l in out.stdout.splitlines()]
        assert len(lines) == 3 and lines[0] == ["model", "elpd_loo", "p_loo", "elpd_diff", "se_diff", "lineages_used", "n_k_gt_0.7"]
        assert open(os.path.join(tmp, "table.tsv")).read() == out.stdout
        best, other = lines[1], lines[2]
        e = {files[k]: np.load(files[k])["elpd"] for k in files}
        assert float(best[1]) == float(np.sum(e[best[0]])) >= float(other[1]) == float(np.sum(e[other[0]]))
        assert float(best[3]) == 0.0 and float(other[3]) == float(np.sum(e[other[0]] - e[best[0]]))
        key = {files[k]: k for k in files}
        assert float(best[2]) == rows[key[best[0]]]["p_loo"] and int(best[6]) == rows[key[best[0]]]["n_k_gt_0.7"]
        # a LiteRateForward.py file beside them: another window and model id
        lrf = _run_lrf(tmp, data, 0) + "_LOO_pointwise.npz"
        out = subprocess.run([sys.executable, "-m", "literate_amd.loo", files[(2, 2)], lrf], capture_output=True, text=True,
                             timeout=120, cwd=ROOT)
        say(out.stderr.strip())
        assert out.returncode != 0 and "fingerprint mismatch" in out.stderr and "not comparable" in out.stderr
        # the WAIC file of the same run: the same fingerprint, another method
        wfile = files[(0, 0)].replace("_LOO_", "_WAIC_")
        assert os.path.exists(wfile)
        out = subprocess.run([sys.executable, "-m", "literate_amd.loo", files[(0, 0)], wfile], capture_output=True, text=True,
                             timeout=120, cwd=ROOT)
        say(out.stderr.strip())
        assert out.returncode != 0 and "not a PSIS-LOO pointwise file" in out.stderr


def case_cli_trend():
    """trend_rate.py --loo with a synthetic covariate against the restatement on ops.trend_rates of the drawn log rows"""
    from literate_amd import ops
    from literate_amd.trendrate import model_suffix, normalise_trend
    with tempfile.TemporaryDirectory() as tmp:
        data = waic_cases._data(tmp)
        ts, te, origin, n_bins, DT = waic_cases._dd_setup(data)
        raw = 3.0 + np.sin(np.arange(n_bins + 1) / 4.0) + np.arange(n_bins + 1) / 10.0
        trend_file = os.path.join(tmp, "trend.tsv")
        with open(trend_file, "w") as f:
            f.write("year\tcovariate\n" + "".join("%d\t%r\n" % (i, float(v)) for i, v in enumerate(raw)))
        _run_cli("trend_rate.py", data, ["-trend_data", trend_file, "-trend_index", "1"])
        stem = os.path.join(tmp, "example_31" + model_suffix(False, False))
        par = np.array(waic_cases._log_rows(["%s_c%d_1.trendrate.log" % (stem, c) for c in range(CH)]))[:, 6:12]
        lam, mu = [v.cpu().numpy() for v in ops.trend_rates(par, normalise_trend(raw), False, False)]
        _check_files(stem + "_1", ts, te, origin, lam, mu, 2, None, float(te.max()))


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
