"""The device logarithm and the rate-map kernels at their edges.

  part A  lr_log (csrc/lr_math.h), probed bit-exactly through lr_binned_keiding over 1.4 million arguments - every binade
          and the subnormals, the neighbourhoods of 1, sqrt(1/2) (the kernel's own switch) and sqrt 2 at seven scales,
          every power of two - against the long-double logarithm in ulps;
  part B  lr_dd_rates, lr_ddv2_rates and lr_trend_rates against the long-double restatement of DD:71-100,
          DDRatev2.py:55-104 and trend_rate.py:73-88 under a propagated first-order bound, across the 128-thread block
          edge, at one bin and ragged chain counts, under every model pair, with the floors, an overflowing and a
          vanishing logistic, zero bins, fractions far from 1, negative and ZERO exponents;
  part C  lr_binned_keiding and lr_bd_loglik_batch on rate vectors out of part B's maps (1e-15 floors beside rates near
          10), and the argument errors of the three maps.

The cases, references and bounds come from tests/helpers/math_edges.py; tests/test_math_edges_host.py proves with numpy
alone that they mean something.  No case is skipped."""
import numpy as np
import pytest

from helpers import math_edges as ME

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: no ROCm device visible")
    from literate_amd import ops as _ops
    return _ops


def _np(x):
    return x.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------
# part A
# ------------------------------------------------------------------------------------------------------------------
def _lr_log(ops, x):
    """lr_log(x) bit for bit: one chain per argument, one bin, one event, no exposure (the argument why this is exact is
    in helpers/math_edges.py).  +inf cannot be probed this way - inf * 0.0 is nan - and is left alone."""
    x = np.asarray(x, dtype=np.float64)
    out = []
    for a in range(0, len(x), 1 << 20):
        part = x[a:a + (1 << 20), None]
        out.append(_np(ops.binned_keiding(part, np.ones_like(part), [1], [1], [0.0])[0]))
    return np.concatenate(out)


def test_lr_log_special_values(ops):
    """log 1 is exactly 0; +0 and -0 give -inf; negative arguments (the largest and the smallest among them) and nan
    give nan; the probe itself turns 1 into the other column's log 1 = 0."""
    x = np.array([1.0, 0.0, -0.0, -1.0, -5e-324, -1.7976931348623157e308, -np.inf, np.nan, 2.0, 0.5])
    got = _lr_log(ops, x)
    assert got[0] == 0.0
    assert got[1] == -np.inf and got[2] == -np.inf
    assert np.all(np.isnan(got[3:8])), got[3:8]
    assert got[8] == -got[9] and abs(got[8] - np.log(2.0)) <= np.spacing(np.log(2.0))


def test_lr_log_within_1p2_ulp_of_the_long_double_logarithm(ops):
    """Every argument set of helpers/math_edges.log_arguments(): the error in ulps of the double nearest the long-double
    logarithm is at most 1.2 (csrc/lr_math.h records the measured maximum, 0.8921 ulp at 0x1.681b7b548f6a1p-1).  What
    this can see: with P0 changed by 2^-45 relative (its third hex digit from the end) the maximum is 3.4 ulp and the test
    fails; a change in P0's LAST hex digit moves no result by more than 0.01 ulp, which no bound in ulps can tell from the
    logarithm as it is - and need not."""
    sets = ME.log_arguments()
    x = ME.log_probe_arguments()
    got = _lr_log(ops, x)
    a = 0
    for name, v in sets.items():
        ok, worst, at = ME.check_log(v, got[a:a + len(v)], ME.LOG_ULP_BOUND)
        print("lr_log, %-45s %8d arguments: %.4f ulp at %s" % (name + ":", len(v), worst, at))
        a += len(v)
    ok, worst, at = ME.check_log(x, got, ME.LOG_ULP_BOUND)
    print("lr_log: maximum error %.4f ulp at x = %s over %d arguments" % (worst, at, len(x)))
    assert ok, "lr_log is off by %.4f ulp at x = %s (bound %.1f)" % (worst, at, ME.LOG_ULP_BOUND)


# ------------------------------------------------------------------------------------------------------------------
# part B
# ------------------------------------------------------------------------------------------------------------------
def _run(ops, kind, args, vec, ma, mb):
    f = dict(dd=ops.dd_rates, ddv2=ops.ddv2_rates, trend=ops.trend_rates)[kind]
    return dict(zip(ME.COLUMNS[kind], [_np(o) for o in f(args, vec, ma, mb)]))


def _models(kind):
    seen = []
    for key in ME.case_lists()[kind]:
        if key[2:] not in seen:
            seen.append(key[2:])
    return [pytest.param(kind, m[0], m[1], id="%s-%d-%d" % (kind, m[0], m[1])) for m in seen]


@pytest.mark.parametrize("kind,ma,mb", _models("dd") + _models("ddv2") + _models("trend"))
def test_rate_maps_against_long_double(ops, kind, ma, mb):
    """Every shape of the model pair (trend: flag pair): birth, death, niche and niche_frac within the propagated bound of
    the long-double evaluation (helpers/math_edges.rate_bound), nan and inf agreeing in kind and position, the 1e-15
    floor exactly where the unfloored value is <= 0 (either branch only within the bound of 0)."""
    failures, worst, n = [], 0.0, 0
    for key in ME.case_lists()[kind]:
        if key[2:] != (ma, mb):
            continue
        args, vec = ME.case_of(kind, *key)
        ref = ME.reference(kind, *key)
        got = _run(ops, kind, args, vec, ma, mb)
        for name in ME.COLUMNS[kind]:
            assert got[name].shape == (key[1], key[0])
        failures += ME.describe_failures(kind, key, got, ref)
        worst = max([worst] + [ME.worst_ratio(got[c], ref[c]) for c in ("birth", "death")])
        n += 1
    print("%s (%d, %d): %d cases, worst error %.3f of the bound" % (kind, ma, mb, n, worst))
    assert n >= 1 and not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ("dd", "ddv2", "trend"))
def test_zero_exponents_give_one(ops, kind):
    """x ** 0.0 == 1.0 for every base, as in numpy: bases 0, 1e-300, 1, 1e300 and inf (trend: 0, 1e-300, 0.5, 1) under
    exponents (0, 0), (0, 1.5) and (-0.5, 0), every niche model."""
    args, vec = {"dd": ME.zero_exponent_dd, "ddv2": ME.zero_exponent_ddv2, "trend": ME.zero_exponent_trend}[kind]()
    models = [(False, False), (False, True), (True, False)]
    if kind != "trend":
        models = [(1, 1), (2, 2), (1, 2), (2, 1), (0, 2), (1, -1)]
    failures = []
    for ma, mb in models:
        ref = ME.EVAL[kind](args, vec, ma, mb)
        got = _run(ops, kind, args, vec, ma, mb)
        failures += ME.describe_failures(kind, ("zero exponents", ma, mb), got, ref)
        if kind == "dd" and ma > 0:
            assert np.all(got["birth"][:2] == ME.SMALL), got["birth"][:2]
        if kind == "dd" and mb > 0:
            assert np.all(got["death"][[0, 2]] == 1.0), got["death"][[0, 2]]
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------------
# part C
# ------------------------------------------------------------------------------------------------------------------
def test_likelihoods_on_floored_rates(ops):
    """lr_binned_keiding and lr_bd_loglik_batch (model 2) on five DDRate rate vectors over 129 bins that hold 1e-15 beside
    rates above 1, 4,099 lineages with integer and non-integer times: against the long-double sums of the very rates the
    device produced, within 64 ulp of the sum of |terms|."""
    args, DT = ME.lik_case()
    ts, te, n_spec, n_exti = ME.lik_data()
    birth, death = [_np(o) for o in ops.dd_rates(args, DT, 2, 2)[:2]]
    both = np.concatenate([birth, death], axis=1)
    assert np.all(np.isfinite(both)) and np.all(np.any(both == ME.SMALL, axis=1)) and np.all(both.max(axis=1) >= 1.0)
    ob, od = [_np(o) for o in ops.binned_keiding(birth, death, n_spec, n_exti, DT)]
    rb, rd, tb, td = ME.keiding_reference(birth, death, n_spec, n_exti, DT)
    for c in range(ME.LIK_CHAINS):
        print("chain %d: binned birth %.3e / death %.3e of the tolerance" %
              (c, abs(ob[c] - rb[c]) / tb[c], abs(od[c] - rd[c]) / td[c]))
        assert abs(ob[c] - rb[c]) <= tb[c] and abs(od[c] - rd[c]) <= td[c], (c, ob[c], rb[c], od[c], rd[c])
    lik = _np(ops.bd_loglik_batch(ts, te, ME.LIK_T0, birth, death, 2))
    for c in range(ME.LIK_CHAINS):
        ref, tol = ME.lineage_reference(ts, te, ME.LIK_T0, birth[c], death[c])
        print("chain %d: per-lineage %.6f, off by %.3e (tolerance %.3e)" % (c, lik[c], abs(lik[c] - ref), tol))
        assert abs(lik[c] - ref) <= tol, (c, lik[c], ref, tol)


def test_rate_map_argument_errors(ops):
    """m_birth = 3 and m_death = -3 are LR_ERR_MODEL; a wrong parameter count raises before anything is launched;
    65,536 chains are LR_ERR_SIZE and 65,535 run."""
    DT = np.array([2.0])
    for f, npar in ((ops.dd_rates, 8), (ops.ddv2_rates, 9)):
        a = np.ones((2, npar))
        with pytest.raises(ValueError, match="LR_ERR_MODEL"):
            f(a, DT, 3, 2)
        with pytest.raises(ValueError, match="LR_ERR_MODEL"):
            f(a, DT, 2, -3)
        f(a, DT, 2, -2), f(a, DT, 0, 2)
    for f, npar in ((ops.dd_rates, 8), (ops.ddv2_rates, 9), (ops.trend_rates, 6)):
        for wrong in (npar - 1, npar + 1):
            with pytest.raises(ValueError, match="parameters"):
                f(np.ones((2, wrong)), DT)
        with pytest.raises(ValueError, match="LR_ERR_SIZE"):
            f(np.ones((65536, npar)), DT)
    rng = np.random.default_rng(65535)
    for kind, f in (("dd", ops.dd_rates), ("ddv2", ops.ddv2_rates), ("trend", ops.trend_rates)):
        args = ME.case_of(kind, 1, 300, *((False, False) if kind == "trend" else (2, 2)))[0]
        args = args[rng.integers(0, 300, 65535)]
        vec = np.array([0.75])
        flags = (False, False) if kind == "trend" else (2, 2)
        got = dict(zip(ME.COLUMNS[kind], [_np(o) for o in f(args, vec, *flags)]))
        assert got["birth"].shape == (65535, 1)
        assert not ME.describe_failures(kind, "65535 chains", got, ME.EVAL[kind](args, vec, *flags))
