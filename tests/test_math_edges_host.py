"""The inputs, references and bounds of tests/test_hip_math_edges.py, checked with numpy alone (no GPU): that the
long-double references are what they claim (against mpmath on a subsample), that the ulp checker of part A passes a
faithful restatement of lr_log and rejects two subtly wrong ones, that the propagated bound of part B holds the
project's float64 oracle on every case and rejects a logarithm that is off by 2^-40, and that the cases reach the
floors, the overflowing and vanishing logistic and the zero bins they are there for.  Both modules import
tests/helpers/math_edges.py, so they see identical inputs."""
import numpy as np
import pytest

from helpers import math_edges as ME

KINDS = ("dd", "ddv2", "trend")


# ------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------
def test_long_double_log_and_power_against_mpmath():
    """np.log and np.power on long double against 40-digit mpmath on 1,500 of the part-A arguments and 300 (base,
    exponent) pairs of part B's ranges: within 2^-62 relative, i.e. 2^-9 ulp of fp64 - beside a bound of 1.2 ulp the
    reference's own error does not count."""
    import mpmath
    mpmath.mp.prec = 140
    x = ME.log_host_subsample()[::13]
    ref = ME.log_reference(x)
    worst = 0.0
    for xi, ri in zip(x, ref):
        exact = mpmath.log(mpmath.mpf(float(xi)))
        if exact == 0:
            assert ri == 0
            continue
        worst = max(worst, abs(float((mpmath.mpf(str(np.format_float_scientific(ri, precision=25))) - exact) / exact)))
    rng = np.random.default_rng(5)
    base = np.exp(rng.uniform(np.log(1e-8), np.log(1e8), 300))
    nu = rng.normal(0.0, 3.0, 300)
    pw = np.power(base.astype(ME.LD), nu.astype(ME.LD))
    worst_p = 0.0
    for b, n, r in zip(base, nu, pw):
        exact = mpmath.power(mpmath.mpf(float(b)), mpmath.mpf(float(n)))
        worst_p = max(worst_p, abs(float((mpmath.mpf(str(np.format_float_scientific(r, precision=25))) - exact) / exact)))
    print("long double vs mpmath: log %.2e, power %.2e relative" % (worst, worst_p))
    assert worst <= 2.0 ** -62 and worst_p <= 2.0 ** -58        # the power's exponent nu log(base) reaches 16 * 18


def test_log_arguments_are_the_sets_named():
    a = ME.log_arguments()
    assert len(a["bit patterns"]) == 1 << 20 and len(a["uniform [0.5, 2)"]) == 1 << 18
    assert len(a["rates [1e-15, 1e3]"]) == 1 << 16
    assert np.any(a["bit patterns"] < np.finfo(np.float64).tiny)               # subnormals
    exps = np.frexp(a["bit patterns"])[1]
    assert exps.min() < -1000 and exps.max() > 1000
    p2 = a["powers of two"]
    assert len(p2) == 2098 and p2[0] == 5e-324 and p2[-1] == 2.0 ** 1023
    near = a["near 1, sqrt 1/2, sqrt 2"]
    assert len(near) == 3 * 129 and near[64] == 1.0 and near[129 + 64] == ME.SQRT_HALF and near[258 + 64] == ME.SQRT_TWO
    assert np.all(np.diff(near[:129].view(np.int64)) == 1)
    for k in ME.LOG_SCALES:
        assert np.array_equal(a["near 1, sqrt 1/2, sqrt 2, times 2^%d" % k] / 2.0 ** k if abs(k) < 1000 else
                              np.ldexp(a["near 1, sqrt 1/2, sqrt 2, times 2^%d" % k], -k), near)
    assert len(a["1 +- 2^-k"]) == 104 and 1.0 + 2.0 ** -52 in a["1 +- 2^-k"] and 0.5 in a["1 +- 2^-k"]
    assert len(ME.log_probe_arguments()) <= 2 << 20
    sub = ME.log_host_subsample()
    assert 19990 <= len(sub) <= 20000 and ME.SQRT_HALF in sub


def test_log_checker_passes_the_restatement_and_rejects_two_wrong_logs():
    """The plain-numpy restatement of lr_log stays within 2.5 ulp on the 20,000-argument subsample (no fma: up to 2 ulp);
    the same restatement times 1 + 2^-50, and one whose exponent decrement switches 2^-30 above the mantissa's
    sqrt(1/2), are rejected - the second only by the arguments placed around sqrt(1/2)."""
    x = ME.log_host_subsample()
    ok, worst, at = ME.check_log(x, ME.log_emulated(x), ME.LOG_EMULATION_ULP_BOUND)
    print("restatement: %.3f ulp at %s" % (worst, at))
    assert ok, (worst, at)
    ok, worst, at = ME.check_log(x, ME.log_emulated(x, rel=1.0 + 2.0 ** -50), ME.LOG_EMULATION_ULP_BOUND)
    print("times 1 + 2^-50: %.3f ulp at %s" % (worst, at))
    assert not ok and worst < 20.0
    ok, worst, at = ME.check_log(x, ME.log_emulated(x, switch_k=ME.SQRT_HALF + 2.0 ** -30), ME.LOG_EMULATION_ULP_BOUND)
    print("switch slipped by 2^-30: %.3g ulp at %s" % (worst, at))
    assert not ok
    m = np.frexp(float.fromhex(at))[0]
    assert ME.SQRT_HALF <= m < ME.SQRT_HALF + 2.0 ** -30
    # numpy's own fp64 logarithm passes the device bound: the checker does not reject a good logarithm
    assert ME.check_log(x, np.log(x), ME.LOG_ULP_BOUND)[0]
    # and a special value in place of a number is an infinite error
    bad = np.log(x)
    bad[7] = np.nan
    assert not ME.check_log(x, bad, 1e300)[0]


# ------------------------------------------------------------------------------------------------------------------
# the rate-map cases
# ------------------------------------------------------------------------------------------------------------------
def test_case_lists_hold_the_shapes_and_models_named():
    dd = ME.dd_case_list()
    assert {(mb, md) for nb, c, mb, md in dd if (nb, c) == (129, 3)} == set(ME.DD_PAIRS) and len(ME.DD_PAIRS) == 15
    for pair in ME.SHAPE_PAIRS:
        assert {(nb, c) for nb, c, mb, md in dd if (mb, md) == pair} == {(nb, c) for nb in ME.BINS for c in ME.CHAINS}
    assert len(dd) == len(set(dd)) == 15 + 4 * 15 - 4
    tr = ME.trend_case_list()
    assert len(tr) == len(set(tr)) == 4 * 15
    assert ME.BINS == (1, 127, 128, 129, 257) and ME.CHAINS == (1, 3, 300)


@pytest.mark.parametrize("kind", KINDS)
def test_cases_stay_in_the_priors_domain(kind):
    """div_0 >= 0, L >= 0, div_0 + L > 0, DT >= 0, TREND in (0, 1], rates >= 0."""
    for key in ME.case_lists()[kind]:
        args, vec = ME.case_of(kind, *key)
        assert args.shape == (key[1], {"dd": 8, "ddv2": 9, "trend": 6}[kind]) and vec.shape == (key[0],)
        assert np.all(np.isfinite(args))
        if kind == "trend":
            assert np.all((vec > 0.0) & (vec <= 1.0)) and np.all(args[:, :2] >= 0.0)
            continue
        o = 3 if kind == "dd" else 4
        assert np.all(vec >= 0.0) and np.all(np.isfinite(vec))
        assert np.all(args[:, o] >= 0.0) and np.all(args[:, o + 1] >= 0.0) and np.all(args[:, o] + args[:, o + 1] > 0.0)
        assert np.all(args[:, 0] >= 0.0) and (kind == "ddv2" or np.all(args[:, 5] >= 0.0))
        assert np.all(vec[::7] == 0.0)


@pytest.mark.parametrize("kind", KINDS)
def test_float64_oracle_stays_within_the_bound_on_every_case(kind):
    """oracle.literate_oracle's dd_rates / ddv2_rates / trend_rates - the reference's own expressions in float64 - against
    the long-double restatement under the propagated bound, every column of every case, no exception list."""
    worst, failures = 0.0, []
    for key in ME.case_lists()[kind]:
        args, vec = ME.case_of(kind, *key)
        ref = ME.reference(kind, *key)
        got = ME.oracle_eval(kind, args, vec, key[2], key[3])
        failures += ME.describe_failures(kind, key, got, ref)
        worst = max([worst] + [ME.worst_ratio(got[n], ref[n]) for n in ("birth", "death")])
    print("%s: the float64 oracle reaches %.3f of the bound" % (kind, worst))
    assert not failures, "\n".join(failures)
    assert 0.05 < worst <= 1.0


def _off_log(x):
    with np.errstate(all="ignore"):
        return np.log(x) * (1.0 + 2.0 ** -40)


def _pow_with_off_log(x, nu):
    with np.errstate(all="ignore"):
        return np.where(nu == 0, 1.0, np.exp(nu * _off_log(x)))


@pytest.mark.parametrize("kind", KINDS)
def test_a_logarithm_off_by_2_to_minus_40_is_rejected_under_every_model(kind):
    """The kernels' own form, frac ** nu = exp(nu * log frac) in float64: with numpy's logarithm it passes every case; with
    one that is wrong by 2^-40 relative it falls outside the bound in at least one case of every (m_birth, m_death) pair
    (trend: flag pair) under which a power is taken."""
    caught, good_failures = {}, []
    for key in ME.case_lists()[kind]:
        args, vec = ME.case_of(kind, *key)
        ref = ME.reference(kind, *key)
        good = ME.to_f64(ME.EVAL[kind](args, vec, key[2], key[3], T=np.float64,
                                       powf=lambda x, nu: np.where(nu == 0, 1.0, np.exp(nu * np.log(x)))))
        good_failures += ME.describe_failures(kind, key, good, ref)
        off = ME.to_f64(ME.EVAL[kind](args, vec, key[2], key[3], T=np.float64, powf=_pow_with_off_log))
        caught[key[2:]] = caught.get(key[2:], 0) + len(ME.describe_failures(kind, key, off, ref))
    assert not good_failures, "\n".join(good_failures)
    print(kind, caught)
    for pair, n in caught.items():
        has_power = (not (pair[0] and pair[1])) if kind == "trend" else (pair[0] > 0 or pair[1] > 0)
        assert (n > 0) == has_power, (kind, pair, n)


@pytest.mark.parametrize("kind", KINDS)
def test_cases_reach_what_they_name(kind):
    """Over the kernel's case set: each floor engages in >= 1 % of the entries that have it; the logistic's exp
    overflows to inf and vanishes to 0 in fp64 (trend: the power itself does); there are zero-DT entries (trend: entries
    at the covariate's 1e-15 floor); a power is taken of fractions far from 1 and with negative exponents; and in no
    case do more than 0.5 % of a column's entries lie within their bound of 0, where either branch is accepted."""
    n_floor, n_all = {"birth": 0, "death": 0}, {"birth": 0, "death": 0}
    over = under = zero = far = neg = one = 0
    for key in ME.case_lists()[kind]:
        args, vec = ME.case_of(kind, *key)
        ref = ME.reference(kind, *key)
        for name in ("birth", "death"):
            col = ref[name]
            if col.raw is None:
                continue
            n_floor[name] += int(ME.floored(col).sum())
            n_all[name] += col.raw.size
            share = ME.either_branch(col).mean()
            assert share <= 0.005, (kind, key, name, share)
        with np.errstate(all="ignore"):
            if kind == "trend":
                if key[2] and key[3]:
                    continue
                p = np.power(vec[None, :, None], args[:, None, 4:6])
                zero += int(np.sum(vec == ME.SMALL))
                frac = vec[None, :] * np.ones((key[1], 1))
                neg += int(np.sum(args[:, 4:] < 0))
            else:
                if max(key[2], key[3]) < 1:
                    continue
                o = 1 if kind == "dd" else 2
                p = np.exp(-args[:, o:o + 1] * (np.arange(key[0], dtype=float)[None, :] - args[:, o + 1:o + 2]))
                if max(key[2], key[3]) < 2:
                    p = np.ones_like(p)
                zero += int(np.sum(vec == 0.0)) * key[1]
                frac = np.asarray(ref["niche_frac"].value, dtype=np.float64)
                neg += int(np.sum(args[:, -2:] < 0))
            over += int(np.sum(np.isinf(p)))
            under += int(np.sum(p == 0.0))
            far += int(np.sum((frac > 0) & ((frac < 1e-6) | (frac > 1e6))))
            one += int(np.sum(frac == 1.0))
    share = {n: n_floor[n] / n_all[n] for n in n_all}
    print(kind, "floored", share, "exp inf", over, "exp 0", under, "zero bins", zero, "far fractions", far,
          "negative exponents", neg, "fraction exactly 1", one)
    assert share["birth"] >= 0.01 and share["death"] >= 0.01
    assert over > 0 and under > 0 and zero > 0 and far > 0 and neg > 0 and one > 0


@pytest.mark.parametrize("kind", KINDS)
def test_zero_exponent_rows_have_the_values_numpy_gives(kind):
    """x ** 0.0 is 1.0 for every base, 0 and inf included: a zero birth exponent floors the DDRate birth rate
    (l_max - l_max) to 1e-15, a zero death exponent gives 2 m_max; the float64 oracle says the same."""
    args, vec = {"dd": ME.zero_exponent_dd, "ddv2": ME.zero_exponent_ddv2, "trend": ME.zero_exponent_trend}[kind]()
    flags = (False, False) if kind == "trend" else (1, 1)
    ref = ME.EVAL[kind](args, vec, *flags)
    assert 0.0 in vec and (kind == "trend" or np.inf in vec)
    b, d = np.asarray(ref["birth"].value, dtype=np.float64), np.asarray(ref["death"].value, dtype=np.float64)
    if kind == "dd":
        assert np.all(b[:2] == ME.SMALL) and np.all(d[0] == 1.0) and np.all(d[2] == 1.0)
    elif kind == "ddv2":
        assert np.all(b[:2] == 2.0) and np.all(d[0] == 2.0) and np.all(d[2] == 2.0)      # rate_max - (rate_max - l_f), rate_min + (l_f - rate_min)
    else:
        assert np.all(b[:2] == ME.SMALL) and np.all(d[0] == 1.25) and np.all(d[2] == 1.25)
    assert np.all(np.isfinite(b[:2])) and np.all(np.isfinite(d[[0, 2]]))
    got = ME.oracle_eval(kind, args, vec, *flags)
    assert not ME.describe_failures(kind, "zero exponents", got, ref)
    # the form the kernels had, exp(0 * log 0), is rejected
    with np.errstate(all="ignore"):
        old = ME.to_f64(ME.EVAL[kind](args, vec, *flags, T=np.float64, powf=lambda x, nu: np.exp(nu * np.log(x))))
    assert ME.describe_failures(kind, "zero exponents", old, ref)


def test_likelihood_case_holds_floors_beside_ordinary_rates():
    args, DT = ME.lik_case()
    assert args.shape == (ME.LIK_CHAINS, 8) and DT.shape == (ME.LIK_BINS,)
    ref = ME.dd_eval(args, DT, 2, 2)
    both = np.concatenate([np.asarray(ref[n].value, dtype=np.float64) for n in ("birth", "death")], axis=1)
    assert np.all(np.any(both == ME.SMALL, axis=1)) and np.all(both.max(axis=1) >= 1.0) and both.max() <= 20.0
    ts, te, n_spec, n_exti = ME.lik_data()
    assert len(ts) == ME.LIK_LINEAGES and np.any(ts == np.floor(ts)) and np.any(ts != np.floor(ts))
    assert len(n_spec) == len(n_exti) == ME.LIK_BINS
    # the long-double per-lineage sum agrees with the float64 oracle of the same sum
    from oracle import literate_oracle as lo
    lam, mu = both[0, :ME.LIK_BINS], both[0, ME.LIK_BINS:]
    total, tol = ME.lineage_reference(ts, te, ME.LIK_T0, lam, mu)
    assert abs(lo.per_lineage_loglik(ts, te, ME.LIK_T0, lam, mu, 2) - float(total)) <= tol
    assert tol < 1e-9 * abs(float(total))
