"""Cases, long-double references and error bounds for the device logarithm (csrc/lr_math.h) and the three rate maps
(lr_dd_rates, lr_ddv2_rates, lr_trend_rates in csrc/lr_stats.hip; the DD and trend arithmetic is csrc/lr_dd.h, shared
with the engines' parametric steps).  Shared by tests/test_hip_math_edges.py (the device against the references) and
tests/test_math_edges_host.py (numpy alone: that the cases reach what they name and that the bounds reject a
subtly wrong evaluation).  Everything is drawn from seeded generators: both modules see identical inputs.

Part A - the probe of lr_log.  lr_binned_keiding computes, per chain c and bin b,

    sb += lr_log(birth[c, b]) * (double) n_spec[b] - birth[c, b] * DT[b]

and returns the wave sum of sb.  With n_bins = 1, n_spec = [1] and DT = [0.0] the term of lane 0 is
lr_log(x) * 1.0 - x * 0.0.  For every finite x the product x * 0.0 is a zero, so the difference is exactly lr_log(x)
whether the compiler keeps the two roundings or contracts the expression to fma(-x, 0.0, lr_log(x) * 1.0): no rounding
takes place.  sb starts at 0.0, the other 63 lanes add nothing, and the wave sum adds 63 zeros: the output IS
lr_log(x), bit for bit (a -0.0 result would come out as +0.0; the value compares equal).  x = +inf cannot be carried:
inf * 0.0 is nan.  One call takes 2^20 chains.

Part B - the rate maps in long double, and a first-order bound on what an honest fp64 evaluation may differ by.

Part C - rate vectors for the binned and the per-lineage likelihoods that hold 1e-15 floors beside rates near 10."""
import functools

import numpy as np

LD = np.longdouble
# the references below are only references if long double carries more than fp64: the x87 format's 64-bit significand
assert np.finfo(LD).nmant >= 63, "np.longdouble is not an extended format here: no high-precision reference"

EPS = 2.0 ** -53                       # unit roundoff of fp64
SMALL = 0.000000000000001              # SMALL_NUMBER, the floor of a rate (LR_DD_SMALL)
SQRT_HALF = float.fromhex("0x1.6a09e667f3bcdp-1")      # lr_log's own switch constant
SQRT_TWO = float.fromhex("0x1.6a09e667f3bcdp+0")

# ------------------------------------------------------------------------------------------------------------------
# part A: lr_log
# ------------------------------------------------------------------------------------------------------------------
LOG_ULP_BOUND = 1.2            # lr_math.h's recorded worst case of 1.1 ulp over 2^26 arguments, plus 0.1 for arguments
#                                that sample missed and for the long-double reference's own 2^-11 ulp
LOG_EMULATION_ULP_BOUND = 2.5  # the plain-numpy restatement has no fma: up to 2 ulp on the host subsample
LOG_SCALES = (-1000, -100, -1, 1, 100, 1000)


def _neighbours(centre, half=64):
    """The 2 * half + 1 doubles centred on `centre`, one ulp apart (consecutive bit patterns)."""
    bits = np.array([centre], dtype=np.float64).view(np.int64)[0]
    return (bits + np.arange(-half, half + 1, dtype=np.int64)).view(np.float64)


@functools.lru_cache(maxsize=None)
def log_arguments():
    """dict name -> float64 array of positive finite arguments."""
    out = {}
    rng = np.random.default_rng(20260)
    # every positive finite bit pattern is equally likely: all binades, the subnormals (exponent field 0) among them
    out["bit patterns"] = rng.integers(1, 0x7ff0000000000000, 1 << 20, dtype=np.int64).view(np.float64)
    out["uniform [0.5, 2)"] = rng.uniform(0.5, 2.0, 1 << 18)
    out["rates [1e-15, 1e3]"] = np.exp(rng.uniform(np.log(1e-15), np.log(1e3), 1 << 16))
    out["powers of two"] = np.ldexp(1.0, np.arange(-1074, 1024))
    near = np.concatenate([_neighbours(c) for c in (1.0, SQRT_HALF, SQRT_TWO)])
    out["near 1, sqrt 1/2, sqrt 2"] = near
    for k in LOG_SCALES:
        out["near 1, sqrt 1/2, sqrt 2, times 2^%d" % k] = np.ldexp(near, k)          # exact: all stay normal
    k = np.arange(1, 53)
    out["1 +- 2^-k"] = np.concatenate([1.0 + np.ldexp(1.0, -k), 1.0 - np.ldexp(1.0, -k)])
    for name, x in out.items():
        assert x.dtype == np.float64 and np.all(x > 0.0) and np.all(np.isfinite(x)), name
    return out


def log_probe_arguments():
    """All of log_arguments() in one vector (2^20 + 2^18 + 2^16 + ~2^14 < 2^21: two probe calls of <= 2^20 chains)."""
    return np.concatenate(list(log_arguments().values()))


def log_host_subsample(n=20000):
    """Every structured argument plus a seeded draw from the three random sets, n in all."""
    a = log_arguments()
    fixed = np.concatenate([v for k, v in a.items() if k not in ("bit patterns", "uniform [0.5, 2)", "rates [1e-15, 1e3]")])
    rng = np.random.default_rng(20261)
    per = (n - len(fixed)) // 3
    rest = [rng.choice(a[k], per, replace=False) for k in ("bit patterns", "uniform [0.5, 2)", "rates [1e-15, 1e3]")]
    return np.concatenate([fixed] + rest)


def log_reference(x):
    return np.log(np.asarray(x, dtype=np.float64).astype(LD))


def log_ulp_errors(x, got):
    """|got - log x| in ulps of the double nearest the long-double logarithm (log 1 = 0: spacing(0) is the smallest
    subnormal, so anything but an exact 0 there is an astronomic error)."""
    ref = log_reference(x)
    ulp = np.spacing(np.abs(ref.astype(np.float64))).astype(LD)
    with np.errstate(invalid="ignore"):
        err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref) / ulp
    return np.where(np.isfinite(np.asarray(got, dtype=np.float64)), err, np.inf).astype(np.float64)


def check_log(x, got, bound):
    """(ok, worst error in ulp, its argument as a hex string)."""
    err = log_ulp_errors(x, got)
    i = int(np.argmax(err))
    return bool(err[i] <= bound), float(err[i]), float(np.asarray(x)[i]).hex()


def log_emulated(x, rel=1.0, switch_k=SQRT_HALF):
    """lr_log restated in plain numpy, operation for operation but without fused multiply-adds and with a correctly
    rounded reciprocal in place of v_rcp_f64 and its two Newton steps.  `rel` scales the result; `switch_k` is the
    threshold at which the EXPONENT is decremented (the mantissa doubles at SQRT_HALF whatever it is), so a value other
    than SQRT_HALF is a slip between the two uses of the switch: arguments between the thresholds come out wrong by
    ln 2.  (Moving both uses together by 2^-30 only hands a few mantissas to the other branch, where the polynomial is
    as good: no accuracy check can see that, and none should.)"""
    x = np.asarray(x, dtype=np.float64)
    LN2_HI, LN2_LO = float.fromhex("0x1.62e42fee00000p-1"), float.fromhex("0x1.a39ef35793c76p-33")
    P = [float.fromhex(h) for h in ("0x1.5555555555558p-1", "0x1.9999999995273p-2", "0x1.2492492dfd922p-2",
                                    "0x1.c71c62d5d7104p-3", "0x1.7462b91f3eb6bp-3", "0x1.39fdcc7eb44fcp-3",
                                    "0x1.2b5f6d341e1a9p-3")]
    m, k = np.frexp(x)
    low = m < SQRT_HALF
    kd = (k - (m < switch_k)).astype(np.float64)
    m = np.where(low, 2.0 * m, m)
    f, d = m - 1.0, m + 1.0
    s = f * (1.0 / d)
    z = s * s
    p = np.full_like(z, P[6])
    for c in P[5::-1]:
        p = p * z + c
    t = f - z * p
    tail = kd * LN2_LO - s * t
    return (kd * LN2_HI + (f + tail)) * rel


# ------------------------------------------------------------------------------------------------------------------
# part B: the rate maps
# ------------------------------------------------------------------------------------------------------------------
BINS = (1, 127, 128, 129, 257)          # the 128-thread block edge and a third block
CHAINS = (1, 3, 300)
DD_PAIRS = tuple((mb, md) for mb in (0, 1, 2) for md in (-2, -1, 0, 1, 2))
SHAPE_PAIRS = ((2, 2), (1, 2), (2, -1), (0, 0))
TREND_FLAGS = ((False, False), (False, True), (True, False), (True, True))
N_PLACED = 12                            # placed rows of a 300-chain case


def dd_case_list():
    """(n_bins, C, m_birth, m_death): every model pair at (129, 3), every shape at four pairs."""
    out = [(129, 3, mb, md) for mb, md in DD_PAIRS]
    out += [(nb, c, mb, md) for mb, md in SHAPE_PAIRS for nb in BINS for c in CHAINS if (nb, c, mb, md) not in out]
    return out


def trend_case_list():
    """(n_bins, C, const_birth, const_death): every shape under all four flag pairs."""
    return [(nb, c, cb, cd) for cb, cd in TREND_FLAGS for nb in BINS for c in CHAINS]


def _seed(*key):
    return [int(k) + 1000 for k in key]


def _exponents(rng, n):
    """A third each from N(0, 1), from U(0.01, 30) and exactly 1."""
    kind = rng.integers(0, 3, n)
    return np.where(kind == 0, rng.normal(0.0, 1.0, n), np.where(kind == 1, rng.uniform(0.01, 30.0, n), 1.0))


def _logu(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _dt(rng, n_bins):
    """log-uniform in [1e-3, 1e5], every seventh bin (0, 7, ...) exactly 0."""
    DT = _logu(rng, 1e-3, 1e5, n_bins)
    DT[::7] = 0.0
    return DT


def _logistic_params(rng, C, n_bins):
    k = rng.normal(0.0, 1.0, C) * rng.choice([1e-3, 1.0, 5.0], C)
    x0 = rng.uniform(-50.0, n_bins + 50.0, C)
    return k, x0, _logu(rng, 1e-2, 1e4, C), _logu(rng, 1e-2, 1e4, C)


# Placed bins of a case with n_bins >= 127 and 300 chains: DT there is chosen against the constant niche L + div_0 = 4
# of the placed rows (L = 3, div_0 = 1: exact in every format), or against their logistic niche, which is 1 + 3 / (1 +
# exp(-k (x - x0))) with k = 0 -> exactly 2.5.
_PLACED_DT = {1: 4.0, 2: 4.0 * (1.0 + 2.0 ** -30), 3: 4.0 * (1.0 - 2.0 ** -30), 4: 4e-300, 5: 4e300,
              8: 2.5, 9: 2.5 * (1.0 + 2.0 ** -30), 10: 2.5 * (1.0 - 2.0 ** -30)}


def _place_dt(DT):
    for b, v in _PLACED_DT.items():
        DT[b] = v
    assert DT[0] == 0.0 and DT[7] == 0.0


@functools.lru_cache(maxsize=None)
def dd_case(n_bins, C, m_birth, m_death):
    """(args [C, 8], DT [n_bins]) for lr_dd_rates: [l_max, k, x0, div_0, L, m_max, nuB, nuD]."""
    rng = np.random.default_rng(_seed(1, n_bins, C, m_birth, m_death + 2))
    k, x0, div_0, L = _logistic_params(rng, C, n_bins)
    l_max, m_max = _logu(rng, 1e-3, 10.0, C), _logu(rng, 1e-3, 10.0, C)
    # the Gamma priors of the two rates reach down to 0, where `dr <= 0 -> 1e-15` is the only way DDRate's death floor
    # can engage (m_max + m_max * frac ** nu is positive otherwise)
    m_max[rng.random(C) < 0.05] = 0.0
    args = np.stack([l_max, k, x0, div_0, L, m_max, _exponents(rng, C), _exponents(rng, C)], axis=1)
    DT = _dt(rng, n_bins)
    if C >= 300 and n_bins >= 127:
        _place_dt(DT)
        #                l_max  k    x0   div_0 L   m_max nuB    nuD
        args[0] = [2.0, 0.0, 5.0, 1.0, 3.0, 0.5, 1.0, 1.0]      # frac == 1 exactly at bin 1 (const niche) / bin 8 (logistic)
        args[1] = [2.0, 0.0, 5.0, 1.0, 3.0, 0.5, 2.5, 0.3]      # ... and 1 +- 2^-30, 1e-300, 1e300 beside it
        args[2] = [2.0, 0.0, 5.0, 1.0, 3.0, 0.5, -1.0, -1.0]    # a negative nu on a zero DT: 0 ** -1 = inf
        args[3] = [2.0, 0.0, 5.0, 1.0, 3.0, 0.0, -2.5, -0.5]    # ... and on m_max = 0: 0 * inf
        args[4] = [2.0, 12.0, 64.0, 1.0, 3.0, 0.5, 1.0, 1.0]    # exp(-k (x - x0)) from e^768 = inf down to e^-2316 = 0
        args[5] = [2.0, -5.0, 100.0, 1.0, 3.0, 0.5, 1.0, 2.0]   # ... from e^-500 up to e^780
        args[6] = [2.0, 12.0, -40.0, 0.0, 3.0, 0.5, 0.5, 1.0]   # div_0 = 0
        args[7] = [2.0, 12.0, 300.0, 1.0, 0.0, 0.5, 0.5, 1.0]   # L = 0
        args[8] = [10.0, 1e-3, 0.0, 1e4, 1e4, 10.0, 30.0, 30.0]
        args[9] = [1e-3, 1e-3, 0.0, 1e-2, 1e-2, 1e-3, 0.01, 0.01]
        args[10] = [0.0, 1.0, 60.0, 1.0, 3.0, 0.0, 1.0, 1.0]    # both rates 0
        args[11] = [2.0, 0.0, 5.0, 1.0, 3.0, 0.5, -30.0, 30.0]
    return args, DT


@functools.lru_cache(maxsize=None)
def ddv2_case(n_bins, C, m_birth, m_death):
    """(args [C, 9], DT [n_bins]) for lr_ddv2_rates: [l_f, l_mul, k, x0, div_0, L, m_mul, nuB, nuD].  The multipliers
    are log-uniform in [0.25, 8]: m_mul > 1 (three fifths of the rows) makes rate_min negative, so the death floor engages."""
    rng = np.random.default_rng(_seed(2, n_bins, C, m_birth, m_death + 2))
    k, x0, div_0, L = _logistic_params(rng, C, n_bins)
    args = np.stack([_logu(rng, 1e-3, 10.0, C), _logu(rng, 0.25, 8.0, C), k, x0, div_0, L, _logu(rng, 0.25, 8.0, C),
                     _exponents(rng, C), _exponents(rng, C)], axis=1)
    DT = _dt(rng, n_bins)
    if C >= 300 and n_bins >= 127:
        _place_dt(DT)
        #                l_f  l_mul k    x0    div_0 L  m_mul nuB   nuD
        args[0] = [2.0, 1.0, 0.0, 5.0, 1.0, 3.0, 2.0, 1.0, 1.0]
        args[1] = [2.0, 0.5, 0.0, 5.0, 1.0, 3.0, 4.0, 2.5, 0.3]
        args[2] = [2.0, 1.0, 0.0, 5.0, 1.0, 3.0, 2.0, -1.0, -1.0]
        args[3] = [2.0, 1.0, 0.0, 5.0, 1.0, 3.0, 1.0, -2.5, -0.5]     # m_mul = 1: rate_min exactly 0
        args[4] = [2.0, 1.0, 12.0, 64.0, 1.0, 3.0, 8.0, 1.0, 1.0]
        args[5] = [2.0, 1.0, -5.0, 100.0, 1.0, 3.0, 1.5, 1.0, 2.0]
        args[6] = [2.0, 1.0, 12.0, -40.0, 0.0, 3.0, 2.0, 0.5, 1.0]
        args[7] = [2.0, 1.0, 12.0, 300.0, 1.0, 0.0, 2.0, 0.5, 1.0]
        args[8] = [10.0, 8.0, 1e-3, 0.0, 1e4, 1e4, 8.0, 30.0, 30.0]
        args[9] = [1e-3, 0.25, 1e-3, 0.0, 1e-2, 1e-2, 0.25, 0.01, 0.01]
        args[10] = [2.0, 1.0, 1.0, 60.0, 1.0, 3.0, 2.0, 1.0, 1.0]
        args[11] = [2.0, 1.0, 0.0, 5.0, 1.0, 3.0, 2.0, -30.0, 30.0]
    return args, DT


@functools.lru_cache(maxsize=None)
def trend_case(n_bins, C, const_birth, const_death):
    """(args [C, 6], TREND [n_bins]) for lr_trend_rates: [l_min, m_min, alpha, beta, delta, gamma].  TREND is what
    parse_trend_data leaves: in (0, 1], the minimum replaced by 1e-15 (every seventh bin here), the maximum exactly 1."""
    rng = np.random.default_rng(_seed(3, n_bins, C, int(const_birth), int(const_death)))
    l_min, m_min = _logu(rng, 1e-3, 10.0, C), _logu(rng, 1e-3, 10.0, C)
    alpha, beta = rng.normal(0.0, 5.0, C), rng.normal(0.0, 5.0, C)          # the slopes' own prior, Normal(0, 5)
    args = np.stack([l_min, m_min, alpha, beta, _exponents(rng, C), _exponents(rng, C)], axis=1)
    TREND = rng.uniform(0.0, 1.0, n_bins)
    TREND[TREND == 0.0] = 0.5
    TREND[::7] = SMALL
    if n_bins >= 127:
        TREND[1], TREND[2], TREND[3], TREND[4] = 1.0, 1.0 - 2.0 ** -53, 1e-300, 0.5
    if C >= 300:
        #               l_min m_min alpha  beta  delta gamma
        args[0] = [1.0, 0.5, -1.0, -0.5, 1.0, 2.0]          # l_min + alpha * 1 ** delta == 0 exactly at TREND = 1
        args[1] = [1.0, 0.5, -4.0, -3.0, 0.5, 0.25]         # slopes < -l_min: floored wherever TREND is not small
        args[2] = [1.0, 0.5, -4.0, -3.0, -1.0, -0.5]        # ... everywhere, and -inf at the smallest bases
        args[3] = [1.0, 0.5, 4.0, 3.0, -30.0, 30.0]
        args[4] = [0.0, 0.0, 0.0, 0.0, 1.0, 1.0]            # 0 + 0 * x: floored, or 0 * inf = nan
        args[5] = [0.0, 0.0, 0.0, 0.0, -1.0, -30.0]
        args[6] = [1e-3, 10.0, 1e-3, -10.0, 0.01, 0.01]
    return args, TREND


# -- zero exponents -------------------------------------------------------------------------------------------------
# numpy (and C's pow) give x ** 0.0 == 1.0 for EVERY x: 0, inf and nan included.  Bases 0, 1e-300, 1, 1e300 and inf,
# through DT over the constant niche 4 / the k = 0 logistic niche 2.5 (TREND: 0, 1e-300, 0.5, 1).
ZERO_EXP_DT = np.array([0.0, 4e-300, 4.0, 2.5, 4e300, np.inf])
ZERO_EXP_TREND = np.array([0.0, 1e-300, 0.5, 1.0])


def zero_exponent_dd():
    """args [3, 8]: (nuB, nuD) = (0, 0), (0, 1.5), (-0.5, 0): birth = l_max - l_max floors to 1e-15, death = 2 m_max."""
    base = [2.0, 0.0, 5.0, 1.0, 3.0, 0.5]
    return np.array([base + [0.0, 0.0], base + [0.0, 1.5], base + [-0.5, 0.0]]), ZERO_EXP_DT.copy()


def zero_exponent_ddv2():
    base = [2.0, 1.0, 0.0, 5.0, 1.0, 3.0, 2.0]
    return np.array([base + [0.0, 0.0], base + [0.0, 1.5], base + [-0.5, 0.0]]), ZERO_EXP_DT.copy()


def zero_exponent_trend():
    base = [1.0, 0.5, -1.0, 0.75]
    return np.array([base + [0.0, 0.0], base + [0.0, 1.5], base + [-0.5, 0.0]]), ZERO_EXP_TREND.copy()


# -- the maps, generic over the number format and the power function ---------------------------------------------------
class Col:
    """One output column of a rate map: `raw` before the floor (None: no floor applies), and what the bound needs."""

    def __init__(self, value, raw=None, bound=None, rel=None):
        self.value, self.raw, self.bound, self.rel = value, raw, bound, rel


def _power_term(T, scale, frac, nu, e_frac, powf):
    """(scale * frac ** nu, first-order error bound of its fp64 evaluation, frac ** nu), see rate_bound().  A power
    beyond the fp64 range is inf, as it is in any fp64 evaluation (long double would carry 1e3000 on, and 0 * 1e3000 is
    not 0 * inf)."""
    with np.errstate(all="ignore"):
        p = powf(frac, nu)
        if T is LD:
            p = np.where(p > LD(np.finfo(np.float64).max), LD(np.inf), p)
        term = scale * p
        if T is not LD:
            return term, None, p
        lf = np.abs(np.log(frac))
        lf = np.where(np.isfinite(lf), lf, LD(0))         # frac 0 / inf: p is 0 or inf (or 1), exact in every evaluation
        a = np.abs(nu)
        e_y = a * (e_frac + LOG_ULP_BOUND * EPS * lf) + EPS * a * lf
        return term, np.abs(scale) * p * (e_y + 3 * EPS), p


def rate_bound(term_bound, rate, coef=0):
    """The propagated bound of  rate = c +- scale * frac ** nu  evaluated in fp64 the way the kernels do, to first
    order in eps = 2^-53, every quantity taken from the long-double evaluation:

      u       = -k (x - x0): two roundings, relative 2 eps, so exp(u) is off by (2 |u| + 1) eps relative with a 1-ulp exp;
      e_frac  = that (0 for the constant niche) + 4 eps: 1 + exp, L / (..), div_0 + (..), DT / niche - sums of positive
                terms, no amplification.  For lr_trend_rates the base is an input: e_frac = 0;
      e_y     = |nu| (e_frac + 1.2 eps |log frac|) + eps |nu log frac|: the relative error of frac is the absolute error
                of its logarithm, lr_log adds LOG_ULP_BOUND = 1.2 ulp of its own, the product with nu rounds once;
      frac ** nu = exp(y) is then off by e_y + eps relative, the product with `scale` and (ddv2) the rounding of `scale`
                itself add 2 eps: scale * frac ** nu * (e_y + 3 eps);
      eps |rate| for the final sum;
      the factor 2 covers the second-order terms and an exp that is 1 ulp, not 1/2 ulp.

    `scale` is the coefficient of the power: l_max, m_max, rate_max - l_f, l_f - rate_min, alpha or beta.

    `coef` is for lr_ddv2_rates alone, whose two coefficients are computed, not given: c = rate_max = l_f + l_f * l_mul
    or rate_min = l_f - l_f * m_mul carries e_c = eps (|l_f * mul| + |c|) from its product and its sum, the scale
    l_f - c (or c - l_f) carries the same error with the other sign, so the rate c -+ scale * p moves by e_c |1 - p|.
    Where rate_min cancels (m_mul near 1) or the rate does (m_mul > 1, p < 1) this is far above eps |rate|: the
    project's float64 oracle, the same expressions in the same order, misses the bound without it by up to 200 times."""
    with np.errstate(all="ignore"):
        return 2 * (term_bound + coef + EPS * np.abs(rate))


def _niche(T, model, k, x0, div_0, L, x, DT):
    """(niche, frac, e_frac) of one process: model 1 constant, 2 logistic (DD:55-59)."""
    with np.errstate(all="ignore"):
        if model == 1:
            niche = (L + div_0) * np.ones_like(x)
            e = np.zeros_like(x)
        else:
            u = -k * (x - x0)
            niche = div_0 + L / (1 + np.exp(u))
            e = (2 * np.abs(u) + 1) * EPS
        return niche, DT / niche, e + 4 * EPS


def _floor(raw):
    with np.errstate(invalid="ignore"):
        return np.where(raw <= 0, type(raw.flat[0])(SMALL), raw)


def _cast(T, args, vec):
    a = np.asarray(args, dtype=np.float64).astype(T)
    v = np.asarray(vec, dtype=np.float64).astype(T)
    return [a[:, j:j + 1] for j in range(a.shape[1])], v[None, :], np.arange(len(vec)).astype(T)[None, :]


def dd_eval(args, DT, m_birth, m_death, T=LD, powf=np.power):
    """DD:71-100 for C parameter vectors at once: dict of Col for birth, death, niche, niche_frac, each [C, n_bins]."""
    (l_max, k, x0, div_0, L, m_max, nuB, nuD), DT, x = _cast(T, args, DT)
    shape = (l_max.shape[0], DT.shape[1])
    one = np.ones(shape, dtype=T)
    niche, frac, e_frac = one, one, None
    with np.errstate(all="ignore"):
        if m_birth == 0:
            birth = Col(one * l_max)
        else:
            niche, frac, e_frac = _niche(T, m_birth, k, x0, div_0, L, x, DT)
            term, tb, _ = _power_term(T, l_max, frac, nuB, e_frac, powf)
            raw = l_max - term
            birth = Col(_floor(raw), raw, None if tb is None else rate_bound(tb, raw))
        if m_death <= 0:
            death = Col(one * m_max)
        else:
            niche, frac, e_frac = _niche(T, m_death, k, x0, div_0, L, x, DT)
            term, tb, _ = _power_term(T, m_max, frac, nuD, e_frac, powf)
            raw = m_max + term
            death = Col(_floor(raw), raw, None if tb is None else rate_bound(tb, raw))
    rel = None if e_frac is None else (e_frac + 2 * EPS) * one
    return dict(birth=birth, death=death, niche=Col(niche * one, rel=rel), niche_frac=Col(frac * one, rel=rel))


def ddv2_eval(args, DT, m_birth, m_death, T=LD, powf=np.power):
    """DDRatev2.py:55-104, as dd_eval."""
    (l_f, l_mul, k, x0, div_0, L, m_mul, nuB, nuD), DT, x = _cast(T, args, DT)
    shape = (l_f.shape[0], DT.shape[1])
    one = np.ones(shape, dtype=T)
    niche, frac, e_frac = one, one, None
    with np.errstate(all="ignore"):
        if m_birth == 0:
            birth = Col(one * l_f * l_mul, rel=EPS * one)                 # one product, rounded once
        else:
            niche, frac, e_frac = _niche(T, m_birth, k, x0, div_0, L, x, DT)
            rate_max = l_f + l_f * l_mul
            term, tb, p = _power_term(T, rate_max - l_f, frac, nuB, e_frac, powf)
            raw = rate_max - term
            e_c = EPS * (np.abs(l_f * l_mul) + np.abs(rate_max)) * np.abs(1 - p)
            birth = Col(_floor(raw), raw, None if tb is None else rate_bound(tb, raw, e_c))
        if m_death <= 0:
            death = Col(one)
        else:
            niche, frac, e_frac = _niche(T, m_death, k, x0, div_0, L, x, DT)
            rate_min = l_f - l_f * m_mul
            term, tb, p = _power_term(T, l_f - rate_min, frac, nuD, e_frac, powf)
            raw = rate_min + term
            e_c = EPS * (np.abs(l_f * m_mul) + np.abs(rate_min)) * np.abs(1 - p)
            death = Col(_floor(raw), raw, None if tb is None else rate_bound(tb, raw, e_c))
    rel = None if e_frac is None else (e_frac + 2 * EPS) * one
    return dict(birth=birth, death=death, niche=Col(niche * one, rel=rel), niche_frac=Col(frac * one, rel=rel))


def trend_eval(args, TREND, const_birth, const_death, T=LD, powf=np.power):
    """trend_rate.py:73-88, as dd_eval: birth and death only."""
    (l_min, m_min, alpha, beta, delta, gamma), t, _ = _cast(T, args, TREND)
    one = np.ones((l_min.shape[0], t.shape[1]), dtype=T)
    out = {}
    with np.errstate(all="ignore"):
        for name, const, r_min, slope, expo in (("birth", const_birth, l_min, alpha, delta),
                                                ("death", const_death, m_min, beta, gamma)):
            if const:
                out[name] = Col(one * r_min)
                continue
            term, tb, _ = _power_term(T, slope, t * one, expo, LD(0), powf)
            raw = r_min + term
            out[name] = Col(_floor(raw), raw, None if tb is None else rate_bound(tb, raw))
    return out


EVAL = dict(dd=dd_eval, ddv2=ddv2_eval, trend=trend_eval)
COLUMNS = dict(dd=("birth", "death", "niche", "niche_frac"), ddv2=("birth", "death", "niche", "niche_frac"),
               trend=("birth", "death"))


def either_branch(col):
    """Entries whose unfloored long-double value lies within its (positive) bound of 0: an honest fp64 evaluation may
    land on either side of `<= 0`.  A bound of exactly 0 means every evaluation gives exactly 0: the floor is due."""
    if col.raw is None:
        return np.zeros(col.value.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        return (np.abs(col.raw) <= col.bound) & (col.bound > 0) & np.isfinite(col.bound)


def floored(col):
    if col.raw is None:
        return np.zeros(col.value.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        return col.raw <= 0


def column_failures(got, col):
    """Boolean [C, n_bins]: where `got` (fp64) is NOT an acceptable evaluation of the long-double column `col`.

    nan must meet nan; an infinite reference, or one beyond the fp64 range, its own fp64 image exactly; a rate whose
    unfloored value is <= 0 must be exactly the floor 1e-15, unless it lies within its bound of 0, where the floor and
    the value are both right; everything else within the bound of the unfloored value."""
    got = np.asarray(got, dtype=np.float64)
    g = got.astype(LD)
    with np.errstate(all="ignore"):
        ref = col.value if col.raw is None else col.raw
        ref64 = ref.astype(np.float64)
        if col.raw is None:
            tol = LD(0) if col.rel is None else col.rel * np.abs(ref)
            ok = (got == ref64) | (np.abs(g - ref) <= tol)
        else:
            near = np.abs(g - ref) <= col.bound
            is_floor = got == SMALL
            either = either_branch(col)
            ok = np.where(either, is_floor | near,
                          np.where(ref <= 0, is_floor, near | ((got == ref64) & np.isinf(ref64))))
        ok = np.where(np.isnan(ref), np.isnan(got), ok & ~np.isnan(got))
    return ~ok


def describe_failures(kind, case, got, ref):
    """One line per column that fails, with its worst entry; [] when all agree."""
    out = []
    for name in COLUMNS[kind]:
        col = ref[name]
        bad = column_failures(got[name], col)
        if bad.any():
            c, b = [int(v[0]) for v in np.nonzero(bad)]
            r = col.value if col.raw is None else col.raw
            out.append("%s %s %s: %d of %d entries, first at chain %d bin %d: got %r, reference %r (unfloored), bound %r"
                       % (kind, case, name, bad.sum(), bad.size, c, b, float(np.asarray(got[name])[c, b]),
                          float(r[c, b]), None if col.bound is None else float(col.bound[c, b])))
    return out


def worst_ratio(got, col):
    """max |got - reference| / bound over the entries that are compared by the bound (diagnostic)."""
    if col.raw is None:
        return 0.0
    with np.errstate(all="ignore"):
        g = np.asarray(got, dtype=np.float64).astype(LD)
        use = (col.raw > 0) & ~either_branch(col) & np.isfinite(col.raw) & (col.bound > 0) & np.isfinite(g)
        r = np.where(use, np.abs(g - col.raw) / np.where(use, col.bound, 1), 0)
    return float(np.max(r)) if r.size else 0.0


def oracle_eval(kind, args, vec, ma, mb):
    """The project's float64 oracle, row by row, as a dict of [C, n_bins] arrays."""
    from oracle import literate_oracle as lo
    rows = []
    with np.errstate(all="ignore"):
        for a in np.asarray(args):
            if kind == "trend":
                rows.append(lo.trend_rates(a, np.asarray(vec), ma, mb))
            else:
                f = lo.dd_rates if kind == "dd" else lo.ddv2_rates
                rows.append(f(a, np.asarray(vec), np.arange(len(vec), dtype=float), ma, mb))
    return {name: np.stack([r[i] for r in rows]) for i, name in enumerate(COLUMNS[kind])}


def to_f64(ev):
    return {k: np.asarray(c.value, dtype=np.float64) for k, c in ev.items()}


def case_of(kind, *key):
    return dict(dd=dd_case, ddv2=ddv2_case, trend=trend_case)[kind](*key)


def case_lists():
    return dict(dd=dd_case_list(), ddv2=dd_case_list(), trend=trend_case_list())


@functools.lru_cache(maxsize=None)
def reference(kind, *key):
    """The long-double evaluation of one case, computed once and shared (treat as read-only)."""
    args, vec = case_of(kind, *key)
    return EVAL[kind](args, vec, key[2], key[3])


# ------------------------------------------------------------------------------------------------------------------
# part C: likelihoods on rate vectors that come out of the maps
# ------------------------------------------------------------------------------------------------------------------
LIK_BINS, LIK_LINEAGES, LIK_CHAINS, LIK_T0 = 129, 4099, 5, 3.0


@functools.lru_cache(maxsize=None)
def lik_case():
    """(args [5, 8], DT [129]) for lr_dd_rates under (2, 2): the first five random rows of the (129, 300) DDRate case whose
    rates over the (129, 3) case's DT (zeros and values up to 1e5, none of the placed extremes) are all finite, reach
    above 1 but not above 20, and hold at least one floored entry - 1e-15 beside ordinary rates in one table."""
    args = dd_case(LIK_BINS, 300, 2, 2)[0][N_PLACED:]
    DT = dd_case(LIK_BINS, 3, 2, 2)[1]
    ref = dd_eval(args, DT, 2, 2)
    both = np.concatenate([np.asarray(ref[n].value, dtype=np.float64) for n in ("birth", "death")], axis=1)
    ok = np.all(np.isfinite(both), axis=1) & (both.max(axis=1) <= 20.0) & (both.max(axis=1) >= 1.0) & \
        np.any(both == SMALL, axis=1) & ~np.any(either_branch(ref["birth"]) | either_branch(ref["death"]), axis=1)
    rows = np.nonzero(ok)[0][:LIK_CHAINS]
    assert len(rows) == LIK_CHAINS
    return args[rows].copy(), DT.copy()


@functools.lru_cache(maxsize=None)
def lik_data():
    """(ts, te, n_spec, n_exti): 4,099 lineages over the 129 unit bins from t0 = 3, integer and non-integer times (as
    test_hip_parity.py::test_loglik_random_float_data_vs_oracle), and event counts per bin for the binned form."""
    rng = np.random.default_rng(4099)
    n, nb, t0 = LIK_LINEAGES, LIK_BINS, LIK_T0
    ts = rng.uniform(t0 - 2, t0 + nb + 1, n)
    te = ts + rng.exponential(nb / 6.0, n)
    te[rng.random(n) < 0.2] = t0 + nb + 0.5
    k = rng.integers(0, n, n // 20)
    ts[k], te[k] = np.floor(ts[k]), np.ceil(te[k])
    return ts, te, rng.integers(0, 2000, nb), rng.integers(0, 2000, nb)


def keiding_reference(birth, death, n_spec, n_exti, DT):
    """(birth_lik, death_lik, tol_birth, tol_death), each [C], in long double; tol = 64 ulp of the sum of |terms|."""
    out = []
    DT = np.asarray(DT, dtype=np.float64).astype(LD)
    for r, n in ((birth, n_spec), (death, n_exti)):
        r = np.asarray(r, dtype=np.float64).astype(LD)
        a, b = np.log(r) * np.asarray(n).astype(LD), r * DT
        out.append(((a - b).sum(axis=1), 64 * 2.0 ** -52 * (np.abs(a) + np.abs(b)).sum(axis=1)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def lineage_reference(ts, te, t0, lam, mu):
    """(log-likelihood, tolerance) of ONE chain under model 2, the per-lineage sum in long double: the gather form of
    oracle.literate_oracle.per_lineage_loglik with its own exact bin indices and in-bin fractions.  Tolerance in the
    form of tests/test_hip_edges.py::_fixed_point_bound, second term: 64 ulp of the sum of |terms|."""
    from oracle import literate_oracle as lo
    lam, mu = np.asarray(lam, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    n_bins = len(lam)
    js, fs, je, fe = lo.lineage_bins(ts, te, t0, n_bins)
    L, M = lam.astype(LD), mu.astype(LD)
    R = L + M
    cum = np.concatenate(([LD(0)], np.cumsum(R)))
    SA = np.concatenate(([LD(0)], np.log(L) + cum[:-1], [cum[-1]]))
    SR = np.concatenate(([LD(0)], R, [LD(0)]))
    EA = np.concatenate(([LD(0)], np.log(M) - cum[:-1], [-cum[-1]]))
    total = np.sum(SA[js] + fs.astype(LD) * SR[js] + EA[je] - fe.astype(LD) * SR[je])
    Rmax, csum = float(np.max(lam + mu)), float(np.sum(lam + mu))
    terms = len(ts) * (np.max(np.abs(np.log(np.concatenate([lam, mu])))) + 2 * csum + 2 * Rmax + 10.0)
    return total, 64 * 2.0 ** -52 * terms
