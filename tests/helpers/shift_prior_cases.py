"""The GPU cases of tests/test_hip_shift_prior.py, each run in a child process of its own (under the test's time limit):

    python tests/helpers/shift_prior_cases.py CASE

A case prints its figures, asserts, and exits 0 - or raises.  Yardstick: tests/helpers/shift_prior_ref.py, the numpy
restatement of lr_shift_prior on the same Philox draws; every comparison is np.array_equal on integers."""
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers.shift_prior_ref import shift_prior_ref  # noqa: E402

SEED_HIGH = 0x9E3779B97F4A7C15
NAMES = ("totals", "shift_hist", "k_drawn", "k_accepted")


def header_int(name):
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, f.read()).group(1))


def device(a, b, n_reps, seed=0, poi_lambda=None, rep0=0, out=None):
    from literate_amd import ops
    res = ops.shift_prior(a, b, n_reps=n_reps, seed=seed, poi_lambda=poi_lambda, rep0=rep0, out=out)
    return res, [t.cpu().numpy() for t in res]


def same(what, got, want):
    ok = all(np.array_equal(g, w) and g.shape == w.shape for g, w in zip(got, want))
    print("%s: %s" % (what, "identical" if ok else "DIFFER"))
    sys.stdout.flush()
    if not ok:
        for name, g, w in zip(NAMES, got, want):
            bad = np.nonzero(np.asarray(g) != np.asarray(w))[0] if g.shape == w.shape else "shape"
            print(" ", name, "differs at", bad, np.asarray(g)[bad] if g.shape == w.shape else g.shape,
                  np.asarray(w)[bad] if g.shape == w.shape else w.shape)
    assert ok, what


def against_ref(what, a, b, n_reps, seed=0, poi_lambda=None, rep0=0):
    _, got = device(a, b, n_reps, seed, poi_lambda, rep0)
    want = shift_prior_ref(a, b, rep0, n_reps, seed, poi_lambda)
    print("%s: accepted %d of %d, shifts in bins %d of %d, capped %d, largest K %d" % (
        what, want.totals[0], n_reps, want.totals[1], want.totals[3], want.totals[2], want.K.max()))
    same(what, got, want[:4])
    return got, want


def case_spans():
    got, want = against_ref("(1960, 2010.5)", 1960.0, 2010.5, 1 << 16, seed=11)
    assert len(got[1]) == 50 and 0.85 < got[0][0] / (1 << 16) < 0.875       # the reference's loop accepts 0.863
    got, _ = against_ref("(-35.25, 12.5)", -35.25, 12.5, 1 << 16, seed=12)
    assert len(got[1]) == 47
    # two bins: the smallest span that can accept a shift (x in [1, 1.5] only)
    got, want = against_ref("(0, 2.5)", 0.0, 2.5, 1 << 16, seed=13)
    assert len(got[1]) == 2 and got[1][0] == 0 and got[1][1] > 0 and not got[3][2:].any() and got[3][1] == got[1][1]
    # one bin: every point of [-1, 2.5) is within 1 of an end, nothing with K > 1 is accepted
    got, want = against_ref("(0, 1.5)", 0.0, 1.5, 1 << 16, seed=14)
    assert len(got[1]) == 1 and got[1][0] == 0 and got[0][0] == got[3][0] == got[2][0] and not got[3][1:].any()
    assert got[0][1] == 0 and got[0][3] == 0


def case_most_bins():
    nb = header_int("LR_MAX_BINS")
    got, want = against_ref("n_bins = %d" % nb, 0.0, nb + 0.5, 1 << 14, seed=21)
    assert len(got[1]) == nb == 4094
    assert got[0][1] == got[1].sum() > 0


def case_counts():
    blocks = header_int("LR_SHIFT_PRIOR_BLOCKS")
    one_pass = blocks * 256
    beyond = one_pass + 4321                                   # some threads take a second replicate, most do not
    assert beyond <= 1 << 18
    for n in (1, 63, 65537, beyond):
        against_ref("n_reps = %d" % n, 1960.0, 2010.5, n, seed=31)
    print("one grid pass holds %d replicates" % one_pass)


def case_seed_and_range():
    against_ref("seed with high bits", 1960.0, 2010.5, 1 << 15, seed=SEED_HIGH)
    _, lo = device(1960.0, 2010.5, 1 << 15, seed=SEED_HIGH & 0xFFFFFFFF)
    _, hi = device(1960.0, 2010.5, 1 << 15, seed=SEED_HIGH)
    assert not np.array_equal(lo[1], hi[1])                    # the high word is part of the key
    against_ref("replicates across 2^32", 1960.0, 2010.5, 1000, seed=5, rep0=(1 << 32) - 100)
    _, low = device(1960.0, 2010.5, 1000, seed=5, rep0=0)
    _, wrap = device(1960.0, 2010.5, 1000, seed=5, rep0=(1 << 32) - 100)
    assert not np.array_equal(low[2][:4], wrap[2][:4]) or not np.array_equal(low[1], wrap[1])


def case_additivity():
    a, b, seed, rep0, n1, n2 = 1960.0, 2010.5, 41, 12345, 70001, 50000
    _, whole = device(a, b, n1 + n2, seed, rep0=rep0)
    res, first = device(a, b, n1, seed, rep0=rep0)
    res2, both = device(a, b, n2, seed, rep0=rep0 + n1, out=res)
    assert res2 is res
    same("counts(rep0, n1 + n2) = counts(rep0, n1) + counts(rep0 + n1, n2)", both, whole)
    _, second = device(a, b, n2, seed, rep0=rep0 + n1)
    same("the second range alone", [f + s for f, s in zip(first, second)], whole)
    want = shift_prior_ref(a, b, rep0, n1 + n2, seed)
    same("the whole against the restatement", whole, want[:4])


def case_fixed_lambda():
    got, want = against_ref("lambda = 0.5", 1960.0, 2010.5, 1 << 16, seed=51, poi_lambda=0.5)
    assert got[0][2] == 0 and got[2][0] > 0.7 * (1 << 16)      # P(K = 1) = 0.5 e^-0.5 / (1 - e^-0.5) = 0.771
    # lambda = 80: K is around 80, the cap at 64 stops most replicates; 63 shift times do not fit 52.5 time units
    got, want = against_ref("lambda = 80 on (1960, 2010.5)", 1960.0, 2010.5, 1 << 14, seed=52, poi_lambda=80.0)
    kcap = header_int("LR_SHIFT_PRIOR_KCAP")
    assert got[0][2] > 0.9 * (1 << 14) and got[2][kcap - 1] >= got[0][2] and got[0][0] == 0
    got, want = against_ref("lambda = 80 on (0, 4000.5)", 0.0, 4000.5, 1 << 12, seed=53, poi_lambda=80.0)
    assert got[0][2] > 0.9 * (1 << 12) and got[0][0] > 0 and got[3][kcap - 1] > 0      # capped replicates are accepted too


def case_repeatable():
    _, x = device(1960.0, 2010.5, 1 << 17, seed=61)
    _, y = device(1960.0, 2010.5, 1 << 17, seed=61)
    same("two launches of the same arguments", x, y)
    assert x[0][0] > 0


def case_arguments():
    import torch
    from literate_amd import _hip, ops
    lib = _hip.load()
    P = _hip.ptr
    kcap = _hip.LR_SHIFT_PRIOR_KCAP
    tot = torch.zeros(4, dtype=torch.int64, device="cuda")
    hist = torch.zeros(50, dtype=torch.int64, device="cuda")
    kd = torch.zeros(kcap, dtype=torch.int64, device="cuda")
    ka = torch.zeros(kcap, dtype=torch.int64, device="cuda")

    def call(a=1960.0, b=2010.5, rep0=0, n=1000, seed=1, lam=0.0, acc=0, totals=tot, shift_hist=hist, k_drawn=kd, k_accepted=ka):
        return lib.lr_shift_prior(a, b, rep0, n, seed, lam, acc, P(totals), P(shift_hist), P(k_drawn), P(k_accepted), None)

    for kw in (dict(totals=None), dict(shift_hist=None), dict(k_drawn=None), dict(k_accepted=None)):
        assert call(**kw) == _hip.LR_ERR_NULL, kw
    bad = (dict(b=1960.5), dict(b=1961.0), dict(b=1960.0), dict(b=1950.0),      # n_bins < 1
           dict(b=1962.0),                                                      # ceil(b - a) - 1 != int(b - a)
           dict(a=0.0, b=_hip.LR_MAX_BINS + 1.5), dict(a=0.0, b=1e9),           # n_bins > LR_MAX_BINS
           dict(b=float("nan")), dict(a=float("-inf")),
           dict(n=0), dict(n=-3), dict(n=(1 << 40) + 1), dict(rep0=-1),
           dict(lam=700.5), dict(lam=float("nan")), dict(lam=float("inf")))
    for kw in bad:
        assert call(**kw) == _hip.LR_ERR_SIZE, kw
    torch.cuda.synchronize()
    assert not tot.any() and not hist.any() and not kd.any() and not ka.any()      # nothing was launched
    assert call(lam=700.0, n=64) == 0 and call(lam=-1.0) == 0 and call(lam=float("-inf")) == 0      # <= 0: the hyper-prior
    torch.cuda.synchronize()
    assert int(kd.sum()) == 1000 and int(tot[0]) == int(ka.sum())
    # the wrapper: errors as ValueError, an `out` of another span refused
    for kw in (dict(n_reps=0), dict(rep0=-1), dict(poi_lambda=701.0)):
        try:
            ops.shift_prior(1960.0, 2010.5, **dict(dict(n_reps=10), **kw))
        except ValueError as ex:
            assert "LR_ERR_SIZE" in str(ex)
        else:
            raise AssertionError(kw)
    try:
        ops.shift_prior(1960.0, 1960.5, n_reps=10)
    except ValueError as ex:
        assert "LR_ERR_SIZE" in str(ex)
    else:
        raise AssertionError("span below one bin")
    res = ops.shift_prior(1960.0, 2010.5, n_reps=10)
    assert [tuple(t.shape) for t in res] == [(4,), (50,), (kcap,), (kcap,)] and res.totals.dtype == torch.int64
    try:
        ops.shift_prior(0.0, 12.5, n_reps=10, out=res)
    except ValueError as ex:
        assert "same span" in str(ex)
    else:
        raise AssertionError("out of another span")


def _synthetic_data(path):
    """80 lineages over 1960 .. 1990 whose birth rate drops after 1975"""
    rng = np.random.default_rng(8)
    ts = np.concatenate([np.full(3, 1960), rng.integers(1960, 1975, 57), rng.integers(1975, 1988, 20)])
    te = np.minimum(ts + rng.integers(1, 12, len(ts)), 1990)
    with open(path, "w") as f:
        f.write("id\tts\tte\n")
        for i, (s, e) in enumerate(zip(ts, te)):
            f.write("%d\t%d\t%d\n" % (i, s, e))
    return float(ts.min()), float(te.max()) + 0.5          # the run's span: -death_jitter 0.5 is added to te


def case_cli(tmp):
    from literate_amd import logs, shift_bf
    data = os.path.join(tmp, "tiny.tsv")
    a, b = _synthetic_data(data)
    env = dict(os.environ, LR_SHARED_DEVICE="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    base = [sys.executable, os.path.join(ROOT, "LiteRateForward.py"), "-d", data, "-n", "2000", "-s", "20", "-p", "1000",
            "-seed", "9", "--chains", "4", "--rtt", "0.2"]
    subprocess.run(base + ["-out", "_plain"], check=True, stdout=subprocess.DEVNULL, timeout=240, env=env)
    out = subprocess.run(base + ["-out", "_bf", "--rtt_bf", "65536"], check=True, capture_output=True, text=True,
                         timeout=240, env=env)
    assert "Bayes factors for rate shifts" in out.stdout
    logdir = os.path.join(tmp, "literate_mcmc_logs")
    stem = os.path.join(logdir, "tiny_BD_bf")
    for suffix in ("_RTT.tsv", "_RTT_K.tsv"):
        plain = open(os.path.join(logdir, "tiny_BD_plain" + suffix), "rb").read()
        assert len(plain) > 200 and open(stem + suffix, "rb").read() == plain, suffix
    for suffix in ("_RTT_BF.tsv", "_RTT_BF_prior.tsv", "_RTT_BF_K.tsv"):
        assert os.path.exists(stem + suffix) and not os.path.exists(os.path.join(logdir, "tiny_BD_plain" + suffix)), suffix
    rtt = np.loadtxt(stem + "_RTT.tsv", skiprows=1, ndmin=2)
    head = open(stem + "_RTT.tsv").readline().split()
    bf = np.loadtxt(stem + "_RTT_BF.tsv", skiprows=1, ndmin=2)
    assert open(stem + "_RTT_BF.tsv").readline().split() == logs.RTT_BF_HEAD
    pr = open(stem + "_RTT_BF_prior.tsv").read().split("\n")
    assert pr[0].split("\t") == logs.RTT_BF_PRIOR_HEAD
    prior = dict(zip(pr[0].split("\t"), [float(x) for x in pr[1].split("\t")]))
    print("prior", prior)
    assert prior["reps"] == 65536 and 0.5 * 65536 < prior["accepted"] < 65536 and prior["capped"] == 0 and prior["poi_lambda"] == 0
    # the prior is the device's counts for the run's span and seed
    want = shift_prior_ref(a, b, 0, 65536, 9)
    assert prior["accepted"] == want.totals[0] and len(bf) == len(want.shift_hist) == int(b - a)
    assert np.array_equal(bf[:, 3], want.shift_hist / float(want.totals[0]))
    ps = shift_bf.prior_s(want.shift_hist, want.totals[0])
    bf2, bf6 = shift_bf.thresholds(ps)
    assert (prior["prior_s"], prior["bf2"], prior["bf6"]) == (ps, bf2, bf6)
    # the BF columns are shift_bf applied to the table's own count columns
    fb, fd = rtt[:, head.index("birth_counts")], rtt[:, head.index("death_counts")]
    assert np.array_equal(bf[:, 0], rtt[:, 0]) and np.array_equal(bf[:, 1], fb) and np.array_equal(bf[:, 2], fd)
    assert np.array_equal(bf[:, 4], shift_bf.two_ln_bf(fb, ps), equal_nan=True)
    assert np.array_equal(bf[:, 5], shift_bf.two_ln_bf(fd, ps), equal_nan=True)
    b2, b6 = shift_bf.flags(fb, rtt[:, head.index("birth_rate")], bf2, bf6)
    d2, d6 = shift_bf.flags(fd, rtt[:, head.index("death_rate")], bf2, bf6)
    for col, v in ((6, b2), (7, b6), (8, d2), (9, d6)):
        assert np.array_equal(bf[:, col], v, equal_nan=True), col
    K = np.loadtxt(stem + "_RTT_BF_K.tsv", skiprows=1, ndmin=2)
    kc = np.loadtxt(stem + "_RTT_K.tsv", skiprows=1, ndmin=2)
    assert np.array_equal(K[:, 1], want.k_accepted / float(want.totals[0]))
    assert np.array_equal(K[:32, 2], kc[:, 1] / kc[:, 1].sum()) and np.array_equal(K[:32, 3], kc[:, 2] / kc[:, 2].sum())
    assert prior["birth_2lnBF_shift"] == shift_bf.k_bayes_factor(kc[:, 1], want.k_accepted) or (
        np.isnan(prior["birth_2lnBF_shift"]) and np.isnan(shift_bf.k_bayes_factor(kc[:, 1], want.k_accepted)))
    print("bins flagged: birth BF2 %d BF6 %d, death BF2 %d BF6 %d" % tuple(int(np.sum(~np.isnan(v))) for v in (b2, b6, d2, d6)))


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % sys.argv[1])
