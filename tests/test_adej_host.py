"""The joint sampler of (death-rate skyline, Weibull shape) without a GPU: the restatement tests/helpers/adej_ref.py, which is
the specification the device is held to (tests/test_hip_adej.py), against what can be known exactly - its likelihood in
both forms against tests/helpers/ade_ref.py, the posterior of (log rate, log shape) at K = 1 against a grid integration, the
distribution of K under the prior alone against its closed form - and the host surface of literate_amd.ade_joint."""
import math
import os

import numpy as np
import pytest

from helpers import ade_ref
from helpers import adej_cases as K
from helpers import adej_ref as ref
from helpers import ess_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["a12", "a40", "a1", "a2"])
def test_both_forms_of_the_likelihood_equal_the_profile_restatement_at_c_1(name):
    dead, cens = K.table(name)
    data = ref.Data(dead, cens)
    rng = np.random.default_rng(7)
    for k in (0.3, 1.0, 2.5):
        mu = np.exp(rng.normal(size=data.A) * 0.7 - 1.5)
        want, mag = ade_ref.loglik(1.0, *ade_ref.tables(dead, cens, mu, k))
        a, b = ref.loglik(data, mu, k), ref.loglik_cum(data, mu, k)
        print(name, k, want, a - want, b - want, mag)
        assert abs(a - want) <= 1e-12 * mag and abs(b - want) <= 1e-12 * mag
    if name == "a12":
        assert (data.A, int(dead.sum() + cens.sum()), int(dead.sum()), len(data.n)) == (12, 480, 250, 71)


def pooled(series):
    """pooled mean and Tracer's ESS (summed over the chains, as lr_ess_summary pools) of kept series [C, n]"""
    return float(np.mean(series)), float(sum(ess_ref.series(x)["ess"] for x in series))


def test_the_exact_posterior_at_one_rate():
    dead, cens = K.table("a12")
    data = ref.Data(dead, cens)
    exact = ref.grid_posterior(data)
    print("grid:", exact)
    assert abs(exact["g"][0] - (-0.2582)) < 5e-4 and abs(exact["g"][1] - 0.0645) < 5e-4
    st = ref.Settings(const=1, use_rate_hp=0)
    n_it, s_freq, burn = K.EXACT_ITERS, K.EXACT_S, K.EXACT_BURN
    rows = np.stack([ref.run(data, 0.0, st, ref.PhiloxDraws(K.EXACT_SEED, c), n_it, s_freq)["rows"] for c in range(K.EXACT_CHAINS_HOST)])
    K.check_exact(rows[:, burn:], exact, pooled)


def test_the_number_of_rates_under_the_prior_alone():
    A = 12
    data = ref.Data(np.zeros((A, A), dtype=np.int64), np.zeros(A, dtype=np.int64))
    st = ref.Settings(poisson_prior=2.0, use_rate_hp=0)
    p = ref.k_prior_pmf(A, 2.0)
    assert np.allclose(p[:4], [0.4907, 0.4089, 0.0920, 0.0081], atol=6e-5)
    rows = np.stack([ref.run(data, 0.0, st, ref.PhiloxDraws(K.PRIOR_SEED, c), K.PRIOR_ITERS, K.PRIOR_S)["rows"]
                     for c in range(K.PRIOR_CHAINS_HOST)])
    K.check_prior_k(rows[:, K.PRIOR_BURN:], p, pooled)


def test_a_run_cut_in_two_is_the_same_run_and_the_cap_forces_rejects():
    dead, cens = K.table("a12")
    data = ref.Data(dead, cens)
    st = ref.Settings()
    one = ref.run(data, 0.0, st, ref.PhiloxDraws(3, 5), 300, 3)
    a = ref.run(data, 0.0, st, ref.PhiloxDraws(3, 5), 100, 3)
    b = ref.run(data, 0.0, st, ref.PhiloxDraws(3, 5), 200, 3, it0=100, state=a["state"])
    assert np.array_equal(np.concatenate([a["rows"], b["rows"]]), one["rows"], equal_nan=True)
    assert np.array_equal(one["state"].proposed, b["state"].proposed) and one["state"].proposed.sum() == 300
    assert (one["rows"][:, ref.COL["K"]] > 1).any()
    capped = ref.run(data, 0.0, st, ref.PhiloxDraws(3, 5), 300, 1, k_max=2)
    assert capped["forced"] > 0 and capped["K"].max() == 2


def test_arg_error_and_the_tables_round_trip(tmp_path):
    from literate_amd import _hip, ade, ade_joint
    assert ade_joint.MAX_BINS == 128 == _hip.LR_ADEJ_MAX_BINS == ref.MAX_BINS
    ok = dict(burnin=0.2, n_iter=1000, s_freq=10, win=0.4, n_bins=40)
    assert ade_joint.arg_error(**ok) is None
    for kw, word in ((dict(burnin=1.0), "burn-in"), (dict(burnin=-0.1), "burn-in"), (dict(n_iter=0), "--ade_joint_n"),
                     (dict(s_freq=0), "--ade_joint_s"), (dict(win=0.0), "--ade_joint_win"), (dict(win=float("nan")), "--ade_joint_win"),
                     (dict(n_bins=129), "128"), (dict(model=3), "-model_BDI 3"), (dict(pyrate_output=1), "-pyrate_output"),
                     (dict(n_iter=10, s_freq=10), "samples")):
        msg = ade_joint.arg_error(**dict(ok, **kw))
        assert msg and word in msg, (kw, msg)
    assert ade.arg_error(0.2, 100, model=3) and ade.arg_error(0.2, 100, pyrate_output=1)      # (the same two refusals)
    fit = {k: (3 if k in ade_joint.FIT_INTS else 0.1 + i / 7.0) for i, k in enumerate(ade_joint.FIT_HEAD)}
    rates = [(b, 0.1 + b / 3.0, 0.05, 0.2 + b) for b in range(5)]
    draws = dict(shape=np.random.default_rng(1).random((4, 3)), K=np.ones((4, 3)), lik=np.zeros((4, 3)), prior=np.zeros((4, 3)))
    stem = str(tmp_path / "x")
    ade_joint.write_tables(stem, fit, rates, draws)
    fit2, rates2, draws2 = ade_joint.read_tables(stem)
    assert fit2 == fit and rates2 == [tuple(float(v) for v in r) for r in rates]
    assert all(np.array_equal(draws2[k], draws[k]) for k in draws)
    with open(stem + "_ADE_joint.tsv") as f:
        assert f.readline().rstrip("\n").split("\t") == ade_joint.FIT_HEAD


def test_the_header_matches_the_bindings_and_the_build():
    import re
    from literate_amd import _hip, build
    with open(os.path.join(ROOT, "include", "literate_hip_adej.h")) as f:
        text = f.read()
    assert "#define LR_ADEJ_MAX_BINS 128" in text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decl = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int64_t|int)\s+(lr_\w+)\s*\(([^)]*)\)\s*;", code)}
    assert sorted(decl) == ["lr_adej_init", "lr_adej_loglik", "lr_adej_prepare", "lr_adej_steps", "lr_adej_workspace_bytes"]
    C = _hip.C
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double, "uint64_t": C.c_uint64}
    for name, (res, args) in decl.items():
        want = [C.c_void_p if "*" in a else ctype[a.split()[0]] for a in (x.strip() for x in args.split(","))]
        got_res, got_args = _hip.SIGNATURES[name]
        assert got_res is (C.c_int64 if res == "int64_t" else C.c_int32) and got_args == want, name
    for name, val in (("LR_ADEJ_STATE_W", _hip.LR_ADEJ_STATE_W), ("LR_ADEJ_ROW_W", _hip.LR_ADEJ_ROW_W), ("LR_ADEJ_MOVES", len(ref.MOVES))):
        assert re.search(r"#define %s %d\b" % (name, val), text), name
    assert _hip.LR_ADEJ_ROW_W == ref.ROW_W
    assert "lr_adej.hip" in build.SOURCES and "lr_adej.hip" not in build.ASYNC_UNITS
    assert any(h.endswith("literate_hip_adej.h") for h in build.HEADERS)
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        assert "lr_adej" not in f.read()
    lib = _hip.load()
    for name in decl:
        assert hasattr(lib, name)
    assert lib.lr_adej_workspace_bytes(128) >= 8 * 128 * 129 // 2 and lib.lr_adej_workspace_bytes(129) == _hip.LR_ERR_SIZE
    with open(os.path.join(ROOT, "literate_amd", "csrc", "lr_device.h")) as f:
        assert "48-51 lr_adej.hip" in f.read()
