"""Age-dependent extinction without a GPU: the header against the ctypes bindings and the build; the numpy restatement of
lr_ade_profile against its own scalar loop; scale invariance; k = 1 as the cumulative sum of the rates; the grid, mixture and
quantile logic of literate_amd.ade on hand-built curves; the tables' headers and a round trip; the sentences of arg_error and
the flags of the three command lines; and recovery of a simulated shape with the restatement in the device's place."""
import importlib
import math
import os
import re

import numpy as np
import pytest

from helpers import ade_cases as K
from helpers import ade_ref as ref
from literate_amd import ade

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_matches_the_bindings_and_the_build():
    from literate_amd import _hip, build
    with open(os.path.join(ROOT, "include", "literate_hip_ade.h")) as f:
        text = f.read()
    assert '#include "literate_hip.h"' in text and "#define LR_ADE_MAX_BINS 512" in text
    assert _hip.LR_ADE_MAX_BINS == 512 == ade.MAX_BINS
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decl = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int64_t|int)\s+(lr_\w+)\s*\(([^)]*)\)\s*;", code)}
    assert sorted(decl) == ["lr_ade_classes", "lr_ade_profile", "lr_ade_profile_workspace_bytes"]
    C = _hip.C
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    for name, (res, args) in decl.items():
        want = [C.c_void_p if "*" in a else ctype[a.split()[0]] for a in (x.strip() for x in args.split(","))]
        got_res, got_args = _hip.SIGNATURES[name]
        assert got_res is (C.c_int64 if res == "int64_t" else C.c_int32) and got_args == want, name
    assert "lr_ade.hip" in build.SOURCES and any(h.endswith("literate_hip_ade.h") for h in build.HEADERS)
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        assert "lr_ade" not in f.read()                       # (its own header: other tests enumerate literate_hip.h)
    lib = _hip.load()
    for name in decl:
        assert hasattr(lib, name)
    assert lib.lr_ade_profile_workspace_bytes(40, 1000, 65) >= 8 * (40 * 40 + 1000 * 40 + 820) + 4 * (820 + 40)
    assert lib.lr_ade_profile_workspace_bytes(513, 1, 1) == _hip.LR_ERR_SIZE
    assert lib.lr_ade_profile_workspace_bytes(512, 1 << 16, 1 << 15) == _hip.LR_ERR_SIZE


@pytest.mark.parametrize("name", ["a1", "a2", "a3", "a40"])
def test_the_vectorised_restatement_equals_the_scalar_loop(name):
    dead, cens, mu, shapes = K.profile_inputs(name)
    ll, c, flag, mag = ref.profile(dead, cens, mu, shapes, with_scale=True)
    assert not flag.any()
    for s in range(min(len(mu), 2)):
        for g in sorted({0, len(shapes) // 2, len(shapes) - 1}):
            l2, c2 = ref.profile_loop(dead, cens, mu[s], shapes[g])
            assert abs(ll[s, g] - l2) <= 1e-12 * mag[s, g] and (c[s, g] == c2 or abs(c[s, g] / c2 - 1.0) <= 1e-11), (s, g)


def test_the_classes_of_the_edge_lineages():
    es, ee = K.P.edge_lineages(40)
    dead, cens, tot = ref.classes(es, ee, K.T0, 40)
    assert tot.tolist() == [7, 8] and dead.sum() == 3 and cens.sum() == 4
    assert dead[0, 0] == 1 and dead[0, 39] == 1 and dead[39, 0] == 1 and cens[0] == 2 and cens[39] == 2


def test_scaled_rates_give_the_multiplier_divided_and_the_same_value():
    dead, cens, mu, shapes = K.profile_inputs("a40")
    for k in (0.125, 1.0, 8.0):
        ll, c, mag = ref.profile_one(dead, cens, mu[0], k)
        for f in (1e-12, 1e6, 0.25):
            l2, c2, _ = ref.profile_one(dead, cens, mu[0] * f, k)
            assert abs(l2 - ll) <= 1e-11 * mag and abs(c2 * f / c - 1.0) <= 1e-11, (k, f)


def test_at_shape_one_the_hazard_is_the_cumulative_sum_of_the_rates():
    dead, cens, mu, _ = K.profile_inputs("a40")
    assert np.allclose(ref.weights(1.0, 40), 1.0, rtol=1e-15, atol=0)          # (j expm1(log1p(1 / j)): 1 to an ulp or two)
    n, h, d, ce = ref.tables(dead, cens, mu[0], 1.0)
    jb, a, _ = ref.class_list(dead)
    C = np.concatenate([[0.0], np.cumsum(mu[0])])
    assert np.allclose(h, C[jb + a] - C[jb], rtol=1e-13, atol=0) and np.allclose(d, mu[0][jb + a], rtol=1e-15)
    assert math.isclose(ce, float(np.sum(cens * (C[40] - C[:40]))), rel_tol=1e-13)
    # and (j + 1)^k - j^k without the cancellation
    j = np.arange(1, 40.0)
    assert np.allclose(ref.weights(2.0, 40)[1:], (j + 1) ** 2 - j ** 2, rtol=1e-14)
    assert np.allclose(ref.weights(0.5, 40)[1:], 1.0 / (np.sqrt(j + 1) + np.sqrt(j)), rtol=1e-14)


def test_flags_and_degenerate_cases_of_the_restatement():
    dead = np.zeros((3, 3), dtype=np.int64)
    dead[0, 1] = 2
    cens = np.array([0, 1, 0])
    mu = np.array([[0.1, 0.2, 0.3], [0.1, 0.0, 0.3], [0.0, 0.2, 0.0], [np.nan, 0.2, 0.3], [0.1, 0.2, -1.0], [0.1, np.inf, 0.3]])
    ll, c, flag = ref.profile(dead, cens, mu, [1.0, np.nan, 0.0, -2.0, np.inf, 2.0])
    assert flag.tolist() == [0, 1, 0, 1, 1, 1]
    assert np.isnan(ll[flag == 1]).all() and np.isnan(ll[:, 1:5]).all() and np.isfinite(ll[flag == 0][:, [0, 5]]).all()
    assert ref.profile_one(np.zeros((3, 3), dtype=np.int64), cens, mu[0], 1.0) == (0.0, 0.0, 0.0)
    assert ref.profile_one(np.array([[3]]), np.array([0]), np.array([0.3]), 2.0) == (0.0, math.inf, 0.0)


def test_the_coarse_grid_and_the_parabola():
    ks = ade.coarse_shapes()
    assert len(ks) == 65 and ks[0] == 0.125 and ks[32] == 1.0 and ks[64] == 8.0 and (np.diff(ks) > 0).all()
    logk = np.log(ks)
    h = logk[1] - logk[0]
    # an exact parabola: vertex and width are recovered wherever the maximum node lies inside
    for m, se in ((0.3, 0.2), (-1.01, 0.05), (1.9, 0.5)):
        v, s = ade.refine(logk, (-0.5 * ((logk - m) / se) ** 2)[None, :])
        assert abs(v[0] - m) <= 1e-9 and abs(s[0] / se - 1.0) <= 1e-9
    # a maximum on the edge: the index is clamped to 1 and the vertex clipped to the neighbours
    v, s = ade.refine(logk, (-0.5 * ((logk + 5.0) / 0.5) ** 2)[None, :])
    assert v[0] == logk[0] and abs(s[0] / 0.5 - 1.0) <= 1e-9
    # no curvature: the middle node and the grid step
    v, s = ade.refine(logk, np.zeros((1, 65)))
    assert v[0] == logk[1] and abs(s[0] - h) <= 1e-15
    v, s = ade.refine(logk, np.abs(logk - logk[10])[None, :] * -1.0 + np.where(np.arange(65) == 10, -1.0, 0.0)[None, :])
    assert logk[8] <= v[0] <= logk[12] and s[0] > 0
    fs = ade.fine_shapes(np.array([0.1, 0.3]), np.array([0.05, 0.02]))
    assert len(fs) == 129 and math.isclose(fs[0], math.exp(0.1 - 0.3)) and math.isclose(fs[-1], math.exp(0.3 + 0.12))
    assert np.allclose(np.diff(np.log(fs)), (0.42 + 0.2) / 128)
    fs = ade.fine_shapes(np.array([-2.0, 2.0]), np.array([0.5, 0.5]))
    assert math.isclose(fs[0], 0.125) and math.isclose(fs[-1], 8.0)          # clipped to the coarse range


def test_the_mixture_and_its_quantile_nodes():
    shapes = np.array([0.5, 0.8, 1.0, 1.25, 2.0])
    p = np.array([0.02, 0.28, 0.15, 0.53, 0.02])                 # CDF 0.02, 0.30, 0.45, 0.98, 1
    m = ade.mixture(shapes, p)
    assert math.isclose(m["shape_mean"], float(np.sum(p * shapes))) and m["shape_median"] == 1.25 and m["shape_q025"] == 0.8
    assert m["shape_q975"] == 1.25 and math.isclose(m["p_shape_lt_1"], 0.3) and math.isclose(m["edge_mass"], 0.04)
    assert ade.quantile_node(shapes, p, 0.01) == 0.5 and ade.quantile_node(shapes, p, 0.999) == 2.0
    assert ade.quantile_node(shapes, np.array([0.2] * 5), 1.5) == 2.0      # beyond the CDF's end: the last node
    w = ade.node_weights(np.array([[0.0, math.log(3.0)], [-1e4, -1e4 + math.log(3.0)]]))
    assert np.allclose(w, [[0.25, 0.75], [0.25, 0.75]])
    # p(g) is the mean over the draws of the per-draw weights, not the weights of the mean curve
    class Two:
        def classes(self, ts, te, t0, n_bins):
            # (a death per birth bin, in the last bin: cells with jb + a < n_bins, as lr_ade_classes fills them)
            return np.eye(n_bins, dtype=np.int64)[:, ::-1].copy(), np.ones(n_bins, dtype=np.int64), np.array([2 * n_bins, 0])

        def profile(self, dead, cens, mu, shapes):
            logk = np.log(np.asarray(shapes))
            peak = np.asarray(mu)[:, :1]                                 # the draw's first rate is its curve's peak
            return -0.5 * ((logk[None, :] - peak) / 0.1) ** 2, np.ones((len(mu), len(shapes))), np.zeros(len(mu), dtype=np.int32)

        def summary(self, vals):
            return ref.Restated().summary(vals)
    mu = np.zeros((4, 3))
    mu[:, 0] = [-0.2, -0.2, 0.4, 0.4]
    res = ade.fit_rates(None, None, 0.0, mu, profile=Two())
    assert np.allclose(res.cond.shape_ml, np.exp(mu[:, 0]), rtol=1e-9) and np.allclose(res.cond.se, 0.1, rtol=1e-6)
    logf = np.log(res.fine_shapes)
    assert math.isclose(logf[0], -0.8, abs_tol=1e-9) and math.isclose(logf[-1], 1.0, abs_tol=1e-9)
    assert math.isclose(res.fit["p_shape_lt_1"], 0.5, abs_tol=0.03) and math.isclose(res.weight.sum(), 1.0, rel_tol=1e-12)
    assert math.isclose(res.fit["shape_mean"], 0.5 * (math.exp(-0.2) + math.exp(0.4)) * math.exp(0.005), rel_tol=1e-3)
    assert res.fit["shape_q025"] < math.exp(-0.2) < res.fit["shape_median"] <= math.exp(0.4) < res.fit["shape_q975"]
    assert math.isclose(res.fit["grid_step_over_se"], 1.8 / 128 / 0.1, rel_tol=1e-6) and res.fit["edge_mass"] < 1e-6
    assert np.allclose(res.cond.lr, 2.0 * 0.5 * (mu[:, 0] / 0.1) ** 2, rtol=1e-3)
    assert res.fit["draws"] == 4 and res.fit["draws_flagged"] == 0 and res.fit["bins"] == 3 and res.fit["classes"] == 3
    assert res.fit["shape_ml_hpd_low"] == res.cond.shape_ml.min() and res.fit["shape_ml_hpd_high"] == res.cond.shape_ml.max()


def test_too_few_unflagged_draws_and_too_many_bins_are_refused():
    ts, te = K.recovery_data(1.0, 1.0)
    mu = np.stack([K.REC_MU] * 3)
    mu[1:, 4] = np.nan
    with pytest.raises(ValueError, match="fewer than a 95 % HPD takes"):
        ade.fit_rates(ts, te, 0.0, mu, profile=ref.Restated())
    with pytest.raises(ValueError, match="at most 512"):
        ade.fit_rates(ts, te, 0.0, np.ones((2, 513)), profile=ref.Restated())

    class Eng:
        n_bins = 513
    with pytest.raises(ValueError, match="513 time bins"):
        ade.write_run(Eng(), 1, 1, 1, 0, 0.2, 10, "x")


_recovered = {}


def recovered(k, c):
    """fit_rates on the recovery data with the true rates (twice: an HPD takes two draws), computed once"""
    if (k, c) not in _recovered:
        ts, te = K.recovery_data(k, c)
        _recovered[(k, c)] = ade.fit_rates(ts, te, 0.0, np.stack([K.REC_MU, K.REC_MU]), profile=ref.Restated())
    return _recovered[(k, c)]


def test_a_simulated_shape_is_recovered_given_the_true_rates():
    """30 bins, 100 births per bin, rates 0.05 / 0.15 / 0.3 by thirds, k = 0.6, c = 1.5"""
    ts, te = K.recovery_data(0.6, 1.5)
    dead, cens, tot = ref.classes(ts, te, 0.0, K.REC_BINS)
    assert tot.tolist() == [3000, 0]
    # the seed, by the restatement alone: the profile at the truth is within a 95 % likelihood-ratio of the best node
    ks = ade.coarse_shapes()
    ll = ref.profile(dead, cens, K.REC_MU[None, :], np.concatenate([ks, [0.6]]))[0][0]
    assert 2.0 * (ll[:65].max() - ll[65]) < 3.84
    f = recovered(0.6, 1.5).fit
    print({k: f[k] for k in ade.FIT_FLOATS})
    assert f["shape_q025"] <= 0.6 <= f["shape_q975"] and f["shape_q975"] - f["shape_q025"] < 0.08
    assert f["edge_mass"] < 1e-6 and f["p_shape_lt_1"] > 0.999 and f["lr_mean"] > 100.0 and 0.05 < f["grid_step_over_se"] < 0.2
    assert f["const_shape_ml"] > f["shape_q975"]                    # the constant baseline reads the rising rates as ageing
    assert f["deaths"] + f["censored"] == 3000 and f["draws"] == 2
    k_hat = f["const_shape_ml"]
    assert math.isclose(f["const_mean_longevity"], f["const_scale"] * math.gamma(1.0 + 1.0 / k_hat), rel_tol=1e-12)


def test_without_an_age_effect_the_constant_baseline_gives_a_false_signal():
    f = recovered(1.0, 1.0).fit
    print({k: f[k] for k in ade.FIT_FLOATS})
    assert f["shape_q025"] <= 1.0 <= f["shape_q975"]
    assert f["const_lr"] > f["lr_mean"] and f["lr_mean"] < 3.84 and f["const_shape_ml"] > 1.0


def test_the_tables_headers_and_a_round_trip(tmp_path):
    res = recovered(0.6, 1.5)
    stem = str(tmp_path / "run")
    ade.write_tables(stem, res)
    with open(stem + "_ADE.tsv") as f:
        head, vals = [l.rstrip("\n").split("\t") for l in f]
    assert head == ade.FIT_HEAD == ade.FIT_INTS + ade.FIT_FLOATS and len(vals) == len(head)
    assert head[:9] == ["draws", "draws_flagged", "lineages", "lineages_used", "lineages_unused", "bins", "deaths", "censored", "classes"]
    assert all("." not in vals[i] for i in range(9)) and all("." in v or "e" in v or v in ("inf", "nan") for v in vals[9:])
    with open(stem + "_ADE_shape.tsv") as f:
        rows = [l.rstrip("\n").split("\t") for l in f]
    assert rows[0] == ade.SHAPE_HEAD == ["grid", "shape", "weight", "loglik_mean", "loglik_min", "loglik_max"]
    assert len(rows) == 1 + 65 + 129
    fit, shape = ade.read_tables(stem)
    assert fit == {k: res.fit[k] for k in ade.FIT_HEAD}
    assert [r[0] for r in shape] == ["coarse"] * 65 + ["fine"] * 129
    assert [r[1] for r in shape[:65]] == res.coarse_shapes.tolist() and [r[1] for r in shape[65:]] == res.fine_shapes.tolist()
    assert [r[2] for r in shape[65:]] == res.weight.tolist() and all(r[4] <= r[3] <= r[5] for r in shape)
    assert "edge_mass" in ade._say(stem, res) and ade._say(stem, res).startswith("ADE: ")


def test_arg_error():
    assert ade.arg_error(0.2, 1000) is None and ade.arg_error(0.0, 1) is None and ade.arg_error(0.2, 10, model=1) is None
    assert "burn-in fraction in [0, 1)" in ade.arg_error(1.0, 10) and "burn-in" in ade.arg_error(-0.1, 10)
    assert "burn-in" in ade.arg_error(float("nan"), 10)
    assert "--ade_draws must be at least 1" in ade.arg_error(0.2, 0)
    assert "-pyrate_output" in ade.arg_error(0.2, 10, pyrate_output=True)
    assert "-rm_first_bin 1" in ade.arg_error(0.2, 10, rm_first_bin=True)
    assert "-model_BDI 3" in ade.arg_error(0.2, 10, model=3)
    # what --ppc_age refuses, --ade refuses
    from literate_amd import ppc_age
    for kw in (dict(), dict(model=3), dict(pyrate_output=True), dict(rm_first_bin=True), dict(model=0), dict(model=1)):
        for burn, n in ((0.2, 10), (1.0, 10), (0.2, 0)):
            assert (ade.arg_error(burn, n, **kw) is None) == (ppc_age.arg_error(burn, n, **kw) is None)


@pytest.mark.parametrize("script", ["LiteRateForward", "DDRate", "trend_rate"])
def test_the_command_lines_take_the_flags(script):
    cli = importlib.import_module(script)
    a = cli.build_parser().parse_args(["-d", "x"])
    assert a.ade == -1.0 and a.ade_draws == 1000
    a = cli.build_parser().parse_args(["-d", "x", "--ade", "0.25", "--ade_draws", "64", "--ppc_age", "0.5"])
    assert a.ade == 0.25 and a.ade_draws == 64 and a.ppc_age == 0.5 and a.ppc_age_draws == 1000
    src = open(os.path.join(ROOT, script + ".py")).read()
    assert src.index("args.ppc_age != -1.0 and n_samples") < src.index("args.ade != -1.0 and n_samples") < src.index("args.waic != -1.0 and n_samples")
    with pytest.raises(SystemExit) as ex:
        cli.main(["-d", "x", "--ade", "1.5"])
    assert "--ade takes a burn-in fraction" in str(ex.value)
