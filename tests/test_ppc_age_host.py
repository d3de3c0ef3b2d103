"""The lifespan check without a GPU: the numpy restatement of lr_ppc_age against its own scalar loop on every case of the
table (tests/helpers/ppc_age_cases.py), the condition the device test rests on (no fragile pair in any case), the
conservation laws of the counts, the distribution of the simulated lifespans, the summary tables on a hand-made matrix,
the sentences of arg_error, the flags of the three command lines and the header against the ctypes bindings."""
import os
import re

import numpy as np
import pytest

from helpers import ppc_age_cases as K
from helpers import ppc_age_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(K.TABLE)


@pytest.mark.parametrize("name", NAMES)
def test_the_vectorised_restatement_equals_the_scalar_loop(name):
    ts, te, mu, seed, _ = K.inputs(name)
    w = K.want(name)
    obs, rep, tot = ref.ppc_age_loop(ts, te, K.T0, mu, seed)
    assert np.array_equal(w["obs"], obs) and np.array_equal(w["rep"], rep) and np.array_equal(w["totals"], tot)
    # the per-pair record agrees with the counts
    good = w["rep"][:, 0, 0] >= 0
    for s in np.nonzero(good)[0]:
        A = mu.shape[1]
        assert np.array_equal(np.bincount(w["cls"][w["dead"][:, s], s], minlength=A), w["rep"][s, 0])


@pytest.mark.parametrize("name", NAMES)
def test_no_case_holds_a_fragile_pair(name):
    ts, te, mu, seed, _ = K.inputs(name)
    frag = ref.fragile(ts, te, K.T0, mu, seed, base=K.want(name))
    assert len(frag) == 0, frag[:10]


@pytest.mark.parametrize("name", NAMES)
def test_the_counts_conserve_the_lineages(name):
    ts, te, mu, seed, _ = K.inputs(name)
    w = K.want(name)
    n, (S, A) = len(ts), mu.shape
    used, x, jb, fs, dead, oc, cc = ref.lineage_terms(ts, te, K.T0, A)
    assert w["totals"][0] == used.sum() and w["totals"][0] + w["totals"][1] == n and w["totals"][2] + w["totals"][3] == S
    assert w["obs"].sum() == used.sum()
    censor_hist = np.bincount(cc[used], minlength=A)
    bad = ref.flagged(mu)
    assert bad.sum() == w["totals"][3]
    for s in range(S):
        if bad[s]:
            assert (w["rep"][s] == -1).all()
            continue
        assert w["rep"][s].sum() == used.sum()                       # sum_a (deaths + censored) == used
        assert (w["rep"][s, 1] <= censor_hist).all()                 # nobody is censored outside the data's censor classes
    if S > 1 and not bad[1] and (mu[1] == 0).all():
        assert np.array_equal(w["rep"][1, 1], censor_hist) and w["rep"][1, 0].sum() == 0       # an all-zero draw censors everybody


def test_the_table_covers_what_it_says():
    n_s = {v[0] for v in K.TABLE.values()}
    assert {1, K.TILE - 1, K.TILE, K.TILE + 1, 2 * K.TILE + 1} <= n_s
    assert {1, 2, 3, 65} <= {v[1] for v in K.TABLE.values()} and K.TABLE["draws65_slices4"][6] == 4
    assert {1, 2, 64, 65, K.LR_MAX_BINS} <= {v[2] for v in K.TABLE.values()}
    assert {v[3] for v in K.TABLE.values()} == {"year", "continuous"}
    # the chunk edges the docstring names
    assert [K.chunk_of(nb, 99) for nb in (1, 64, 682, 683, 1365, 1366)] == [64, 21, 2, 1, 1, 1]
    assert 24 * 1365 + 8 == 32768 and 24 * 2730 + 16 == 65536
    # every kind of flagged draw and every special draw occurs in a case with more than 12 draws
    mu = K.inputs("bins65")[2]
    assert np.isnan(mu[2]).any() and (mu[6] < 0).any() and np.isinf(mu[9]).any() and np.isfinite(mu[12]).all()
    assert ref.flagged(mu).tolist() == [s in (2, 6, 9, 12) for s in range(16)]
    assert (mu[1] == 0).all() and (mu[3] == 1e-300).all() and (mu[5] == 1e300).sum() == 1
    # the edge lineages: used or not as the definition says
    ts, te = K.edge_lineages(7)
    used, x, jb, fs, dead, oc, cc = ref.lineage_terms(ts, te, K.T0, 7)
    assert used.tolist() == [True] * 6 + [False] * 8 + [True]
    assert dead[:6].tolist() == [True, True, False, True, False, False] and not dead[14]
    assert oc[:6].tolist() == [0, 6, 6, 0, 1, 0] and cc[:6].tolist() == [6, 6, 6, 0, 1, 0] and jb[3] == 6 and fs[3] == 0.5


def test_1e300_kills_everybody_who_reaches_its_bin():
    ts, te, mu, seed, _ = K.inputs("bins65")
    w = K.want("bins65")
    A = mu.shape[1]
    b = A // 2
    used, x, jb, *_ = ref.lineage_terms(ts, te, K.T0, A)
    reach = used & (jb <= b)
    # under draw 5 nobody born at or before the bin lives past it
    life_end = x + w["cls"][:, 5] + 1.0
    assert w["dead"][reach, 5].all() and (np.floor(x[reach]) + w["cls"][reach, 5] <= b).all() and (life_end[reach] <= b + 2).all()


def test_the_simulated_lifespans_follow_the_exponential_law():
    ts, te, mu = K.dist_inputs()
    w = ref.ppc_age(ts, te, K.T0, mu, K.DIST_SEED)
    K.check_distribution(w["rep"])


def test_the_summary_tables_on_a_hand_made_matrix():
    from literate_amd import ppc_age
    A = 3
    obs = np.array([[4, 2, 0], [1, 1, 2]])
    # 21 kept draws and a flagged one: s % 5 deaths in class 0, 5 in class 1, the rest of 10 dead in class 2; 10 survive
    rep = np.zeros((22, 2, A), dtype=np.int64)
    for s in range(21):
        rep[s] = [[s % 5, 5, 5 - s % 5], [2, 3, 5]]
    rep = np.insert(rep[:21], 7, -1, axis=0)

    on_host = ref.col_stats
    kept = rep[:, 0, 0] >= 0
    assert kept.sum() == 21 and not kept[7]
    at_risk, deaths, hazard, overall = ppc_age.summarise(obs, rep[kept], on_host)
    assert at_risk.tolist() == [10, 5, 2]
    assert deaths[:, 0].tolist() == [4, 2, 0] and hazard[:, 0].tolist() == [0.4, 0.4, 0.0]
    # class 1: always 5 deaths
    assert deaths[1].tolist() == [2.0, 5.0, 5.0, 5.0, 1.0]
    assert deaths[0, 1] == np.mean([s % 5 for s in range(21)]) and deaths[0, 4] == np.mean([s % 5 >= 4 for s in range(21)])
    assert hazard[0, 1] == pytest.approx(np.mean([(s % 5) / 20.0 for s in range(21)]), rel=1e-14)
    assert overall[0].tolist() == [6.0, 10.0, 10.0, 10.0, 1.0]                       # total deaths: 6 observed, always 10
    assert overall[1, 0] == 2.0 / 6.0 and overall[2, 0] == 1.0                       # survival 0.6, then 0.36 <= 0.5
    sm = ref.summary(obs, rep)
    assert np.array_equal(sm["kept"], kept) and np.array_equal(sm["at_risk_obs"], at_risk)
    for a, b in ((sm["deaths"], deaths), (sm["hazard"], hazard), (sm["overall"], overall)):
        assert np.array_equal(a, b, equal_nan=True)
    # nobody at risk in the top class of one kept draw: its hazard is undefined, and says so
    rep2 = rep.copy()
    rep2[3] = [[5, 15, 0], [0, 0, 0]]
    _, d2, h2, o2 = ppc_age.summarise(obs, rep2[kept], on_host)
    assert np.isnan(h2[2, 1:]).all() and h2[2, 0] == 0.0 and np.isfinite(h2[:2]).all() and np.isfinite(d2).all()
    obs0 = np.array([[4, 2, 0], [1, 1, 0]])
    _, _, h3, _ = ppc_age.summarise(obs0, rep[kept], on_host)
    assert np.isnan(h3[2]).all() and np.isfinite(h3[:2]).all()
    # no deaths at all in one draw: the mean class at death is undefined
    rep3 = rep.copy()
    rep3[0] = [[0, 0, 0], [10, 5, 5]]
    _, _, _, o3 = ppc_age.summarise(obs, rep3[kept], on_host)
    assert np.isnan(o3[1, 1:]).all() and o3[1, 0] == 2.0 / 6.0 and np.isfinite(o3[0]).all() and o3[2, 1] == (20 * 2.0 + 3.0) / 21.0


def test_the_restated_mean_sums_in_the_devices_order():
    rng = np.random.default_rng(5)
    for n in (1, 2, 255, 256, 257, 1000):
        ints = rng.integers(0, 1 << 40, n).astype(np.float64)
        assert ref.device_mean(ints) == ints.sum() / n                    # integers: exact in any order
        x = rng.random(n) / 3.0
        d = np.sort(x)
        part = [0.0] * 256
        for e in range(n):                                                # thread e % 256 adds its elements in ascending order
            part[e % 256] = part[e % 256] + d[e]
        w = 128
        while w:
            for t in range(w):
                part[t] = part[t] + part[t + w]
            w //= 2
        assert ref.device_mean(x) == part[0] / n and abs(ref.device_mean(x) - x.mean()) <= 4 * n * np.finfo(float).eps * x.mean()


def test_the_files_hold_counts_as_integers_and_numbers_as_floats(tmp_path):
    from literate_amd import ppc_age
    A = 2
    fit = {k: 1 for k in ppc_age.FIT_HEAD}
    fit.update(draws=30, coverage_deaths=0.5, total_deaths_mean=3.25, mean_class_at_death_obs=float("nan"))
    res = ppc_age.AgeResult(None, None, None, None, (1024, 1, 1, 1), None, np.array([7, 3]), np.arange(10.0).reshape(A, 5),
                            np.arange(10.0).reshape(A, 5) / 8.0, None, fit)
    stem = str(tmp_path / "run")
    ppc_age.write_tables(stem, res)
    lines = open(stem + "_PPC_age.tsv").read().splitlines()
    assert lines[0].split("\t") == ppc_age.AGE_HEAD and len(ppc_age.AGE_HEAD) == 12
    assert lines[1].split("\t") == ["0", "7", "0.0", "1.0", "2.0", "3.0", "4.0", "0.0", "0.125", "0.25", "0.375", "0.5"]
    head, row = [l.split("\t") for l in open(stem + "_PPC_age_fit.tsv").read().splitlines()]
    assert head == ppc_age.FIT_HEAD and len(head) == 6 + 15 + 3
    got = dict(zip(head, row))
    assert got["draws"] == "30" and got["classes"] == "1" and got["hazard_classes_extreme"] == "1"
    assert got["coverage_deaths"] == "0.5" and got["total_deaths_mean"] == "3.25" and got["mean_class_at_death_obs"] == "nan"
    assert got["total_deaths_obs"] == "1.0"


def test_arg_error_names_what_it_refuses():
    from literate_amd.ppc_age import arg_error
    assert arg_error(0.2, 1000) is None and arg_error(0.0, 1) is None
    assert arg_error(0.2, 10, model=1) is None and arg_error(0.2, 10, model=0) is None          # immigration-death: the same deaths
    for b in (-0.1, 1.0, 1.5, float("nan")):
        assert "burn-in fraction in [0, 1)" in arg_error(b, 10)
    assert "--ppc_age_draws must be at least 1" in arg_error(0.2, 0)
    assert "-pyrate_output" in arg_error(0.2, 10, pyrate_output=True)
    assert "-rm_first_bin 1" in arg_error(0.2, 10, rm_first_bin=True)
    e = arg_error(0.2, 10, model=3)
    assert "-model_BDI 3" in e and "extinct lineages only" in e
    assert all(arg_error(*a, **k).startswith("--ppc_age") for a, k in (((2.0, 10), {}), ((0.2, 0), {}), ((0.2, 1), dict(model=3))))


@pytest.mark.parametrize("script", ["LiteRateForward", "DDRate", "trend_rate"])
def test_the_three_parsers_carry_both_flags(script):
    import importlib
    cli = importlib.import_module(script)
    a = cli.build_parser().parse_args(["-d", "x"])
    assert a.ppc_age == -1.0 and a.ppc_age_draws == 1000
    a = cli.build_parser().parse_args(["-d", "x", "--ppc_age", "0.25", "--ppc_age_draws", "64", "--ppc", "0.5"])
    assert a.ppc_age == 0.25 and a.ppc_age_draws == 64 and a.ppc == 0.5 and a.ppc_draws == 1000
    src = open(os.path.join(ROOT, script + ".py")).read()
    assert src.index("args.ppc != -1.0 and n_samples") < src.index("args.ppc_age != -1.0 and n_samples") < src.index("args.waic != -1.0 and n_samples")


def test_the_header_matches_the_bindings_and_the_build():
    from literate_amd import _hip, build
    with open(os.path.join(ROOT, "include", "literate_hip_age.h")) as f:
        text = f.read()
    assert '#include "literate_hip.h"' in text
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    decl = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int64_t|int)\s+(lr_\w+)\s*\(([^)]*)\)\s*;", code)}
    assert sorted(decl) == ["lr_ppc_age", "lr_ppc_age_plan", "lr_ppc_age_workspace_bytes"]
    C = _hip.C
    ctype = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double, "uint64_t": C.c_uint64}
    for name, (res, args) in decl.items():
        want = []
        for a in args.split(","):
            a = a.strip()
            if "*" in a:
                want.append(C.POINTER(C.c_int32) if name == "lr_ppc_age_plan" else C.c_void_p)
            else:
                want.append(ctype[a.split()[0]])
        got_res, got_args = _hip.SIGNATURES[name]
        assert got_res is (C.c_int64 if res == "int64_t" else C.c_int32) and got_args == want, name
    assert "lr_age.hip" in build.SOURCES and any(h.endswith("literate_hip_age.h") for h in build.HEADERS)
    assert "LR_PPC_AGE_SLICES" in text and "purpose 41" in text
    src = open(os.path.join(ROOT, "literate_amd", "csrc", "lr_age.hip")).read()
    assert "#define LR_P_PPC_AGE 41" in src and ref.P_PPC_AGE == 41
    assert "41 lr_age.hip" in open(os.path.join(ROOT, "literate_amd", "csrc", "lr_device.h")).read()


def test_the_size_queries_cover_the_case_table(monkeypatch):
    from literate_amd import _hip
    lib = _hip.load()
    plan = (_hip.C.c_int32 * 4)()
    monkeypatch.delenv("LR_PPC_AGE_SLICES", raising=False)
    for name, (n, S, nb, kind, _, _, slices) in K.TABLE.items():
        need = lib.lr_ppc_age_workspace_bytes(n, nb, S)
        assert need >= S * (nb + 1) * 8 + S * 4 and need % 256 == 0, name
        assert lib.lr_ppc_age_plan(n, nb, S, plan) == 0
        assert plan[0] == K.TILE and plan[3] == -(-n // K.TILE) and plan[1] * (plan[2] - 1) < S <= plan[1] * plan[2], (name, list(plan))
    monkeypatch.setenv("LR_PPC_AGE_SLICES", "4")
    assert lib.lr_ppc_age_plan(200, 5, 65, plan) == 0 and list(plan) == [K.TILE, 17, 4, 1]
    monkeypatch.setenv("LR_PPC_AGE_SLICES", "1000")
    assert lib.lr_ppc_age_plan(200, 5, 65, plan) == 0 and list(plan) == [K.TILE, 1, 65, 1]
    assert lib.lr_ppc_age_workspace_bytes(0, 5, 5) == _hip.LR_ERR_SIZE
    assert lib.lr_ppc_age_workspace_bytes(5, _hip.LR_MAX_BINS + 1, 5) == _hip.LR_ERR_SIZE
    assert lib.lr_ppc_age_workspace_bytes(1 << 61, 5, 2) == _hip.LR_ERR_SIZE
