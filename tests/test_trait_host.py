"""Trait-dependent rates, the host side: the numpy restatement (tests/helpers/trait_ref.py) against the oracle's binning and
Keiding likelihood at kappa = 0, the trait file and its refusals, the command line's refusals, the constants of the header and
the log header.  No GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import trait_ref as tr                # noqa: E402
from oracle import literate_oracle as lo           # noqa: E402


@pytest.fixture(scope="module")
def example(golden_dir):
    G = np.load(os.path.join(golden_dir, "binning_lik.npz"))
    return np.asarray(G["example_TBP/ts"], dtype=float), np.asarray(G["example_TBP/te"], dtype=float)


def test_at_kappa_0_W_is_half_the_oracles_br_length(example):
    ts, te = example
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    x = np.random.default_rng(1).normal(size=len(ts))
    for x0 in (0.0, 1.7):
        W, sb, sd, cnt = tr.weights(ts, te, x, float(t0), len(br), [[x0, 0.0]])
        np.testing.assert_allclose(W[0], br / 2.0, rtol=1e-13, atol=1e-13)
        born, died = tr.counted(ts, te, float(t0), len(br))
        assert born.sum() == sp.sum() and died.sum() == ex.sum()
        np.testing.assert_allclose([sb[0], sd[0]], [sp.sum() * math.log(0.5), ex.sum() * math.log(0.5)], rtol=1e-13)
    lW, lsb, lsd, lcnt = tr.weights_loop(ts[:60], te[:60], x[:60], float(t0), len(br), 0.3, -1.1)
    vW, vsb, vsd, vcnt = tr.weights(ts[:60], te[:60], x[:60], float(t0), len(br), [[0.3, -1.1]])
    np.testing.assert_allclose(vW[0], lW, rtol=1e-13, atol=1e-14)
    np.testing.assert_allclose([vsb[0], vsd[0]], [lsb, lsd], rtol=1e-13)
    assert np.array_equal(vcnt, lcnt)


def test_at_kappa_0_the_likelihood_is_the_oracles_keiding_at_half_rates(example):
    ts, te = example
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    rng = np.random.default_rng(2)
    x = rng.normal(size=len(ts))
    nb = len(br)
    W, sb, sd, _ = tr.weights(ts, te, x, float(t0), nb, [[0.2, 0.0]])
    half = float(np.sum(sp + ex)) * math.log(0.5)
    np.testing.assert_allclose(sb[0] + sd[0], half, rtol=1e-13)
    for _ in range(3):
        lam, mu = rng.uniform(0.05, 0.6, nb), rng.uniform(0.02, 0.3, nb)
        want = lo.BD_lik_Keiding(lam / 2.0, mu / 2.0, sp, ex, br)
        # sum_b log(lam_b) sp_b - lam_b br_b / 2 + sp_b log(1/2)  =  sum_b log(lam_b / 2) sp_b - (lam_b / 2) br_b
        base = tr.baseline_lik(lam, mu, sp.astype(float), ex.astype(float), W[0], W[0])
        np.testing.assert_allclose(base + half, want, rtol=1e-12)
        np.testing.assert_allclose(tr.loglik(lam, mu, sp.astype(float), ex.astype(float), W[0], W[0], sb[0], sd[0]), want, rtol=1e-12)


def test_log_sigmoid_is_finite_at_800():
    z = np.array([-800.0, -40.0, 0.0, 40.0, 800.0])
    ls = tr.log_sigmoid(z)
    assert np.all(np.isfinite(ls)) and ls[0] == -800.0 and ls[2] == math.log(0.5) and ls[4] == 0.0
    assert np.array_equal(tr.sigmoid(z)[[0, 2, 4]], [0.0, 0.5, 1.0])


def test_the_headers_constants_against_the_helpers_and_the_binding():
    from literate_amd import _hip
    src = open(os.path.join(ROOT, "include", "literate_hip_trait.h")).read()
    assert ("#define LR_P_TRAIT_MOVE %d" % tr.P_TRAIT_MOVE) in src and ("#define LR_P_TRAIT_ACCEPT %d" % tr.P_TRAIT_ACCEPT) in src
    assert (_hip.LR_P_TRAIT_MOVE, _hip.LR_P_TRAIT_ACCEPT) == (tr.P_TRAIT_MOVE, tr.P_TRAIT_ACCEPT) == (60, 61)
    assert ("#define LR_TRAIT_F %d" % tr.F) in src and _hip.LR_TRAIT_F == tr.F
    assert _hip.LR_TRAIT_MAX_N * 2 ** tr.F < 2 ** 63
    # no other purpose of the library has these numbers
    taken = set()
    for root, _, files in os.walk(os.path.join(ROOT, "literate_amd", "csrc")):
        for f in files:
            if f.endswith((".h", ".hip")) and f != "lr_trait.hip":
                taken |= {int(m) for m in re.findall(r"#define LR_P_\w+ (\d+)", open(os.path.join(root, f)).read())}
    assert not taken & {60, 61}
    assert _hip.LR_TRAIT_STATE_W == _hip.LR_RJBIN_STATE_W + _hip.LR_ROW + 2 * _hip.LR_RJBIN_MAX_BINS == 1536
    assert _hip.LR_TRAIT_ROW_W == _hip.LR_TRACE_W + 8
    for name in ("lr_trait_weights_workspace_bytes", "lr_trait_weights_plan", "lr_trait_weights", "lr_trait_workspace_bytes",
                 "lr_trait_init", "lr_trait_steps"):
        assert name in _hip.SIGNATURES and re.search(r"\b%s\s*\(" % name, src)
    assert "lr_trait.hip" in __import__("literate_amd.build", fromlist=["SOURCES"]).SOURCES


def write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_trait_file_matching_and_its_refusals(tmp_path):
    from literate_amd import traitrate as T
    good = write(tmp_path / "t.tsv", "name\ttrait\nb\t2.5\na\t-1\nzz\t9\n\n")
    traits = T.read_traits(good)
    assert traits == {"b": 2.5, "a": -1.0, "zz": 9.0}
    assert T.match_traits(["a", "b"], traits).tolist() == [-1.0, 2.5]                 # the data's order; zz is ignored
    with pytest.raises(ValueError, match="no trait value for lineage 'c'"):
        T.match_traits(["a", "c", "b"], traits)
    with pytest.raises(ValueError, match="lineage 'a' has more than one"):
        T.read_traits(write(tmp_path / "d.tsv", "name\ttrait\na\t1\nb\t2\na\t1\n"))
    for bad in ("nan", "inf", "-inf", "big", ""):
        with pytest.raises(ValueError, match="lineage 'b' is not a finite number"):
            T.read_traits(write(tmp_path / "n.tsv", "name\ttrait\na\t1\nb\t%s\n" % bad))
    x, m, sd = T.standardise([1.0, 2.0, 3.0, 6.0])
    assert abs(x.mean()) < 1e-15 and abs(x.std() - 1.0) < 1e-15 and (m, sd) == (3.0, float(np.std([1.0, 2.0, 3.0, 6.0])))
    assert T.standardise([1.0, 2.0], raw=True)[1:] == (0.0, 1.0)
    with pytest.raises(ValueError, match="same for every lineage"):
        T.standardise([2.0, 2.0])
    lo_, hi_ = T.x0_range(np.array([-1.0, 4.0]))
    assert (lo_, hi_) == (-1.5, 4.5)
    # lineages the window drops take their traits with them
    data = write(tmp_path / "d.txt", "id\tts\tte\nold\t1900\t1950\nin1\t1960\t1970\nin2\t1980\t1999\nlate\t2005\t2010\n")
    from literate_amd.literate_library import parse_ts_te
    ts, te, _, _ = parse_ts_te(data, False, 1950, 2000, 0.5)
    names = T.kept_names(data, False, 1950, 2000)
    assert names == ["in1", "in2"] and len(ts) == 2
    assert T.match_traits(names, {"in1": 1.0, "in2": 2.0}).tolist() == [1.0, 2.0]    # old and late need no value


def test_the_command_line_refuses_by_name(tmp_path, monkeypatch):
    import LiteTraitRate as cli
    from literate_amd import traitrate as T
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-d", "x.txt", "-trait_data", "t.tsv"]
    for flags, word in ((["-model_BDI", "0"], "-model_BDI 0"), (["-model_BDI", "3"], "-model_BDI 3"), (["--replicates", "a*"], "--replicates"),
                        (["--mc3", "4"], "--mc3"), (["--ppc", "0.1"], "--ppc:"), (["--ppc_age", "0.1"], "--ppc_age"), (["--ade", "0.1"], "--ade:"),
                        (["--ade_joint", "0.1"], "--ade_joint"), (["--waic", "0.1"], "--waic"), (["--loo", "0.1"], "--loo"),
                        (["--trait_tune", "1.0"], "--trait_tune"), (["--trait_every", "-1"], "--trait_every"), (["--rtt", "1.5"], "--rtt")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + flags)
        assert word in str(e.value), (flags, e.value)
    with pytest.raises(SystemExit, match="-trait_data FILE is required"):
        cli.main(["-d", "x.txt"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="several ranks"):
        cli.main(base)
    args = cli.build_parser().parse_args(base)
    assert (args.trait_every, args.trait_win_x0, args.trait_win_kappa, args.trait_tune, args.model_BDI, args.chains) == (10, 0.5, 0.1, 0.1, 2, 1)
    assert T.arg_error(args) is None


def test_log_headers_and_paths(tmp_path):
    from literate_amd import _hip
    from literate_amd import traitrate as T
    # the reference's header (other/LiteTraitRate.py:637), column for column
    assert T.TRAIT_MCMC_HEAD == ["it", "posterior", "likelihood", "prior", "lambda_avg", "mu_avg", "K_l", "K_m", "x0_l", "kappa_l", "x0_m",
                                 "kappa_m", "root_age", "death_age", "gamma_rate_hp", "poisson_rate_hp"]
    data = str(tmp_path / "bands.txt")
    out_dir, paths, stem = T.log_paths(data, "_tag", 3)
    assert out_dir == str(tmp_path) + "/literate_mcmc_logs" and paths["mcmc"] == out_dir + "/bands_tag_c3_trait_mcmc.log"
    assert T.log_paths(data)[1]["sp_rates"].endswith("/bands_trait_sp_rates.log") and T.log_paths(data)[1]["ex_rates"].endswith("/bands_trait_ex_rates.log")
    os.mkdir(out_dir)
    w = T.TraitLogWriter(data, "", 2, T.header_lines(1.25, 0.5, False, 7, -2.0, 2.0))
    K, TW = _hip.LR_KMAX, _hip.LR_TRACE_W
    rows = np.full((2, 2, _hip.LR_TRAIT_ROW_W), np.nan)
    for s in range(2):
        for c in range(2):
            r = rows[s, c]
            r[:13] = [10 * s, -5.5, -4.0, -1.5, 0.3, 0.2, 2, 1, 0.0, 30.5, 1.1, 1.2, 0.9]
            r[13:15], r[13 + K] = [0.25, 0.35], 12.5
            r[13 + 2 * K - 1] = 0.2
            r[TW:] = [0.1, 0.7, -0.2, 1.5, -100.0, -200.0, 3, 4]
    w.append(rows)
    lines = open(T.log_paths(data, "", 1)[1]["mcmc"]).read().splitlines()
    assert lines[0].startswith("# trait: 7 lineages, standardised; mean 1.25, sd 0.5") and lines[1].split("\t") == T.TRAIT_MCMC_HEAD
    assert lines[2].split("\t") == ["0", "-5.5", "-4.0", "-1.5", "0.3", "0.2", "2", "1", "0.1", "0.7", "-0.2", "1.5", "0.0", "30.5", "1.1", "0.9"]
    assert len(lines) == 4 and lines[3].split("\t")[0] == "10"
    assert open(T.log_paths(data, "", 0)[1]["sp_rates"]).read().splitlines()[0].split("\t") == ["0.25", "0.35", "12.5"]
    assert open(T.log_paths(data, "", 0)[1]["ex_rates"]).read().splitlines() == ["0.2", "0.2"]


def test_window_tuning_rule_and_hpd():
    from literate_amd import traitrate as T
    assert T.tuned(0.5, 0.3, 1) == 0.5 and T.tuned(0.5, float("nan"), 3) == 0.5
    assert T.tuned(0.5, 0.0, 1) == 0.5 * math.exp(-1.2) and T.tuned(0.5, 0.8, 4) == 0.5 * math.exp(1.0)
    v = np.arange(100.0)
    assert T.hpd(v) == (0.0, 94.0)
    assert T.hpd(v) == tuple(lo.calcHPD(v, 0.95))
