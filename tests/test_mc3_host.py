"""The host side of the Metropolis-coupled RJ sampler (include/literate_hip_rjmc3.h, literate_amd/mc3.py), no GPU: the numpy
restatement of the ladder (tests/helpers/rjmc3_ref.py) against oracle.mcmc_oracle.run_mcmc at T = 1 and at a constant beta;
the swap round by hand; ladder_betas, the argument refusals and the wiring of --mc3; the header against the binding, the
build and the documents.
"""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

from helpers import rjmc3_ref as ref
from helpers import stream_cases as S
from oracle import literate_oracle as lo
from oracle import mcmc_oracle as mo
from test_hip_replicates import MATRIX, make_stats, settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KMAX = 32


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def same_rows(got, want):
    assert len(got["mcmc"]) == len(want["mcmc"]) > 0
    for k in ("mcmc", "sp", "ex"):
        for a, b in zip(got[k], want[k]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), k


@pytest.mark.parametrize("kw", MATRIX, ids=["_".join("%s%s" % kv for kv in m.items()) for m in MATRIX])
def test_at_one_temperature_the_restatement_is_run_mcmc_bit_for_bit(kw):
    """models 0 to 3 and the settings matrix of test_hip_replicates.py at 40 bins; swap rounds of one replica change nothing"""
    st, start, end = make_stats(1, 40, 7, dead=kw.get("model", 2) == 3)[0]
    with np.errstate(all="ignore"):
        want = mo.run_mcmc(st, start, end, settings(**kw), mo.PhiloxDraws(23, 4), 200, 3, k_max=KMAX)
    got = ref.run_ladder(st, start, end, settings(**kw), 23, 4, [1.0], 5, 200, 3, k_max=KMAX)
    same_rows(got, want)
    assert got["ladder"].shape == (67, 1, 4) and (got["ladder"][:, 0, 0] == 0).all() and got["swaps"].shape == (0, 2)
    np.testing.assert_array_equal(got["ladder"][:, 0, 1], [r[2] for r in want["mcmc"]])
    assert got["states"][0]["likA"] == want["final"][4] and got["pos"] == [0]


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_at_a_constant_beta_the_restatement_is_run_mcmc_on_the_scaled_likelihood(model):
    """beta = 0.3, no swaps: the rows of run_mcmc(lik_fn = 0.3 calc_likelihood) to 1e-12, its likelihood column divided by 0.3"""
    st, start, end = make_stats(1, 40, 7, dead=model == 3)[0]
    with np.errstate(all="ignore"):
        want = mo.run_mcmc(st, start, end, settings(model=model), mo.PhiloxDraws(5, 2), 300, 1, k_max=KMAX,
                           lik_fn=lambda Lv, Mv: 0.3 * lo.calc_likelihood(model, Lv, Mv, st))
    got = ref.run_ladder(st, start, end, settings(model=model), 5, 2, [0.3], 0, 300, 1, k_max=KMAX)
    g, w = np.array(got["mcmc"]), np.array(want["mcmc"])
    np.testing.assert_allclose(g[:, 2], w[:, 2] / 0.3, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g[:, 1], w[:, 2] / 0.3 + w[:, 3], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(np.delete(g, [1, 2], axis=1), np.delete(w, [1, 2], axis=1), rtol=1e-12, atol=1e-12)
    for k in ("sp", "ex"):
        for a, b in zip(got[k], want[k]):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)
    assert (g[:, 6:8].max(axis=0) > 1).any(), "a heated chain holds rate shifts"


def test_the_swap_round_by_hand_for_both_parities():
    betas = [1.0, 0.5, 0.25, 0.125]
    lik = [-10.0, -8.0, -9.0, -12.0]
    # round 2 (even): the pairs of positions (0, 1) and (2, 3).  (1 - .5)(-8 + 10) = 1 >= log u whatever u; (.25 - .125)(-12 + 9) =
    # -.375 against log .5 = -.693: accepted, against log .9 = -.105: refused
    counts, margins = [[0, 0] for _ in range(3)], []
    assert ref.swap_round(2, [0, 1, 2, 3], lik, betas, lambda j: 0.5, counts, margins) == [1, 0, 3, 2]
    assert counts == [[1, 1], [0, 0], [1, 1]]
    np.testing.assert_allclose(margins, [1.0 - np.log(0.5), -0.375 - np.log(0.5)], rtol=1e-15)
    assert ref.swap_round(2, [0, 1, 2, 3], lik, betas, lambda j: {0: 0.5, 2: 0.9}[j], counts) == [1, 0, 2, 3]
    assert counts == [[2, 2], [0, 0], [2, 1]]
    # round 1 (odd): the pair (1, 2) alone.  From pos = [1, 0, 3, 2] replica 0 holds position 1 and replica 3 position 2:
    # (.5 - .25)(lik[3] - lik[0]) = .25 (-2) = -.5 against log .7 = -.357: refused, against log .6 = -.511: accepted
    assert ref.swap_round(1, [1, 0, 3, 2], lik, betas, lambda j: {1: 0.7}[j], counts) == [1, 0, 3, 2]
    assert ref.swap_round(1, [1, 0, 3, 2], lik, betas, lambda j: {1: 0.6}[j], counts) == [2, 0, 3, 1]
    assert counts == [[2, 2], [2, 1], [2, 1]]
    # u = 0 is accepted whatever the likelihoods; an odd ladder's last position sits out the even rounds
    assert ref.swap_round(4, [2, 1, 0], [0.0, 5.0, -50.0], [1.0, 0.5, 0.2], lambda j: {0: 0.0}[j]) == [2, 0, 1]
    # (.5 - .2)(0 - 5) = -1.5 against log .99: refused, against log .2 = -1.609: accepted
    assert ref.swap_round(3, [2, 1, 0], [0.0, 5.0, -50.0], [1.0, 0.5, 0.2], lambda j: {1: 0.99}[j]) == [2, 1, 0]
    assert ref.swap_round(3, [2, 1, 0], [0.0, 5.0, -50.0], [1.0, 0.5, 0.2], lambda j: {1: 0.2}[j]) == [1, 2, 0]
    assert ref.swap_round(7, [0], [1.0], [1.0], lambda j: 1 / 0) == [0] and ref.swap_round(2, [1, 0], [1.0, 2.0], [1.0, 0.5], lambda j: 0.3) == [0, 1]


@pytest.mark.parametrize("T,every", [(2, 1), (3, 1), (5, 1), (8, 3)])
def test_the_positions_stay_a_permutation_and_the_counters_add_up(T, every):
    st, start, end = make_stats(1, 40, 7)[0]
    n_it = 60
    out = ref.run_ladder(st, start, end, settings(), 9, 100, ref.ladder_betas(T, 0.5), every, n_it, 1)
    assert sorted(out["pos"]) == list(range(T))
    who = out["ladder"][:, :, 0].astype(int)
    assert (np.sort(who, axis=1) == np.arange(T)).all(), "every sampled iteration: a permutation"
    rounds = n_it // every
    even, odd = rounds // 2, rounds - rounds // 2          # rounds 1 .. rounds: the odd ones come first
    for j in range(T - 1):
        assert out["swaps"][j, 0] == (even if j % 2 == 0 else odd), j
        assert 0 <= out["swaps"][j, 1] <= out["swaps"][j, 0]
    assert out["swaps"][:, 1].sum() > 0 and np.isfinite(out["margin"])
    # the likelihood of the ladder buffer at position 0 is the cold row's
    np.testing.assert_array_equal(out["ladder"][:, 0, 1], [r[2] for r in out["mcmc"]])
    moved = (who != np.arange(T)).any(axis=1)
    assert moved.any() and not moved[0], "the replicas start at their own position and move"


# ---- mc3.py ---------------------------------------------------------------------------------------------------------------------
def test_ladder_betas():
    from literate_amd import mc3
    assert mc3.ladder_betas(1, 0.1) == [1.0]
    b = mc3.ladder_betas(4, 0.5)
    assert b == [1.0, 1 / 1.5, 1 / 2.0, 1 / 2.5] == ref.ladder_betas(4, 0.5) and b[0] == 1.0
    b = mc3.ladder_betas(8, 0.1)
    assert len(b) == 8 and all(x > y > 0 for x, y in zip(b, b[1:]))
    for T, dt, word in ((0, 0.1, "1 to 8 temperatures"), (9, 0.1, "1 to 8 temperatures"), (4, 0.0, "positive"), (4, -1.0, "positive"),
                        (4, float("nan"), "positive")):
        with pytest.raises(ValueError, match=word):
            mc3.ladder_betas(T, dt)


def cli_args(extra=()):
    import LiteRateForward as LRF
    return LRF.build_parser().parse_args(list(extra))


def test_the_flags_and_their_defaults():
    a = cli_args(["-d", "x.tsv"])
    assert (a.mc3, a.mc3_dt, a.mc3_every) == (1, 0.1, 100)
    a = cli_args(["-d", "x.tsv", "--mc3", "4", "--mc3_dt", "0.3", "--mc3_every", "20"])
    assert (a.mc3, a.mc3_dt, a.mc3_every) == (4, 0.3, 20)


def test_the_argument_errors_each_name_the_flag():
    from literate_amd import mc3
    ok = cli_args(["-d", "x.tsv", "--mc3", "4", "--chains", "4"])
    assert mc3.arg_error(ok) is None and mc3.arg_error(cli_args(["--replicates", "x*.tsv", "--mc3", "2"])) is None
    seen = set()
    for flag in ("ppc", "ppc_age", "ade", "ade_joint", "waic", "loo"):
        err = mc3.arg_error(cli_args(["-d", "x.tsv", "--mc3", "4", "--" + flag, "0.2"]))
        assert err.startswith("--%s " % flag) and err.endswith("not with --mc3"), err
        seen.add(err)
    for extra, word in ((["--checkpoint", "c.npz"], "--checkpoint"), (["--init_shifts", "3"], "--init_shifts"), (["-rm_first_bin", "1"], "-rm_first_bin 1"),
                        (["--chains", "0"], "--chains"), (["--mc3_dt", "0"], "--mc3_dt"), (["--mc3_every", "-1"], "--mc3_every"),
                        (["--replicates", "y*.tsv"], "not on both")):
        err = mc3.arg_error(cli_args(["-d", "x.tsv", "--mc3", "4"] + extra))
        assert err and word in err and "--mc3" in err and "\n" not in err, extra
        seen.add(err)
    for T in ("0", "9", "-2"):
        assert "1 to 8 temperatures" in mc3.arg_error(cli_args(["-d", "x.tsv", "--mc3", T]))
    assert "needs a data file" in mc3.arg_error(cli_args(["--mc3", "4"]))
    assert "WORLD_SIZE is 4" in mc3.arg_error(ok, world=4) and "--mc3" in mc3.arg_error(ok, world=4)
    assert len(seen) == 13, "one sentence each"


def test_the_command_line_goes_through_the_replicate_path(tmp_path, monkeypatch):
    """the device seam replaced: replicates.run is recorded, not run"""
    import LiteRateForward as LRF
    from literate_amd import mc3, replicates
    calls = []
    monkeypatch.setattr(replicates, "run", lambda args, parse=None, **kw: calls.append((args, parse, kw)) or 0)
    d = tmp_path / "sub"
    d.mkdir()
    for name in ("a_1.tsv", "a_2.tsv"):
        (d / name).write_text("id\tts\tte\n0\t1\t5\n")
    LRF.main(["-d", str(d / "a_1.tsv"), "--mc3", "4", "--mc3_dt", "0.5", "--chains", "3", "-n", "100"])
    args, parse, kw = calls.pop()
    assert parse is LRF.parse_data and kw["files"] == [str(d / "a_1.tsv")] and kw["name"] == "a_1_BD" and args.chains == 3
    assert callable(kw["engine"]) and callable(kw["finish"])
    LRF.main(["--replicates", str(d / "a_*.tsv"), "--mc3", "2", "--chains", "2", "-n", "100", "-model_BDI", "2"])
    args, parse, kw = calls.pop()
    assert kw["files"] == [str(d / "a_1.tsv"), str(d / "a_2.tsv")] and kw["name"] is None
    # without --mc3, or with --mc3 1, the program takes the path it took: replicates.run without the new keywords
    LRF.main(["--replicates", str(d / "a_*.tsv"), "--chains", "2", "-n", "100"])
    assert calls.pop()[2] == {}
    LRF.main(["--replicates", str(d / "a_*.tsv"), "--chains", "2", "-n", "100", "--mc3", "1"])
    assert calls.pop()[2] == {} and not calls
    with pytest.raises(SystemExit, match="--waic works on the lineages .* not with --mc3"):
        LRF.main(["-d", str(d / "a_1.tsv"), "--mc3", "4", "--waic", "0.2"])
    with pytest.raises(SystemExit, match="no file matches"):
        LRF.main(["--replicates", str(d / "nothing*.tsv"), "--mc3", "2"])
    assert not calls and mc3.run is not None


def test_the_engine_refuses_a_wide_ladder_on_many_bins_in_a_sentence():
    from literate_amd import _hip, mc3
    reps = types.SimpleNamespace(n_bins=257, R=1)
    with pytest.raises(ValueError, match="257 time bins: a ladder of more than 4 temperatures holds at most 256"):
        mc3.TemperedEngine(reps, 1, betas=mc3.ladder_betas(5, 0.1))
    assert mc3.WIDE_MAX_BINS == _hip.LR_RJMC3_WIDE_MAX_BINS == 256


def test_round_trips_and_the_table(tmp_path):
    from literate_amd import mc3
    # ladder 0: replica 0 walks 0 -> 2 -> 0 -> 2 -> 0 (two trips), replica 1 is cold at samples 1, 2, hot at 4, cold at 5 (one),
    # replica 2 starts hot, is cold at sample 3 and hot again at 6 (none: a trip starts cold); ladder 1: nothing moves
    walk = [[0, 1, 2], [1, 0, 2], [1, 2, 0], [2, 1, 0], [0, 2, 1], [1, 2, 0], [0, 1, 2]]          # per sample: replica at position j
    lad = np.zeros((len(walk), 2, 3, 4))
    for s, w in enumerate(walk):
        lad[s, 0, :, 0], lad[s, 1, :, 0] = w, [0, 1, 2]
    # replica 0: cold at samples 0, 4, 6; hot at samples 2, 3, 5 -> trips completed at samples 4 and 6
    assert mc3.round_trips(lad).tolist() == [3, 0]
    assert mc3.round_trips(lad[:4]).tolist() == [0, 0] and mc3.round_trips(np.zeros((5, 3, 1, 4))).tolist() == [0, 0, 0]
    eng = types.SimpleNamespace(n_chains=2, T=3, swap_every=10, round_trips=lambda: np.array([2, 0]),
                                swap_table=lambda: dict(beta_cold=np.array([1.0, 0.5]), beta_hot=np.array([0.5, 0.25]),
                                                        proposed=np.array([10, 8]), accepted=np.array([5, 0]), rate=np.array([0.5, 0.0])))
    path = str(tmp_path / "x_MC3.tsv")
    mc3.write_mc3_table(path, eng)
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].startswith("# 2 ladders of 3 temperatures") and lines[1].split("\t") == ["pair", "beta_cold", "beta_hot", "proposed", "accepted", "rate"]
    assert lines[2].split("\t") == ["0", "1.0", "0.5", "10", "5", "0.5"] and lines[3].split("\t")[3:] == ["8", "0", "0.0"]
    assert lines[5] == "ladder\tround_trips" and lines[6:] == ["0\t2", "1\t0"]


# ---- the header, the binding, the build, the documents --------------------------------------------------------------------------
def header():
    with open(os.path.join(ROOT, "include", "literate_hip_rjmc3.h")) as f:
        text = f.read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_the_header_the_binding_and_the_build_agree():
    from literate_amd import _hip, build
    text, body = header()
    consts = {k: int(v) for k, v in re.findall(r"#define (LR_RJMC3_\w+) (\d+)", text)}
    assert consts == dict(LR_RJMC3_MAX_TEMPS=_hip.LR_RJMC3_MAX_TEMPS, LR_RJMC3_S_POS=_hip.LR_RJMC3_S_POS, LR_RJMC3_LADDER_W=_hip.LR_RJMC3_LADDER_W,
                          LR_RJMC3_WIDE_MAX_BINS=_hip.LR_RJMC3_WIDE_MAX_BINS)
    assert (consts["LR_RJMC3_MAX_TEMPS"], consts["LR_RJMC3_S_POS"], consts["LR_RJMC3_LADDER_W"]) == (8, 9, 4)
    with open(os.path.join(ROOT, "literate_amd", "csrc", "lr_device.h")) as f:
        dev = f.read()
    assert re.search(r"#define LR_P_INIT 10\n#define LR_P_SWAP 11\b", dev) and _hip.LR_P_SWAP == ref.P_SWAP == 11
    from oracle import philox as px
    used = {v for k, v in vars(px).items() if k.startswith("P_")}
    assert ref.P_SWAP not in used and ref.P_SWAP not in (16, 17, 18, 19, 32, 33, 34, 35), "no existing address is reused"
    decl = {m.group(1): [" ".join(a.split()) for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(lr_rjmc3_\w+)\s*\(([^;{}]*?)\)\s*;", body, flags=re.S)}
    assert set(decl) == {"lr_rjmc3_init", "lr_rjmc3_steps"}
    kinds = {"const lr_rjmc3_problem*": C.POINTER(_hip.Rjmc3Problem), "int64_t": _hip.c_i64, "int32_t": _hip.c_i32, "double*": _hip.c_vp,
             "const double*": _hip.c_vp, "const int32_t*": _hip.c_vp}
    for name, args in decl.items():
        res, got = _hip.SIGNATURES[name]
        assert res is _hip.c_i32 and got == [kinds[a.rsplit(" ", 1)[0]] for a in args], name
        assert "stream" not in args[-1], "the stream rides in the descriptor"
    # the descriptor: every field of lr_rjbin_problem in its order, then the ladder's, the stream last
    struct = re.search(r"typedef struct lr_rjmc3_problem \{(.*?)\} lr_rjmc3_problem;", body, flags=re.S).group(1)
    fields = []
    for stmt in struct.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            typ, names = re.match(r"(.*?)\s+(\w+(?:\s*,\s*\w+)*)$", stmt).groups()
            fields += [(n.strip(), typ) for n in names.split(",")]
    want = {"int32_t": _hip.c_i32, "int64_t": _hip.c_i64, "uint64_t": C.c_uint64, "double": _hip.c_f64}
    assert [(n, want.get(t, _hip.c_vp)) for n, t in fields] == [(n, t) for n, t in _hip.Rjmc3Problem._fields_]
    assert [f for f in _hip.Rjmc3Problem._fields_ if f[0] not in ("betas", "swaps", "T", "swap_every")] == list(_hip.RjbinProblem._fields_)
    assert fields[-1] == ("stream", "void*") and [n for n, _ in fields[-5:-1]] == ["betas", "swaps", "T", "swap_every"]
    assert "lr_rjmc3.hip" in build.SOURCES and "lr_rjbin_iter.h" in build.HEADERS and any(h.endswith("literate_hip_rjmc3.h") for h in build.HEADERS)
    # the iteration exists once: both kernels call the header's, neither file holds the acceptance test itself
    src = {}
    for name in ("lr_rjbin.hip", "lr_rjmc3.hip", "lr_rjbin_iter.h"):
        with open(os.path.join(ROOT, "literate_amd", "csrc", name)) as f:
            src[name] = f.read()
    assert "lr_rjbin_iterate<BPL, false>" in src["lr_rjbin.hip"] and "lr_rjbin_iterate<BPL, true>" in src["lr_rjmc3.hip"]
    assert src["lr_rjbin_iter.h"].count(">= log_u") == 1 and ">= log_u" not in src["lr_rjbin.hip"] + src["lr_rjmc3.hip"]
    assert "atomicAdd" not in src["lr_rjmc3.hip"] and src["lr_rjmc3.hip"].count("__syncthreads()") == 1
    # neither entry point has `void* stream` last: the counted set is what it was
    assert len(S.stream_entry_points()) == 38 and not any(n.startswith("lr_rjmc3") for n in S.stream_entry_points())
    # the order of the errors is written down
    assert "Errors before any launch, in this order" in text and "LR_RJMC3_WIDE_MAX_BINS with T > 4" in text


def test_the_docs_name_the_new_flag_and_symbols():
    for path, words in (("README.md", ("--mc3",)), ("DESIGN.md", ("lr_rjmc3", "LR_P_SWAP", "lr_rjbin_iter.h")),
                        ("INTEGRATION.md", ("literate_hip_rjmc3.h", "lr_rjmc3_init", "lr_rjmc3_steps"))):
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for w in words:
            assert w in text, (path, w)
