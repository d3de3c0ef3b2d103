"""The host side of the RJ sampler on replicate data sets (include/literate_hip_rjbin.h, literate_amd/replicates.py), no GPU:
the header against the ctypes binding and the build; load_replicates' parsing, window check and messages with the GPU binning
replaced by the oracle's (lo.bin_events_cli, lo.bin_events_dead); the chain-to-replicate mapping, the log names, the argument
errors, the expansion and ordering of --replicates; the table of <NAME>_div_replicates.tsv.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import stream_cases as S
from oracle import literate_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def header():
    with open(os.path.join(ROOT, "include", "literate_hip_rjbin.h")) as f:
        text = f.read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_the_header_the_binding_and_the_build_agree():
    from literate_amd import _hip, build, ops
    text, body = header()
    consts = dict(re.findall(r"#define (LR_RJBIN_\w+) (\d+)", text))
    assert int(consts["LR_RJBIN_MAX_BINS"]) == _hip.LR_RJBIN_MAX_BINS == 512
    assert int(consts["LR_RJBIN_STATE_W"]) == _hip.LR_RJBIN_STATE_W == (int(consts["LR_RJBIN_ROW_SCALARS"]) + 1) * _hip.LR_ROW
    assert {k: int(consts["LR_RJBIN_ROW_" + k.upper() if k != "scalars" else "LR_RJBIN_ROW_SCALARS"]) for k in ops.RJBIN_ROWS} == ops.RJBIN_ROWS
    for name, slot in (("likA", "LIKA"), ("priorA", "PRIORA"), ("priorPoiA", "PRIORPOIA"), ("Gamma_rate_l", "GRATE_L"), ("Gamma_rate_m", "GRATE_M"),
                       ("Poi_lambda", "POI"), ("K_l", "KL"), ("K_m", "KM"), ("accepted", "ACCEPTED")):
        assert ops.RJBIN_SCALARS[name] == int(consts["LR_RJBIN_S_" + slot]), name
    decl = {m.group(1): [" ".join(a.split()) for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint\s+(lr_rjbin_\w+)\s*\(([^;{}]*?)\)\s*;", body, flags=re.S)}
    assert set(decl) == {"lr_rjbin_init", "lr_rjbin_steps"}
    kinds = {"const lr_rjbin_problem*": C.POINTER(_hip.RjbinProblem), "int64_t": _hip.c_i64, "int32_t": _hip.c_i32, "double*": _hip.c_vp,
             "const double*": _hip.c_vp, "const int32_t*": _hip.c_vp}
    for name, args in decl.items():
        res, got = _hip.SIGNATURES[name]
        assert res is _hip.c_i32 and got == [kinds[a.rsplit(" ", 1)[0]] for a in args], name
        assert args[-1] != "void* stream" and "stream" not in args[-1], "the stream rides in the descriptor"
    assert len(decl["lr_rjbin_init"]) == 7 and len(decl["lr_rjbin_steps"]) == 7
    # the descriptor, field by field
    struct = re.search(r"typedef struct lr_rjbin_problem \{(.*?)\} lr_rjbin_problem;", body, flags=re.S).group(1)
    fields = []
    for stmt in struct.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            typ, names = re.match(r"(.*?)\s+(\w+(?:\s*,\s*\w+)*)$", stmt).groups()
            fields += [(n.strip(), typ) for n in names.split(",")]
    want = {"int32_t": _hip.c_i32, "int64_t": _hip.c_i64, "uint64_t": C.c_uint64, "double": _hip.c_f64}
    assert [(n, want.get(t, _hip.c_vp)) for n, t in fields] == [(n, t) for n, t in _hip.RjbinProblem._fields_]
    assert fields[-1] == ("stream", "void*")
    assert "lr_rjbin.hip" in build.SOURCES and any(h.endswith("literate_hip_rjbin.h") for h in build.HEADERS)
    with open(os.path.join(ROOT, "literate_amd", "csrc", "lr_rjbin.hip")) as f:
        src = f.read()
    assert '#include "lr_chain.h"' in src and "lr_step.h" not in src.replace("lr_step.h's addresses", "")
    assert "__syncthreads" not in src and "__shared__" not in src, "no barrier, no LDS"
    assert "atomicAdd" not in src, "no floating-point atomics"
    # neither entry point has `void* stream` last, and the header is not among the five the stream contract test reads: the
    # counted set is what it was
    assert len(S.stream_entry_points()) == 38 and not any(n.startswith("lr_rjbin") for n in S.stream_entry_points())


def test_the_library_exports_both_entry_points_when_it_is_built():
    from literate_amd import _hip, build
    assert {"lr_rjbin_init", "lr_rjbin_steps"} <= set(_hip.SIGNATURES), "_hip.py binds them"
    if not os.path.exists(build.LIB):
        return          # (nothing to look at before a build; __graft_entry__.build() makes one)
    lib = C.CDLL(build.LIB)
    assert lib.lr_rjbin_init is not None and lib.lr_rjbin_steps is not None
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True)
    if out.returncode == 0:
        names = {l.split()[-1] for l in out.stdout.splitlines() if l.split()}
        assert {"lr_rjbin_init", "lr_rjbin_steps"} <= names


# ---- load_replicates ----------------------------------------------------------------------------------------------------------
def write_tsv(path, ts, te, clade=False):
    with open(path, "w") as f:
        f.write("clade\tid\tts\tte\n" if clade else "id\tts\tte\n")
        for i, (a, b) in enumerate(zip(ts, te)):
            f.write(("0\t" if clade else "") + "%d\t%d\t%d\n" % (i, a, b))


@pytest.fixture
def cpu_binning(monkeypatch):
    """the GPU binning replaced by the oracle's loops (the windows are the CLI's: every file of a set shares them)"""
    from literate_amd import replicates

    def fake_bin(ts, te, t0, n_bins):
        lo_, sp, ex, br = lo.bin_events_cli(ts, te)
        out = [np.zeros(n_bins), np.zeros(n_bins), np.zeros(n_bins)]
        off = lo_ - int(t0)                      # (a subset may start later and end earlier than the window)
        for o, x in zip(out, (sp, ex, br)):
            o[off:off + len(x)] = x[:n_bins - off]
        return out

    def fake_dead(ts, te, t0, n_bins, end_time):
        ex, br = lo.bin_events_dead(ts, te, end_time)
        assert len(ex) == n_bins and int(np.min(ts)) == int(t0)
        return ex.astype(float), br
    monkeypatch.setattr(replicates, "_bin", fake_bin)
    monkeypatch.setattr(replicates, "_bin_dead", fake_dead)
    return replicates


def files_of(tmp_path, n=3, shift_last=0, first=1950):
    rng = np.random.default_rng(4)
    ts = np.sort(rng.integers(first, 1985, 60))
    ts[0] = first
    files = []
    for r in range(n):
        te = np.minimum(ts + rng.integers(0, 20, 60), 1990)
        te[-1] = 1990 + (shift_last if r == n - 1 else 0)
        files.append(str(tmp_path / ("imp_%02d.tsv" % r)))
        write_tsv(files[-1], ts, te)
    return files


def cli_args(extra=()):
    import LiteRateForward as LRF
    return LRF.build_parser().parse_args(["--replicates", "x"] + list(extra))


def test_load_replicates_parses_and_bins_each_file_on_the_common_window(tmp_path, cpu_binning):
    import LiteRateForward as LRF
    files = files_of(tmp_path)
    args = cli_args()
    reps = cpu_binning.load_replicates(files, args, LRF.parse_data)
    assert reps.R == 3 and reps.n_bins == 40 and reps.t0 == 1950 and reps.paths == files and reps.ex_dead is None
    for r, path in enumerate(files):
        a = cli_args()
        a.d = path
        ts, te, root = LRF.parse_data(a)
        t0, sp, ex, br = lo.bin_events_cli(ts, te)
        assert t0 == 1950 and np.array_equal(reps.sp[r], sp) and np.array_equal(reps.ex[r], ex) and np.array_equal(reps.br[r], br)
        assert reps.start_time[r] == ts.min() == 1950.0 and reps.end_time[r] == te.max() == 1990.5 and reps.n_lineages[r] == 60
        eb, ed = reps.empirical(r)
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(eb, sp / br), np.testing.assert_array_equal(ed, ex / br)
    assert not np.array_equal(reps.ex[0], reps.ex[1]), "the imputations differ"
    # -death_jitter goes through parse_data's rules
    j = cpu_binning.load_replicates(files, cli_args(["-death_jitter", "0.25"]), LRF.parse_data)
    assert (j.end_time == 1990.25).all()


def test_load_replicates_model_3_bins_the_dead_subset_on_the_same_windows(tmp_path, cpu_binning):
    import LiteRateForward as LRF
    files = files_of(tmp_path)
    reps = cpu_binning.load_replicates(files, cli_args(["-model_BDI", "3"]), LRF.parse_data)
    assert reps.ex_dead.shape == reps.br_dead.shape == (3, 40)
    for r, path in enumerate(files):
        a = cli_args()
        a.d = path
        ts, te, _ = LRF.parse_data(a)
        ex, br = lo.bin_events_dead(ts, te, te.max())
        assert np.array_equal(reps.ex_dead[r], ex) and np.array_equal(reps.br_dead[r], br)
        assert (reps.br_dead[r] <= reps.br[r] + 1e-12).all() and reps.br_dead[r].sum() < reps.br[r].sum()


def test_load_replicates_refuses_another_window_by_file_name_and_more_than_512_bins(tmp_path, cpu_binning):
    import LiteRateForward as LRF
    files = files_of(tmp_path, shift_last=3)
    with pytest.raises(ValueError, match=r"imp_02\.tsv: its window \[1950, 1993\].*differs from the first replicate's \[1950, 1990\]"):
        cpu_binning.load_replicates(files, cli_args(), LRF.parse_data)
    d = tmp_path / "early"
    d.mkdir()
    early = files_of(d, n=1, first=1949)
    with pytest.raises(ValueError, match=r"early.imp_00\.tsv: its window \[1949, 1990\]"):
        cpu_binning.load_replicates(files[:2] + early, cli_args(), LRF.parse_data)
    long = str(tmp_path / "long.tsv")
    write_tsv(long, [1000, 1200], [1100, 1513])
    with pytest.raises(ValueError, match=r"long\.tsv: 513 time bins; the replicate sampler holds at most 512"):
        cpu_binning.load_replicates([long], cli_args(), LRF.parse_data)
    write_tsv(long, [1000, 1200], [1100, 1512])
    assert cpu_binning.load_replicates([long], cli_args(), LRF.parse_data).n_bins == 512


# ---- mapping, names, arguments ------------------------------------------------------------------------------------------------
def test_the_chain_to_replicate_mapping_and_the_log_names(tmp_path):
    from literate_amd import replicates
    assert [replicates.replicate_of(c, 1) for c in range(4)] == [0, 1, 2, 3]
    assert [replicates.replicate_of(c, 3) for c in range(7)] == [0, 0, 0, 1, 1, 1, 2]
    assert replicates.chains_per_replicate(100, 100) == 1 and replicates.chains_per_replicate(1024, 32) == 32
    for n, r in ((3, 2), (0, 1), (1, 2), (4, 0)):
        with pytest.raises(ValueError, match="must be a multiple of the %d files" % r):
            replicates.chains_per_replicate(n, r)
    assert replicates.default_name(100) == "replicates100"
    path = str(tmp_path / "sub" / "metal_bands_7.tsv")
    one = replicates.replicate_log_paths(path, 0, "", 1)
    assert len(one) == 1 and one[0]["mcmc"] == str(tmp_path / "sub" / "literate_mcmc_logs" / "metal_bands_7_BD_mcmc.log")     # the reference's own
    assert one[0]["div"].endswith("metal_bands_7_BD_div.log")
    two = replicates.replicate_log_paths(path, 2, "_x", 2)
    assert [os.path.basename(p["sp_rates"]) for p in two] == ["metal_bands_7_BDk_x_c0_sp_rates.log", "metal_bands_7_BDk_x_c1_sp_rates.log"]


def test_the_pattern_is_expanded_and_sorted_by_the_program(tmp_path):
    from literate_amd import replicates
    for name in ("b_10.tsv", "b_2.tsv", "a.tsv", "other.txt"):
        (tmp_path / name).write_text("x\n")
    (tmp_path / "d").mkdir()
    (tmp_path / "d" / "c.tsv").write_text("x\n")
    P = lambda *n: [str(tmp_path.joinpath(*x.split("/"))) for x in n]
    assert replicates.expand_pattern(str(tmp_path / "*.tsv")) == P("a.tsv", "b_10.tsv", "b_2.tsv")
    assert replicates.expand_pattern("%s, %s" % (P("b_2.tsv")[0], P("a.tsv")[0])) == P("a.tsv", "b_2.tsv")
    assert replicates.expand_pattern("%s,%s" % (str(tmp_path / "b_*.tsv"), str(tmp_path / "*" / "c.tsv"))) == P("b_10.tsv", "b_2.tsv", "d/c.tsv")
    assert replicates.expand_pattern("%s,%s" % (P("a.tsv")[0], str(tmp_path / "a.*"))) == P("a.tsv"), "a file named twice is one replicate"
    with pytest.raises(ValueError, match="no file matches .*missing"):
        replicates.expand_pattern("%s,%s" % (P("a.tsv")[0], str(tmp_path / "missing*.tsv")))
    with pytest.raises(ValueError, match="no file matches"):
        replicates.expand_pattern(str(tmp_path / "nothing.tsv"))
    with pytest.raises(ValueError, match="no file given"):
        replicates.expand_pattern(" , ")


def test_the_argument_errors_each_say_why():
    from literate_amd import replicates
    ok = cli_args(["--chains", "4"])
    assert replicates.arg_error(ok) is None and ok.replicates_name == ""
    for flag in ("ppc", "ppc_age", "ade", "ade_joint", "waic", "loo"):
        err = replicates.arg_error(cli_args(["--" + flag, "0.2"]))
        assert err.startswith("--%s " % flag) and "one data set" in err and err.endswith("not with --replicates"), err
    for extra, word in ((["--checkpoint", "c.npz"], "--checkpoint"), (["--init_shifts", "3"], "--init_shifts"), (["-d", "x.tsv"], "-d empty"),
                        (["-rm_first_bin", "1"], "-rm_first_bin 1"), (["--chains", "0"], "--chains")):
        err = replicates.arg_error(cli_args(extra))
        assert err and word in err, extra
    assert "WORLD_SIZE is 4" in replicates.arg_error(ok, world=4)
    assert len({why for _, _, why in replicates.ONE_DATA_SET}) == 6


def test_the_command_line_refuses_before_anything_runs(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda a: subprocess.run([sys.executable, os.path.join(ROOT, "LiteRateForward.py")] + a, cwd=str(tmp_path), env=env, capture_output=True,
                                   text=True, timeout=120)
    res = run(["--replicates", "x*.tsv", "--waic", "0.2"])
    assert res.returncode != 0 and "--waic scores the lineages of one data set" in res.stderr
    res = run(["--replicates", "x*.tsv", "-d", "y.tsv"])
    assert res.returncode != 0 and "leave -d empty" in res.stderr
    res = run(["--replicates", str(tmp_path / "x*.tsv")])
    assert res.returncode != 0 and "no file matches" in res.stderr
    (tmp_path / "x1.tsv").write_text("id\tts\tte\n0\t1\t5\n")
    (tmp_path / "x2.tsv").write_text("id\tts\tte\n0\t1\t5\n")
    res = run(["--replicates", str(tmp_path / "x*.tsv"), "--chains", "3"])
    assert res.returncode != 0 and "--chains 3 is the total over all replicates: it must be a multiple of the 2 files" in res.stderr


def test_the_div_replicates_table_is_the_averagers(tmp_path):
    from literate_amd import replicates
    rng = np.random.default_rng(2)
    br = 5.0 + rng.random((4, 7)) * 20
    br[1, 3] = 0.0
    sp, ex = rng.poisson(0.3 * br).astype(float), rng.poisson(0.2 * br).astype(float)
    path = str(tmp_path / "n_div_replicates.tsv")
    replicates.write_div_replicates(path, sp, ex, br)
    with open(path) as f:
        assert f.readline().rstrip("\n").split("\t") == replicates.DIV_HEAD
    tab = np.loadtxt(path, skiprows=1)
    with np.errstate(all="ignore"):
        eb, ed = sp / br, ex / br
    assert tab.shape == (7, 10) and np.array_equal(tab[:, 0], np.arange(7))
    for j, x in enumerate((eb, ed, br)):          # imputation_averager.py: mean, min, max over the files of each vector
        np.testing.assert_array_equal(tab[:, 1 + 3 * j], x.mean(axis=0))
        np.testing.assert_array_equal(tab[:, 2 + 3 * j], x.min(axis=0))
        np.testing.assert_array_equal(tab[:, 3 + 3 * j], x.max(axis=0))
    assert np.isnan(tab[3, 1]) and np.isnan(tab[3, 4]) and tab[3, 8] == 0.0, "a bin without lineage-time in one replicate: 0 / 0 there"


def test_the_docs_name_the_new_header_and_flag():
    for path, words in (("README.md", ("--replicates",)), ("DESIGN.md", ("lr_rjbin",)), ("INTEGRATION.md", ("literate_hip_rjbin.h", "lr_rjbin_steps"))):
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for w in words:
            assert w in text, (path, w)
