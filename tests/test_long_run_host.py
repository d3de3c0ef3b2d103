"""The host side of the long-run tests (tests/helpers/long_run.py, tests/test_hip_long_run.py): no GPU.

   1. the draws shims forward every public draw method of every draws class they wrap, and refuse one they do not know;
   2. the 32-bit words of a 64-bit counter, as the engines' integer state holds them;
   3. ops.rows_due against lr_rows_due's arithmetic (csrc/lr_internal.h) and a count, at the offsets and their cuts;
   4. the log writer on a row of iteration 2^32 + 5: an integer column, through lr_format_rows and through Python's formatter;
   5. the seeds of the GPU cases run through the restatements alone: no acceptance or swap decision within 1e-6 of a tie (the
      margin and the practice are tests/test_hip_mc3.py's), the rows finite, both start parities of lr_rjmc3's swap rounds met;
   6. power: for every sampler the same restatement drawing from a broken counter - the high word dropped at 2^32, the low
      word sign-extended at 2^31 (long_run.fault_of) - gives the same rows below the boundary and other rows from it on, so a
      kernel with that fault cannot pass the GPU tests.  (Both offsets lie below 2^32, so "the run at N mod 2^32" is the run
      itself: the fault is applied per iteration, which is what a kernel would do.)
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import long_run as LR          # noqa: E402

OFFSETS = LR.OFFSETS


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
class Spy:
    """records the arguments of whatever method is called on it"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **kw: self.calls.append((name, a, kw)) or name


def draws_classes():
    from helpers import adej_ref
    from oracle import dd_mcmc_oracle as ddo
    from oracle import mcmc_oracle as mo
    from oracle import trend_mcmc_oracle as tro
    return {"mcmc": mo.PhiloxDraws, "dd": ddo.PhiloxDraws, "trend": tro.PhiloxDraws, "adej": adej_ref.PhiloxDraws}


def public_methods(cls):
    return sorted(n for n in dir(cls) if not n.startswith("_") and callable(getattr(cls, n)))


@pytest.mark.parametrize("which", ["mcmc", "dd", "trend", "adej"])
def test_1_remapped_draws_forwards_every_public_draw_method(which):
    cls = draws_classes()[which]
    names = public_methods(cls)
    assert names and "accept" in names and "move" in names
    f = lambda it: 3 * it + 7
    for name in names:
        assert name in LR.ADDRESSED | LR.UNADDRESSED, "%s.PhiloxDraws.%s: a draw method RemappedDraws does not know" % (which, name)
        spy = Spy()
        got = getattr(LR.RemappedDraws(spy, f), name)
        if name in LR.UNADDRESSED:
            assert got() == name and spy.calls == [(name, (), {})]
        else:
            assert got(5, "a", b=2) == name and spy.calls == [(name, (22, "a"), {"b": 2})]
    # the real thing: the same numbers as the wrapped object at the mapped address
    real = cls(11, 3)
    assert LR.RemappedDraws(real, LR.engine_map(OFFSETS[1])).accept(2) == real.accept(OFFSETS[1] + 2)
    assert LR.RemappedDraws(real, LR.engine_map(OFFSETS[1])).accept(0) == real.accept(0) != real.accept(OFFSETS[1])
    assert real.accept(5) != real.accept(2 ** 32 + 5) and real.accept(2 ** 31 + 5) != real.accept(LR.sign_extend(2 ** 31 + 5))


def test_1_an_unknown_method_is_refused():
    for shim in (LR.RemappedDraws(Spy(), lambda it: it), LR.PendingFirst(Spy(), "dd", lambda it: it)):
        with pytest.raises(AttributeError, match="does not know"):
            shim.some_new_draw
    with pytest.raises(AttributeError):
        LR.PendingFirst(Spy(), "dd", lambda it: it).init_rates


@pytest.mark.parametrize("kind", ["dd", "trend"])
def test_1_pending_first_shifts_the_loop_by_one_and_proposes_the_state_itself_first(kind):
    names = [n for n in public_methods(draws_classes()[kind])]
    assert set(names) <= LR.ADDRESSED
    f = LR.engine_map(OFFSETS[0])
    for name in names:
        spy = Spy()
        assert getattr(LR.PendingFirst(spy, kind, f), name)(1, [0.5, 0.5]) == name and spy.calls == [(name, (0, [0.5, 0.5]), {})]
        spy = Spy()
        getattr(LR.PendingFirst(spy, kind, f), name)(4, [0.5, 0.5])
        assert spy.calls == [(name, (OFFSETS[0] + 3, [0.5, 0.5]), {})]
    first = LR.PendingFirst(Spy(), kind, f)
    ff, u = first.multiplier(0, np.ones(6) / 6)
    assert not ff.any() and (u == 0.5).all() and 0 < first.accept(0) < 1
    assert first.move(0) == ((0.0, 1.0) if kind == "dd" else 1.0)
    with pytest.raises(AssertionError):
        first.normal(0, 0.2) if kind == "dd" else first.normal_vec(0, np.ones(6), 0.001)


@pytest.mark.parametrize("name", ["E", "F"])
def test_1_the_parametric_reference_starts_from_the_initial_state_and_counts_from_the_offset(name):
    """local iteration 0 of PendingFirst uses no draw and leaves the state alone: run to a single row, two keys give the same
    row, and it is the oracle's initial state (its posterior the sum of its likelihood and prior columns)"""
    from oracle import dd_mcmc_oracle as ddo
    from oracle import trend_mcmc_oracle as tro
    from helpers import chain_edges as CE
    kind = CE.KIND[CE.CONFIGS[name].sampler]
    _, _, bins, trend = CE.param_data(name)
    o, p, nsp, nex, dt, t_range = bins
    rows = []
    for key in (0, 5):
        with np.errstate(all="ignore"):
            if kind == "dd":
                rows.append(ddo.run_dd_mcmc(nsp, nex, dt, t_range, o, p, 2, 2, LR.PendingFirst(ddo.PhiloxDraws(1, key), kind, None), 1, 1)[0])
            else:
                rows.append(tro.run_trend_mcmc(nsp, nex, dt, trend, LR.PendingFirst(tro.PhiloxDraws(1, key), kind, None), 1, 1)[0])
    assert np.array_equal(rows[0], rows[1], equal_nan=True)
    want = ddo.initial_args(o, p) if kind == "dd" else np.array([.1, .1, 0, 0, 1, 1])
    logged = rows[0][6:6 + len(want)].copy()
    if kind == "dd":
        logged[2] -= o
        logged[4] -= logged[3]
    assert np.allclose(logged, want, rtol=1e-15, atol=0)
    got = LR.param_engine_rows(name, 0, OFFSETS[0])
    assert [r[0] for r in got] == list(range(OFFSETS[0], OFFSETS[0] + LR.N_IT)) and np.isfinite(np.array([r[1:6] for r in got])).all()


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
def test_2_the_int32_with_the_same_bits():
    assert LR.as_i32(2 ** 31 + 3) == -(2 ** 31) + 3 and LR.as_u32(-(2 ** 31) + 3) == 2 ** 31 + 3
    assert LR.as_i32(2 ** 31 - 1) == 2 ** 31 - 1 and LR.as_i32(2 ** 32 - 1) == -1 and LR.as_i32(0) == 0
    for word in (0, 1, 2 ** 31 - 24, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 3, 2 ** 32 - 24, 2 ** 32 - 1):
        assert LR.as_i32(word) == int(np.array([word], dtype=np.uint32).view(np.int32)[0]) and LR.as_u32(LR.as_i32(word)) == word
    for n in (OFFSETS[0], OFFSETS[0] + 24, OFFSETS[0] + 60, OFFSETS[1], OFFSETS[1] + 23, OFFSETS[1] + 24, OFFSETS[1] + 60, 2 ** 40 + 2 ** 31):
        lo, hi = LR.split64(n)
        assert -2 ** 31 <= lo < 2 ** 31 and LR.join64(lo, hi) == n
        # engine.py's reassembly of snapshot()["it"]
        I = np.array([lo, hi], dtype=np.int32)
        assert int((I[0].astype(np.int64) & 0xFFFFFFFF) | (I[1].astype(np.int64) << 32)) == n
    assert LR.split64(OFFSETS[0] + 24) == (-2 ** 31, 0) and LR.split64(OFFSETS[1] + 24) == (0, 1) and LR.split64(OFFSETS[1]) == (-24, 0)
    assert LR.boundary(OFFSETS[0]) == 2 ** 31 and LR.boundary(OFFSETS[1]) == 2 ** 32
    assert LR.drop_high(2 ** 32 + 5) == 5 and LR.sign_extend(2 ** 31 + 5) == 2 ** 64 - 2 ** 31 + 5 and LR.sign_extend(2 ** 31 - 1) == 2 ** 31 - 1


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 7, 8])
@pytest.mark.parametrize("N", OFFSETS)
def test_3_rows_due_at_the_offsets(N, s):
    from literate_amd import ops
    it, total = N, 0
    for n in LR.CUTS + (0, LR.N_IT):
        count = sum(1 for i in range(it, it + n) if i % s == 0)
        c_form = (it + n + s - 1) // s - (it + s - 1) // s          # lr_rows_due, in int64_t: far below INT64_MAX - n - s
        assert ops.rows_due(it, n, s) == count == c_form, (it, n, s)
        if n != LR.N_IT:
            it, total = it + n, total + count
    assert it == N + LR.N_IT and total == ops.rows_due(N, LR.N_IT, s) == sum(1 for i in range(N, N + LR.N_IT) if i % s == 0)
    assert s == 7 or total == LR.N_IT // s + (1 if LR.N_IT % s else 0)          # N is a multiple of 8


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def test_4_the_log_line_of_iteration_2_32_plus_5_starts_with_an_integer(tmp_path):
    from literate_amd import _hip, logs
    it = 2 ** 32 + 5
    row = np.full(_hip.LR_TRACE_W, np.nan)
    row[:13] = [it, -120.5, -100.25, -20.25, 0.3, 0.2, 2, 1, 0.0, 24.5, 1.0, 1.5, 2.0]
    H, K = _hip.LR_TRACE_HEAD, _hip.LR_KMAX
    row[H:H + 2], row[H + K], row[H + 2 * K - 1] = [0.25, 0.35], 11.5, 0.2
    rows = np.stack([row, row])
    rows[1, 0] = it + 8
    lm, ls, le = logs._chain_lines(rows, None, 24, False, 0.0)                     # Python's formatter
    assert lm[0].startswith("4294967301\t-120.5\t") and lm[1].startswith("4294967309\t") and ls[0] == "0.25\t0.35\t11.5\n"
    data = tmp_path / "d.tsv"
    (tmp_path / "literate_mcmc_logs").mkdir()
    w = logs.ChainLogWriter(str(data), 0, "", 1)
    w.append(rows[:, None, :])                                                     # whichever formatter the writer takes
    with open(w.paths[0]["mcmc"]) as f:
        lines = f.readlines()
    assert lines[1:] == lm and lines[1].split("\t")[0] == str(it) and "e" not in lines[1].split("\t")[0] and "." not in lines[1].split("\t")[0]
    if os.environ.get("LR_LOG_FORMAT", "native") != "python":
        assert logs._native() is not None, "the built library formats the logs"
        head = np.ascontiguousarray(rows[:, :13])
        text = logs._native_format(head.reshape(-1), np.arange(3, dtype=np.int64) * 13, logs._MCMC_INT_COLS).decode()
        assert text == "".join(lm), text                                            # lr_format_rows' integer columns


# ---- 5, 6 -------------------------------------------------------------------------------------------------------------------
def head_rows(outs):
    """[rows, chains, 13 + ...] of run_mcmc-style outs, rates and times appended where the lengths allow: compared exactly"""
    from test_hip_replicates import want_rows
    return want_rows(outs)


@pytest.mark.parametrize("N", OFFSETS)
@pytest.mark.parametrize("case", sorted(LR.RJBIN_CASES))
def test_5_rjbin_seeds(case, N):
    from test_hip_replicates import check_oracle_rows
    _, outs, margin = LR.rjbin_reference(case, N)
    check_oracle_rows(outs)
    print("smallest margin of a decision: %.3g" % margin)
    assert margin >= LR.MARGIN
    s = LR.RJBIN_CASES[case][2]
    assert [int(r[0]) for r in outs[0]["mcmc"]] == list(range(N, N + LR.N_IT, s))
    assert sum(o["state"]["accepted"] for o in outs) > LR.N_IT, "the chains move"


@pytest.mark.parametrize("N", OFFSETS)
@pytest.mark.parametrize("T,every", LR.RJMC3_CASES)
def test_5_rjmc3_seeds(T, every, N):
    _, outs, margin = LR.rjmc3_reference(T, every, N)
    assert all(np.isfinite(np.array(o["mcmc"])).all() for o in outs)
    print("smallest margin of a decision: %.3g" % margin)
    assert margin >= LR.MARGIN
    rounds = [n for n in range(N // every, (N + LR.N_IT) // every + 1) if N <= n * every - 1 < N + LR.N_IT]
    assert rounds[0] == LR.first_round(N, every)
    for o in outs:
        want = [sum(1 for n in rounds if n % 2 == j % 2) for j in range(T - 1)]
        assert o["swaps"][:, 0].tolist() == want and o["swaps"][:, 1].sum() > 0, (o["swaps"].tolist(), want)


def test_5_both_start_parities_of_the_swap_rounds_occur():
    """lr_rjmc3 derives `par` of a launch from ((it0 + until_swap + 1) / swap_every) & 1.  The first round's number is odd at
    both offsets for swap_every 1 and 5 (N + 1 is odd; (2^31 - 23) / 5 = 429496725, (2^32 - 21) / 5 = 858993455); swap_every
    3 makes it 715827875 at 2^31 - 24 and 1431655758 at 2^32 - 24."""
    first = {(N, e): LR.first_round(N, e) for N in OFFSETS for e in (1, 5, 3)}
    assert first[(OFFSETS[0], 5)] == 429496725 and first[(OFFSETS[1], 5)] == 858993455
    assert first[(OFFSETS[0], 3)] == 715827875 and first[(OFFSETS[1], 3)] == 1431655758
    assert {v & 1 for v in first.values()} == {0, 1} and {e for _, e in LR.RJMC3_CASES} == {1, 5, 3}


@pytest.mark.parametrize("N", OFFSETS)
def test_5_tmlik_and_adej_seeds(N):
    rows, state, margin = LR.tmlik_reference(N)
    assert margin >= LR.MARGIN and np.isfinite(rows).all() and np.array_equal(rows[0, :, 0, 0, 0], np.arange(N, N + LR.N_IT))
    runs, margin = LR.adej_reference(N)
    assert margin >= LR.MARGIN and all(np.array_equal(r["rows"][:, 0], np.arange(N, N + LR.N_IT)) for r in runs.values())
    rows, _ = LR.mlik_reference(N)
    assert np.isfinite(rows[..., :3]).all() and np.array_equal(rows[:, 0, 0, 0], np.arange(N, N + LR.N_IT))


@pytest.mark.parametrize("N", OFFSETS)
def test_6_power_of_the_stepping_samplers(N):
    fault = LR.fault_of(N)
    its = np.arange(N, N + LR.N_IT)
    for case in ("bins40-m2", "bins40-s8"):
        good, bad = LR.rjbin_reference(case, N)[1], LR.rjbin_reference(case, N, fault=fault)[1]
        LR.differs_from(N, [r[0] for r in good[0]["mcmc"]], head_rows(good)[:, :, :13], head_rows(bad)[:, :, :13])
    good, bad = LR.rjmc3_reference(4, 5, N)[1], LR.rjmc3_reference(4, 5, N, fault=fault)[1]
    LR.differs_from(N, its, np.array(good[0]["mcmc"]), np.array(bad[0]["mcmc"]))
    LR.differs_from(N, its, good[1]["ladder"], bad[1]["ladder"])
    LR.differs_from(N, its, LR.tmlik_reference(N)[0].transpose(1, 0, 2, 3, 4), LR.tmlik_reference(N, fault)[0].transpose(1, 0, 2, 3, 4))
    LR.differs_from(N, its, LR.mlik_reference(N)[0], LR.mlik_reference(N, fault)[0])
    good, bad = LR.adej_reference(N)[0], LR.adej_reference(N, fault)[0]
    for c in good:
        LR.differs_from(N, its, good[c]["rows"], bad[c]["rows"])


@pytest.mark.parametrize("N", OFFSETS)
@pytest.mark.parametrize("name", ["A", "B", "C", "E", "F"])
def test_6_power_of_the_engine_reference(name, N):
    """the oracle loop on engine_map's addresses against the same loop on a broken counter's; and the remapping itself has
    power: the rows differ from the loop that draws iteration N at address N instead of 0"""
    from helpers import chain_edges as CE
    case = LR.EngineCase(name, "launch", LR.N_CHAINS, 1, False)
    fault = LR.fault_of(N)
    for c in (0, 5):
        good, bad = LR.engine_rows(case, c, N), LR.engine_rows(case, c, N, fault)
        assert [r[0] for r in good] == list(range(N, N + LR.N_IT))
        LR.differs_from(N, [r[0] for r in good], np.array([r[:6] for r in good]), np.array([r[:6] for r in bad]))
    if CE.CONFIGS[name].sampler == 0:
        rows8 = LR.rj_engine_rows(name, 0, N, 8)
        assert [r[0] for r in rows8] == list(range(N, N + LR.N_IT, 8))
        assert all(np.array_equal(r, good8) for r, good8 in zip(rows8, LR.rj_engine_rows(name, 0, N, 1)[::8]))


def test_5_the_key_wrap_seeds():
    _, outs, margin = LR.rjbin_reference("bins40-m2", 0, LR.RJBIN_SEED, LR.WRAP_CHAIN0, None, 4)
    assert margin >= LR.MARGIN and all(np.isfinite(np.array(o["mcmc"])).all() for o in outs)
    # the keys are the wrapped ones: chains 2, 3 of the run at 2^32 - 2 are chains 0, 1 of the run at chain0 = 0
    low = LR.rjbin_reference("bins40-m2", 0, LR.RJBIN_SEED, 0, None, 4)[1]
    assert all(np.array_equal(np.array(outs[2 + c]["mcmc"]), np.array(low[c]["mcmc"])) for c in range(2))
    assert not np.array_equal(np.array(outs[0]["mcmc"]), np.array(low[2]["mcmc"]))
    _, outs, margin = LR.rjmc3_reference(4, 5, 0, LR.RJMC3_SEED, LR.WRAP_CHAIN0)
    assert margin >= LR.MARGIN and all(np.isfinite(np.array(o["mcmc"])).all() for o in outs)


@pytest.mark.parametrize("case", LR.engine_cases(), ids=[LR.engine_case_id(c) for c in LR.engine_cases()])
def test_6_the_planner_gives_each_engine_case_its_family(case):
    """on the host, for a device of 256 compute units: the layout of every case names the family the case is for"""
    from helpers import chain_edges as CE
    from helpers import edges as E
    cfg = CE.CONFIGS[case.config]
    rc, lay = E.query(cfg.model, cfg.sampler, not cfg.general, cfg.n_bins, case.chains, CE.n_lineages(case.config), E.ENGINES[case.engine])
    assert rc == 0
    got = (lay.persistent, lay.packed_scan, lay.streaming)
    want = {"persistent4": (2, 0, 0), "persistent2": (1, 0, 0), "spec": (3, 0, 0), "packed": (0, 1, 0), "stream": (0, 0, 1), "launch": (0, 0, 0)}
    assert got == want[case.engine], (case, got)
    assert lay.pipelined == (1 if case.chains == LR.PIPELINED_CHAINS else 0)


def test_6_the_engine_cases_are_the_written_set():
    cases = LR.engine_cases()
    assert len(cases) == LR.N_ENGINE_CASES == len(set(cases))
    pairs = {(c.config, c.engine) for c in cases}
    assert not pairs & set(LR.EXCLUDED) and all(not LR.runs(e, n) for n, e in LR.EXCLUDED)
    for name in "AB":
        assert {e for n, e in pairs if n == name} | {e for n, e in LR.EXCLUDED if n == name} == set(LR.FORCED)
    assert {e for n, e in pairs if n == "C"} == {"launch", "persistent4"}
    assert {e for n, e in pairs if n == "E"} == {"launch", "persistent4", "persistent2", "spec"}
    assert {e for n, e in pairs if n == "F"} == {"launch", "persistent4", "spec"}
    assert sorted(c.engine for c in cases if c.s_freq == 8) == sorted(LR.FORCED) and sum(c.generic for c in cases) == 1
    assert set(LR.FORCED) == {"launch", "persistent4", "persistent2", "spec", "stream", "packed"}
