"""The host side of the stream-contract tests (tests/helpers/stream_cases.py, tests/test_hip_stream_contract.py), no GPU:

  - COVERS and BLOCKING against the headers: every function of include/*.h whose last parameter is `void* stream` is in
    exactly one of them, neither names a function that does not exist, every sentence of BLOCKING stands verbatim in a
    header, every case is run by the GPU test file, and the blocking entry points are run by a case too;
  - ordered() against a runtime without a device (DeferredRuntime: streams as queues of closures that a delay holds back
    until somebody synchronises): it passes a well-behaved fake and raises the right kind of violation for one that works
    on another pool stream, works on the null stream, joins nothing back, synchronises, uploads first, or ignores its
    input - the fakes the device self-test replays on HIP streams."""
import os
import re

import numpy as np
import pytest

from helpers import stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the tables against the headers --------------------------------------------------------------
def _uncovered(covers):
    declared = set(S.stream_entry_points())
    covered = {e for eps in covers.values() for e in eps}
    return sorted(declared - covered - set(S.BLOCKING))


def test_every_entry_point_that_takes_the_stream_is_covered_or_blocking():
    declared = S.stream_entry_points()
    assert len(declared) == 38 and {"lr_bd_loglik_batch", "lr_mcmc_steps", "lr_ppc_age", "lr_adej_steps", "lr_mlik_estimate",
                                    "lr_ade_profile"} <= set(declared)
    assert set(declared.values()) == {"literate_hip.h", "literate_hip_age.h", "literate_hip_ade.h", "literate_hip_adej.h",
                                      "literate_hip_mlik.h"}
    covered = {e for eps in S.COVERS.values() for e in eps}
    assert covered <= set(declared), "COVERS names functions no header declares: %s" % sorted(covered - set(declared))
    assert set(S.BLOCKING) <= set(declared), "BLOCKING names functions no header declares: %s" % sorted(set(S.BLOCKING) - set(declared))
    assert not covered & set(S.BLOCKING), "both covered and blocking: %s" % sorted(covered & set(S.BLOCKING))
    assert not _uncovered(S.COVERS), "entry points without a case in tests/helpers/stream_cases.py: %s" % _uncovered(S.COVERS)
    ran = {e for eps in S.RUNS_BLOCKING.values() for e in eps}
    assert ran == set(S.BLOCKING), "blocking entry points no case runs: %s" % sorted(set(S.BLOCKING) - ran)


def test_a_case_deleted_from_the_table_is_named():
    for name, eps in S.COVERS.items():
        rest = {k: v for k, v in S.COVERS.items() if k != name}
        elsewhere = {e for v in rest.values() for e in v}
        assert _uncovered(rest) == sorted(set(eps) - elsewhere), name


def test_every_blocking_sentence_stands_in_a_header():
    text = ""
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        with open(os.path.join(ROOT, "include", h)) as f:
            text += f.read()
    flat = " ".join(re.sub(r"\n\s*\*\s?", " ", text).split())          # (comment continuation lines joined)
    for name, sentence in S.BLOCKING.items():
        assert len(sentence) > 40 and " ".join(sentence.split()) in flat, "%s: no header holds %r" % (name, sentence)
        # ... in the comment that stands before the declaration (or, for the two it names, names the function)
        at = flat.index(" ".join(sentence.split()))
        decl = flat.find(name + "(", at)
        assert name in sentence or 0 < decl - at < 1500, name


def test_every_case_is_run_by_the_gpu_test_file():
    import test_hip_stream_contract as T
    assert set(S.COVERS) == set(S.CASES)
    assert {c[0] for c in T.CHILDREN} == set(S.CASES), set(S.CASES) ^ {c[0] for c in T.CHILDREN}
    assert {tuple(c[1:]) for c in T.CHILDREN if c[0] == "engine"} == {tuple(r) for r in S.ENGINE_RUNS}
    assert {r[0] for r in S.ENGINE_RUNS} == set(S.ENGINES) and "partitioned" in S.ENGINES
    assert ("persistent4", "unit", "dd") in S.ENGINE_RUNS and ("spec1", "unit", "trend") in S.ENGINE_RUNS
    assert {c[1] for c in T.CHILDREN if c[0] == "loglik"} == set(S.LOGLIK_SHAPES)
    for walk in ("waic", "loo"):
        assert {c[1] for c in T.CHILDREN if c[0] == walk} == set(S.WALK_DRAWS)
    assert len(T.CHILDREN) == len(set(T.CHILDREN))


def test_the_partitioned_engine_forks(monkeypatch):
    """64 chains on the launch-based engine: two partitions, each pipelined (the planner on a device of 256 CUs)"""
    import ctypes as C
    from helpers import abi_cases as A
    from helpers import edges as E
    from literate_amd import _hip
    monkeypatch.setenv("LR_DEVICE_CUS", "256")
    kw, chains, want = S.ENGINES["partitioned"]
    assert want["n_parts"] == 2 and want["pipelined"] == 1
    cfg = E.make_config(0, 0, True, A.N_BINS, chains, A.N_LINEAGES, E.ENGINES[kw["engine"]])
    lay = _hip.McmcLayout()
    assert _hip.load().lr_mcmc_query_layout(C.byref(cfg), C.byref(lay)) == 0
    for k, v in want.items():
        assert getattr(lay, k) == v, (k, getattr(lay, k))


def test_the_decoy_lineages_are_valid():
    from helpers import abi_cases as A
    ts, te = A._engine_data("unit")
    o1 = np.argsort(te, kind="stable")
    o2 = np.argsort(np.floor(ts[o1]), kind="stable")
    ts, te = ts[o1[o2]], te[o1[o2]]
    ts2, te2 = S._decoy_lineages(ts, te)
    assert ts2.shape == ts.shape and ts2.min() == ts.min() and te2.max() == te.max() and np.all(te2 > ts2)
    assert np.all(te2 - (np.ceil(te2) - 1.0) == te[0] - (np.ceil(te[0]) - 1.0)) and np.all(ts2 - np.floor(ts2) == ts[0] - np.floor(ts[0]))
    key = np.floor(ts2) * 1e6 + te2
    assert np.all(np.diff(key) >= 0), "sorted by birth bin, then death"
    assert np.count_nonzero(np.sort(te2) != np.sort(te)) > len(te) // 4


# ---- ordered() against fakes on the deferred runtime ----------------------------------------------
@pytest.mark.parametrize("fault,kind", list(S.FAULTS.items()), ids=[str(f).replace(" ", "_") for f in S.FAULTS])
def test_ordered_on_a_fake_that(fault, kind):
    rt = S.DeferredRuntime(S.fake_library())
    lib, names = rt.entry_points()
    if kind is None:
        want, table = S.run_fake(rt, fault)
        assert np.array_equal(np.frombuffer(want["0"]), 3.0 * np.arange(4096))
        assert table["fake_entry"]["calls"] == 1
    else:
        with pytest.raises(S.StreamViolation) as e:
            S.run_fake(rt, fault)
        assert e.value.kind == kind, e.value
    assert lib.fake_entry.__name__ == "fake_entry" and lib.fake_entry.__closure__ is not None          # the hook is taken off again
    assert set(S.FAULTS.values()) == {None, "order", "join", "blocked", "inconclusive", "blind"}


def test_the_deferred_streams_hold_back_what_stands_behind_a_delay():
    rt = S.DeferredRuntime(S.fake_library())
    side, other = rt.side_stream(), rt.pool_stream()
    x, y = np.zeros(3), np.ones(3)
    with rt.stream(side):
        rt.copy(x, y)                                   # nothing holds the stream back: done at once
        assert x.tolist() == [1, 1, 1] and side.query()
        rt.sleep(20.0)
        rt.fill(x, 5.0)
        assert x.tolist() == [1, 1, 1] and not side.query()
        ev = rt.record(side)
    rt.wait(other, ev)
    with rt.stream(other):
        z = rt.clone(x)
    assert not other.query()                            # waits for an event that has not happened
    with rt.stream(rt.null_stream()):
        rt.fill(y, 7.0)                                 # the null stream waits for nobody
    assert y.tolist() == [7, 7, 7] and x.tolist() == [1, 1, 1]
    other.synchronize()                                 # reaches the event: the side stream runs up to it
    assert z.tolist() == [5, 5, 5] and side.query() and other.query()


def test_a_delay_above_the_cap_names_the_call():
    import time
    rt = S.DeferredRuntime(S.fake_library())
    lib, _ = rt.entry_points()
    src = np.zeros(4)

    def slow_entry(a, dst, stream):
        time.sleep((S.MAX_DELAY_MS / S.DELAY_FACTOR + 5.0) / 1e3)
        with rt.stream(stream):
            rt.kernel(dst, a)
        return 0
    lib.fake_entry = slow_entry

    def call():
        dst = rt.alloc_output(4)
        lib.fake_entry(src, dst, rt.current_stream_arg())
        return dst
    with pytest.raises(S.StreamViolation) as e:
        S.ordered(rt, call, [np.ones(4)], [np.full(4, 2.0)], [src], "slow fake")
    assert e.value.kind == "inconclusive" and "fake_entry" in str(e.value)
