"""The chain-count classes of the engine on the host (lr_mcmc_query_layout needs no device; LR_DEVICE_CUS = 256): the
boundaries at which a chain count changes the table grouping, the kernel family, the block shape or the launch
schedule, pinned; every class of the walk covered by a case of tests/test_hip_chain_edges.py; and the checks of those
cases shown to notice what they are for, on fabricated engine output (no kernel is run wrong on purpose)."""
import copy

import numpy as np
import pytest

from helpers import chain_edges as CE
from helpers import edges as E


@pytest.fixture(scope="module")
def all_cases():
    return [CE.resolved(c, CE.HOST_CUS) for c in CE.cases()]


def _walk(name, engine, **kw):
    with CE.environment(kw):
        return CE.walk(name, engine, kw)


def _steps(sigs, field):
    return CE.boundaries(sigs, lambda s: getattr(s, field) if isinstance(field, str) else field(s))


def _extra(key):
    return lambda s: dict(s.extra).get(key)


def test_table_grouping_steps_at_1_2_3_5_9():
    """cb = 1, 2, 4, 8, 16 starts at 1, 2, 3, 5, 9 chains at unit resolution under every engine that keeps unit tables -
    the persistent kernels lay their tables out per group of cb chains too."""
    for name, engine in [("A", "launch"), ("E", "launch"), ("A", "persistent2"), ("A", "spec"), ("G", "spec")]:
        sigs = _walk(name, engine)
        assert sigs[1].cb in (1, 4), (name, engine, sigs[1])          # (a lone chain: below)
        steps = [b for b in _steps(sigs, "cb") if b[0] <= 72]
        assert steps[-3:] == [(3, 4), (5, 8), (9, 16)] and sigs[2].cb == 2, (name, engine, steps)
    for name in "AE":
        assert [b for b in _steps(_walk(name, "persistent4"), "cb")] == [(2, 2), (3, 4), (5, 8), (9, 16)]
    # general times under the launches step alike up to sixteen (the wide scan) and fall back to eight, pipelined, at 17;
    # the pair-general tables of the persistent kernels and the packed scan are grouped by four whatever the count
    assert _steps(_walk("B", "launch"), "cb") == [(2, 2), (3, 4), (5, 8), (9, 16), (17, 8)]
    for engine in ("persistent4", "packed"):
        assert {s.cb for s in _walk("B", engine).values()} == {4}


def test_launch_schedule_boundaries():
    """Unit resolution: pipelined halves from 32 chains (two groups of sixteen), two partitions from 49 (four groups).
    General times: one pass of the wide scan for 9..16, cb = 8 pipelined from 17, two partitions from 25.  Model 3's
    generic scan: two unpipelined partitions from 9."""
    for name in "AE":
        sigs = _walk(name, "launch")
        assert _steps(sigs, _extra("pipelined")) == [(32, 1)] and _steps(sigs, _extra("parts")) == [(49, 2)], name
    for name in "BF":
        sigs = _walk(name, "launch")
        assert _steps(sigs, _extra("pipelined")) == [(17, 1)] and _steps(sigs, _extra("parts")) == [(25, 2)], name
        assert all(sigs[c].cb == 16 for c in range(9, 17))
    sigs = _walk("C", "launch")
    assert _steps(sigs, _extra("pipelined")) == [] and _steps(sigs, _extra("parts")) == [(9, 2)]
    assert {s.table_mode for s in sigs.values()} == {0} and max(s.cb for s in sigs.values()) == 8


def test_speculative_kernel_boundaries():
    """A team per chain up to the CUs, a team per pair up to twice as many, another family beyond; with a forced team
    of k blocks the cap is cpb * floor(CUs / k)."""
    for name in "ABCEFG":
        sigs = _walk(name, "spec")
        assert _steps(sigs, "cpb") == [(257, 2), (513, 0)], name
        assert [b for b in _steps(sigs, "family")] == [(513, 0)], name
        assert sigs[1].family == 3 and sigs[512].family == 3
    caps = {(2, 1): 128, (2, 2): 256, (4, 1): 64, (4, 2): 128, (8, 1): 32, (8, 2): 64}
    for (k, cpb), cap in caps.items():
        assert CE.team_cap(CE.HOST_CUS, k, cpb) == cap
        for name in "AB":
            kw = dict(team=k, chains_per_team=cpb)
            at, above = CE.query(name, "spec", kw, cap), CE.query(name, "spec", kw, cap + 1)
            assert (at.persistent, at.team_blocks, at.spec_chains_per_team) == (3, k, cpb), (name, k, cpb)
            assert above.persistent == 0 and above.team_blocks == 0, (name, k, cpb)


def test_forced_four_chain_kernel_below_four_chains():
    """persistent4 needs cb >= 4: two chains at unit resolution run the two-chain kernel (layout.persistent == 1); a lone
    chain that cannot fill a pair entry has the pair-general layout (cb 4) and does run the four-chain kernel; where a lone
    chain keeps unit tables (model 3, H = 520) it runs the two-chain kernel as well."""
    for name in "AEG":
        sigs = _walk(name, "persistent4")
        assert [sigs[c].family for c in (1, 2, 3, 4)] == [2, 1, 2, 2], name
        assert (sigs[1].table_mode, sigs[1].cb) == (2, 4) and (sigs[2].table_mode, sigs[2].cb) == (1, 2), name
    for name in "CD":
        sigs = _walk(name, "persistent4")
        assert [sigs[c].family for c in (1, 2, 3, 4)] == [1, 1, 2, 2] and sigs[1].table_mode == 1, name
    for name in "BF":
        assert {s.family for s in _walk(name, "persistent4").values()} == {2}, name


def test_lone_chain_tables():
    """A lone chain at unit resolution cannot fill a pair entry: general tables and the launches' scan of ts / te under
    `launch` and `persistent2`, the pair-general layout (table_mode 2, cb 4) under persistent4, spec, packed and auto."""
    for engine, want in [("launch", (0, 0, 1)), ("persistent2", (0, 0, 1)), ("persistent4", (2, 2, 4)), ("spec", (3, 2, 4)),
                         ("packed", (0, 2, 4)), ("auto", (3, 2, 4))]:
        s = CE.signature(CE.query("A", engine, {}, 1), engine, 1)
        assert (s.family, s.table_mode, s.cb) == want, (engine, s)
        assert s.packed == (engine == "packed")
        two = CE.signature(CE.query("A", engine, {}, 2), engine, 2)
        assert two.table_mode == 1, (engine, two)


def test_two_chain_kernel_threads_and_auto_families_on_long_scans():
    """Configuration G (25,000 lineages): lr_persist_kernel runs 1024 threads while there are at most 256 pairs, 512 from
    513 chains; engine="auto" leaves the speculative kernel at 513 for the four-chain kernel and takes the two-chain kernel
    from 1025 (a remainder above a whole round of 1024)."""
    assert CE.n_lineages("G") >= 20000
    sigs = _walk("G", "persistent2")
    assert _steps({c: s for c, s in sigs.items() if c > 1}, "threads") == [(513, 512)] and sigs[2].threads == 1024
    assert {s.threads for c, s in _walk("A", "persistent2").items() if c > 1} == {512}
    assert _steps(_walk("G", "auto"), "family") == [(513, 2), (1025, 1)]
    assert _steps(_walk("A", "auto"), "family") == [(513, 1)]
    assert _steps(_walk("B", "auto"), "family") == [(513, 2)]


def test_packed_scan_pairs_and_partitions():
    """PAIRS of lr_packscan_kernel: 1 up to two chains, 2 for three and four, 4 from five - always 2 from three chains at
    H = 520 (four pairs of its tables do not fit the LDS); LR_PACKED_PARTS=2 makes two partitions from two table groups."""
    for name in "ABCE":
        assert _steps(_walk(name, "packed"), _extra("PAIRS")) == [(3, 2), (5, 4)], name
    assert _steps(_walk("D", "packed"), _extra("PAIRS")) == [(3, 2)]
    assert CE.half_stride(CE.query("D", "packed", {}, 9)) == E.H_WIDE
    assert _steps(_walk("A", "packed", env={"LR_PACKED_PARTS": "2"}), _extra("parts")) == [(9, 2)]
    assert _steps(_walk("B", "packed", env={"LR_PACKED_PARTS": "2"}), _extra("parts")) == [(5, 2)]
    assert _steps(_walk("A", "packed"), _extra("parts")) == []


def test_every_case_names_its_class(all_cases):
    """What each case asserts before it runs, on the layouts of the host: a planner threshold that moves fails here."""
    assert len({CE.case_id(c) for c in all_cases}) == len(all_cases)
    for case in all_cases:
        with CE.environment(case.kwargs):
            lay = CE.query(case.config, case.engine, case.kwargs, case.chains)
        CE.check_class(case, lay, None, CE.HOST_CUS)
    # at 2 CUs + 1 the forced speculative kernel is another family's
    beyond = [c for c in all_cases if c.engine == "spec" and not c.kwargs.get("team") and c.chains == 2 * CE.HOST_CUS + 1]
    assert {c.config for c in beyond} >= set("AB") and all(CE.expected_family(c) == "launch" for c in beyond)


def _have(cases):
    have = {}
    for case in cases:
        have.setdefault((case.config, case.engine), set()).add(CE.case_signature(case))
    return have


def test_every_walked_class_has_a_case(all_cases):
    """The walk goes over EVERY configuration x engine (1..72 chains and both sides of 256, 512 and 1024; also the forced
    teams and LR_PACKED_PARTS=2 of CE.WALKED_VARIANTS), whatever cases there are.  Every signature it finds for a pair
    is the signature of at least one case - except for the eleven pairs of CE.EXCLUDED, which have no case at all: the
    list is held to the walk pair by pair with its class counts (81 classes), so a pair cannot drop out unseen.  The case
    count is held at CE.N_CASES: the counts listed for each engine (352) and one case for each class of the walk those
    leave out in their own pairs (90); the excluded pairs would take it to 523."""
    walked = CE.walked()
    assert set(walked) == {(name, engine) for name in CE.CONFIGS for engine in CE.RJ_ENGINES} and len(walked) == 42
    variants = {(n, e, 0, 0, ()) for n, e in walked} | set(CE.WALKED_VARIANTS)
    assert {CE.variant(c) for c in all_cases} <= variants
    assert set(CE.EXCLUDED) == set(walked) - {(c.config, c.engine) for c in all_cases}
    assert len(CE.EXCLUDED) == 11 and sum(CE.EXCLUDED.values()) == 81
    bad = CE.uncovered(_have(all_cases))
    n_sigs = sum(len(v) for k, v in walked.items() if k not in CE.EXCLUDED)
    assert not bad, "%d cases, %d classes, not covered: %r" % (len(all_cases), n_sigs, bad)
    assert len(all_cases) == CE.N_CASES == 442, "%d cases for %d classes" % (len(all_cases), n_sigs)
    assert n_sigs == 320
    print("%d cases cover %d classes; %d classes of %d pairs excluded" % (len(all_cases), n_sigs, 81, 11))


def test_coverage_notices_a_pair_or_a_class_that_loses_its_cases(all_cases):
    """The coverage check does not follow the cases: without the cases of one pair, or of one class, it fails."""
    assert ("D", "packed") in CE.uncovered(_have([c for c in all_cases if (c.config, c.engine) != ("D", "packed")]))
    assert ("A", "launch") in CE.uncovered(_have([c for c in all_cases if not (c.config == "A" and c.engine == "launch" and 32 <= c.chains < 49)]))
    extra = all_cases + [CE.Case("G", "packed", {}, 5)]
    assert ("G", "packed") in CE.uncovered(_have(extra))          # an excluded pair that gains a case must leave the list


# ---- the checks notice what they are for -----------------------------------------------------------------------------
N_FAKE = 6


@pytest.fixture(scope="module")
def fabricated():
    """What a correct six-chain run of configuration A would leave, made from the oracle alone: the trace rows' heads from
    oracle/mcmc_oracle.run_mcmc, each chain's accepted state a constant-rate state scored by the fp64 oracle."""
    from literate_amd import _hip
    from oracle import literate_oracle as lo
    cfg = CE.CONFIGS["A"]
    ts, te = CE.data("A")
    tr = np.full((CE.N_IT, N_FAKE, _hip.LR_TRACE_W), np.nan)
    for c in range(N_FAKE):
        rows = CE.rj_trajectory("A", c)
        for i in range(CE.N_IT):
            tr[i, c, :13] = rows[i][:13]
    end = float(cfg.n_bins) + 0.5
    snap = dict(L=[np.array([0.3 + 0.01 * c]) for c in range(N_FAKE)], M=[np.array([0.2 + 0.01 * c]) for c in range(N_FAKE)],
                tL=[np.array([end, 0.0]) for _ in range(N_FAKE)], tM=[np.array([end, 0.0]) for _ in range(N_FAKE)],
                priorA=np.linspace(-3.0, -2.0, N_FAKE), it=np.full(N_FAKE, CE.N_IT, dtype=np.int64))
    lam, mu = E.accepted_rates(snap, cfg.n_bins, N_FAKE)
    pre = lo.lineage_bins(ts, te, 0.0, cfg.n_bins)
    snap["likA"] = np.array([E.reference_loglik(ts, te, lam[c], mu[c], cfg.model, CE.rj_stats("A"), pre) for c in range(N_FAKE)])
    return tr, snap


def test_checks_pass_on_a_correct_run(fabricated):
    tr, snap = fabricated
    CE.check_rj_case(tr, snap, "A", 0, "fabricated")


def test_checks_follow_global_ids_under_an_offset(fabricated):
    tr, snap = fabricated
    CE.check_rj_case(tr[:, 2:], {k: v[2:] for k, v in snap.items()}, "A", 2, "fabricated")
    with pytest.raises(AssertionError):
        CE.check_rj_case(tr[:, 2:], {k: v[2:] for k, v in snap.items()}, "A", 3, "fabricated")


def test_a_last_chain_that_repeats_its_neighbour_fails(fabricated):
    """Chain C - 1's rows are chain C - 2's."""
    tr, snap = fabricated
    bad = tr.copy()
    bad[:, N_FAKE - 1] = bad[:, N_FAKE - 2]
    with pytest.raises(AssertionError):
        CE.check_rj_case(bad, snap, "A", 0, "fabricated")
    assert N_FAKE - 1 in CE.followed(N_FAKE) and N_FAKE - 2 in CE.followed(N_FAKE)


def test_a_log_likelihood_off_by_1e_6_relative_fails(fabricated):
    tr, snap = fabricated
    bad = copy.deepcopy(snap)
    bad["likA"][-1] *= 1.0 + 1e-6
    with pytest.raises(AssertionError):
        CE.check_rj_case(tr, bad, "A", 0, "fabricated")
    # ... on a chain that is not followed row by row as well: every chain is re-scored
    mid = [c for c in range(N_FAKE) if c not in CE.followed(N_FAKE)][0]
    bad = copy.deepcopy(snap)
    bad["likA"][mid] *= 1.0 - 1e-6
    with pytest.raises(AssertionError):
        CE.check_rj_case(tr, bad, "A", 0, "fabricated")


def test_two_chains_with_identical_state_rows_fail(fabricated):
    tr, snap = fabricated
    bad = copy.deepcopy(snap)
    for k in ("L", "M", "tL", "tM", "likA", "priorA"):
        bad[k][N_FAKE - 1] = copy.deepcopy(bad[k][N_FAKE - 2])
    with pytest.raises(AssertionError, match="same state"):
        CE.check_every_chain(bad, tr, CE.N_IT)
    with pytest.raises(AssertionError):
        CE.check_rj_case(tr, bad, "A", 0, "fabricated")


def test_an_unfinished_chain_and_a_broken_iteration_column_fail(fabricated):
    tr, snap = fabricated
    bad = copy.deepcopy(snap)
    bad["it"][3] = CE.N_IT - 1
    with pytest.raises(AssertionError):
        CE.check_every_chain(bad, tr, CE.N_IT)
    rows = tr.copy()
    rows[40, 3, 0] = 39.0
    with pytest.raises(AssertionError):
        CE.check_every_chain(snap, rows, CE.N_IT)
    bad = copy.deepcopy(snap)
    bad["likA"][2] = np.nan
    with pytest.raises(AssertionError):
        CE.check_every_chain(bad, tr, CE.N_IT)


# ---- the same for the parametric samplers' rows -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def fabricated_param():
    """Log rows, trace iteration column and end states of a correct six-chain DDRate run (configuration E), from the oracle
    loop alone."""
    from literate_amd import _hip
    rows = {c: [np.array(r, dtype=float) for r in CE.param_trajectory("E", c)] for c in range(N_FAKE)}
    tr = np.full((CE.N_IT, N_FAKE, _hip.LR_TRACE_W), np.nan)
    tr[:, :, 0] = np.arange(CE.N_IT, dtype=float)[:, None]
    last = [rows[c][-1] for c in range(N_FAKE)]
    snap = dict(L=[r[6:14].copy() for r in last], M=[np.zeros(0)] * N_FAKE, tL=[np.zeros(0)] * N_FAKE, tM=[np.zeros(0)] * N_FAKE,
                likA=np.array([r[2] for r in last]), priorA=np.array([r[5] for r in last]),
                it=np.full(N_FAKE, CE.N_IT, dtype=np.int64))
    return rows, tr, snap


def test_param_checks_pass_on_a_correct_run_and_fail_on_a_repeated_chain(fabricated_param):
    rows, tr, snap = fabricated_param
    follow = CE.followed(N_FAKE)
    CE.check_param_case({c: rows[c] for c in follow}, tr, snap, "E", 0, "fabricated")
    bad = {c: rows[c] for c in follow}
    bad[N_FAKE - 1] = rows[N_FAKE - 2]                      # chain C - 1's rows are chain C - 2's
    with pytest.raises(AssertionError):
        CE.check_param_case(bad, tr, snap, "E", 0, "fabricated")
    bad = {c: [r.copy() for r in rows[c]] for c in follow}
    bad[follow[2]][40][2] *= 1.0 + 1e-6                     # a likelihood column off by 1e-6 relative
    with pytest.raises(AssertionError):
        CE.check_param_case(bad, tr, snap, "E", 0, "fabricated")
    with pytest.raises(AssertionError):                     # a chain that is to be followed is missing
        CE.check_param_case({c: rows[c] for c in follow[:-1]}, tr, snap, "E", 0, "fabricated")
