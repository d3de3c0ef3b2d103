"""The inputs of tests/test_hip_many_shifts.py, checked with the oracle alone (no GPU): that the part-B initial states and
seeds take the oracle-checked chains through the moves the device tests claim to cover - accepted adds and removes at
K >= 16, edits below lane 16 whose tail crosses a DPP row boundary, the refused add at the cap, chains falling back
under 16 rates - and that the part-A generators keep the invariants the delete-by-value reference needs.  Both modules
import tests/helpers/many_shifts.py, so they see identical inputs."""
import decimal
import os
import re

import numpy as np
import pytest

from helpers import many_shifts as MS


@pytest.mark.parametrize("name,general,model", MS.oracle_configs(),
                         ids=["%s-%s-m%d" % (n, "gen" if g else "unit", m) for n, g, m in MS.oracle_configs()])
def test_engine_inputs_reach_the_many_shift_moves(name, general, model):
    """Summed over the oracle-checked chains of every part-B configuration, run_mcmc shows: >= 5 accepted adds from
    K >= 16, >= 20 accepted removes from K >= 17, an add refused at K = 32, a chain whose KL or KM passes from >= 17 to
    <= 15, an accepted add and an accepted remove that edit lane <= 15 while K >= 17, and finite posterior, likelihood
    and prior columns throughout."""
    MS.check_initial_states(name)
    cov = MS.coverage(name, general, model)
    print(cov)
    assert cov["adds_from_16"] >= 5, cov
    assert cov["removes_from_17"] >= 20, cov
    assert cov["refused_at_cap"] >= 1 and cov["refused_chains"], cov
    assert cov["chains_crossing_down"] >= 1, cov
    assert cov["adds_low_lane"] >= 1 and cov["removes_low_lane"] >= 1, cov
    assert cov["finite"], cov
    assert cov["k_max"] == 32 and cov["k_min"] <= 15, cov
    assert len(MS.ORACLE_CHAINS) >= 4 and max(MS.ORACLE_CHAINS) == MS.C - 1


def test_engine_cases_cover_every_family_and_class():
    """The case list holds every forced family and the planner's own choice, on unit and general times, on three table
    classes (H = 72, 264, 520), model 3 on one family per table mode and model 2 on the four-chain kernel."""
    from helpers import edges as E
    cases = MS.engine_cases()
    assert [E.table_class(0, MS.window(n)[2]) for n in ("h72", "h264", "h520")] == [72, 264, 520]
    assert MS.window("h264")[2] == 193
    for name in MS.DATASETS:
        for general in (False, True):
            got = {e for n, g, m, e in cases if (n, g, m) == (name, general, 0)}
            want = {e for e in MS.RJ_ENGINES if E.engine_runs(e, 0, 0, not general, MS.window(name)[2])}
            assert got == want and {"launch", "auto", "packed", "persistent4"} <= got
    assert {e for n, g, m, e in cases if m == 0} == set(MS.RJ_ENGINES)
    assert len({(g, e) for n, g, m, e in cases if m == 3}) == 3
    assert any(m == 2 and e == "persistent4" for n, g, m, e in cases)
    assert MS.C == 37 and MS.N_IT == 400


@pytest.mark.parametrize("kmax", MS.SCORER_KMAX)
def test_scorer_records_are_exhaustive_and_distinct(kmax):
    """Every (K, interval) of the add move, every (K, removed shift) of the remove move and every K x mask of the
    multiplier move, each on pairwise distinct rates and strictly increasing times; the add's offset lies inside its
    interval and its Beta variate inside (0, 1), some of them near 0.02 and 0.98."""
    adds, rems, mults = MS.add_records(kmax), MS.remove_records(kmax), MS.mult_records(kmax)
    assert sorted((r["K"], r["ind"]) for r in adds) == [(K, i) for K in range(1, kmax) for i in range(K)]
    assert sorted((r["K"], r["idx"]) for r in rems) == [(K, i) for K in range(2, kmax + 1) for i in range(1, K)]
    assert sorted((r["K"], r["mask"]) for r in mults) == sorted((K, m) for K in range(1, kmax + 1) for m in MS.MULT_MASKS)
    for recs in (adds, rems, mults):
        MS.check_state_invariants(recs)
    for r in adds:
        assert 0.0 < r["delta"] < r["times"][r["ind"] + 1] - r["times"][r["ind"]] and 0.0 < r["u"] < 1.0
        t_prime = r["times"][r["ind"]] + r["delta"]
        assert r["times"][r["ind"]] < t_prime < r["times"][r["ind"] + 1]
    if len(adds) >= 7:
        u = np.array([r["u"] for r in adds])
        assert np.any(u < 0.03) and np.any(u > 0.97)
    rates, times, K, move, index, draws = MS.pack_scorer(adds, kmax, 1)
    assert np.all(K + 1 <= kmax) and rates.shape == (len(adds), kmax) and times.shape == (len(adds), kmax + 1)


def test_expand_cases_fill_the_window():
    """The oracle's rate index has exactly n_bins entries for every chain of every lr_expand_rates case (asserted inside
    expand_reference), every K in 1..63 occurs, shifts share bins (zero-width segments, two and three to a bin) and, in
    round mode, lie on integers and on x.5 next to even and to odd integers."""
    for n_bins in MS.EXPAND_BINS:
        for mode in (0, 1):
            for C in (1, 300):
                case = MS.expand_case(n_bins, mode, C)
                ref = MS.expand_reference(case)
                assert ref.shape == (C, n_bins)
                assert set(case["K"]) == (set(range(1, 64)) if C == 300 else {63})
                if C != 300:
                    continue
                edge = np.rint if mode else np.floor
                same = [np.sum(np.diff(edge(case["times"][c, :k + 1])) == 0) for c, k in enumerate(case["K"])]
                assert max(same) >= 3
                inner = np.concatenate([case["times"][c, 1:k] for c, k in enumerate(case["K"])])
                frac = inner - np.floor(inner)
                assert np.any(frac == 0.0)
                if mode and n_bins > 2:
                    assert np.any((frac == 0.5) & (np.floor(inner) % 2 == 0)) and np.any((frac == 0.5) & (np.floor(inner) % 2 == 1))


def test_log_factorial_table_is_the_reference_sum():
    """lr_log_factorial (csrc/lr_chain.h) holds log k! for k = 0 .. LR_KMAX + 1 as the reference sums it,
    np.sum(np.log(np.arange(1, k + 1))): every entry bit for bit, with the logarithms correctly rounded (taken from 60-digit
    decimal arithmetic, so the check does not depend on the host's libm).  The sampler comparisons hold the prior to 1e-9;
    a table entry one unit in the last place off (7e-15 at entry 20) passes them and fails here."""
    from literate_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "literate_amd", "csrc", "lr_chain.h")) as f:
        m = re.search(r"static const double T\[LR_KMAX \+ 2\] = \{([^}]*)\}", f.read())
    table = [float(x) for x in m.group(1).split(",")]
    assert len(table) == _hip.LR_KMAX + 2
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        logs = np.array([float(decimal.Decimal(j).ln()) for j in range(1, len(table))])
    for k, entry in enumerate(table):
        assert entry == float(np.sum(logs[:k])), (k, entry, float(np.sum(logs[:k])))
