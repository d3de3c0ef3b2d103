"""The reversible-jump moves and every engine family at many rate shifts, up to the cap.

One wave owns one chain and lane j holds rate j and shift time j (csrc/lr_chain.h): an add or a remove moves whole
vectors one lane up or down (DPP wave_shr:1 / wave_shl:1), every reduction ends in row_bcast15 / row_bcast31, and the
table builds broadcast the K - 1 edges with v_readlane.  The other modules keep all of this inside lanes 0..6 of DPP
row 0 (K <= 6).  Here:

  part A  the explicit-draw kernels (lr_rj_propose_score, lr_log_priors, lr_expand_rates, lr_binned_keiding) against the
          oracle's functions, exhaustively over K and the edited lane up to kmax = 63: what a move only relocates must
          come out bit-equal, the padding exactly 0.0;
  part B  every engine family from initial states with 16..32 rates per process, row by row against
          oracle/mcmc_oracle.run_mcmc fed the same Philox draws, with the assertions of
          test_hip_edges.py::test_rj_sampler_at_the_class_edges, the per-segment trace columns, the cap's warning word and
          one checkpoint taken while chains hold more than 16 rates.

The cases come from tests/helpers/many_shifts.py; tests/test_many_shifts_host.py proves with the oracle alone that they
reach the moves named above.  No case is skipped."""
import numpy as np
import pytest

from helpers import edges as E
from helpers import many_shifts as MS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: no ROCm device visible")
    from literate_amd import ops as _ops
    return _ops


def _np(x):
    return x.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------
# part A
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmax", MS.SCORER_KMAX)
def test_add_shift_over_every_lane(ops, kmax):
    """lr_rj_propose_score, add move: every K in 1..kmax-1 x every interval, one launch (1953 chains at kmax = 63)
    against add_shift_RJ_weighted_mean.  K' and the inserted time exact (one fp64 add); every rate and time left of the
    edit and every one the move shifts one lane up bit-equal to its input; the padding beyond K' exactly 0.0; the two new
    rates at rtol 1e-13 and the score at rel = abs = 1e-11 (the tolerances of test_proposal_scorers_golden)."""
    from oracle import literate_oracle as lo
    recs = MS.add_records(kmax)
    rates, times, K, move, index, draws = MS.pack_scorer(recs, kmax, 1)
    o_r, o_t, o_k, o_s = [_np(x) for x in ops.rj_propose_score(rates, times, K, move, index, draws)]
    worst_r = worst_s = 0.0
    for i, r in enumerate(recs):
        k, ind = r["K"], r["ind"]
        ref_r, ref_t, ref_s = lo.add_shift_RJ_weighted_mean(r["rates"], r["times"], ind, r["delta"], r["u"])
        assert o_k[i] == k + 1 == len(ref_r), (kmax, k, ind)
        assert o_t[i, ind + 1] == r["times"][ind] + r["delta"] == ref_t[ind + 1], (kmax, k, ind)
        assert np.array_equal(o_t[i, :ind + 1], r["times"][:ind + 1]), (kmax, k, ind, "times left of the edit")
        assert np.array_equal(o_t[i, ind + 2:k + 2], r["times"][ind + 1:]), (kmax, k, ind, "times shifted up")
        assert np.array_equal(o_t[i, :k + 2], ref_t), (kmax, k, ind)
        assert np.array_equal(o_r[i, :ind], r["rates"][:ind]), (kmax, k, ind, "rates left of the edit")
        assert np.array_equal(o_r[i, ind + 2:k + 1], r["rates"][ind + 1:]), (kmax, k, ind, "rates shifted up")
        assert not np.any(o_r[i, k + 1:]) and not np.any(o_t[i, k + 2:]), (kmax, k, ind, "padding")
        assert np.allclose(o_r[i, ind:ind + 2], ref_r[ind:ind + 2], rtol=1e-13, atol=0.0), (kmax, k, ind)
        worst_r = max(worst_r, np.max(np.abs(o_r[i, ind:ind + 2] / ref_r[ind:ind + 2] - 1.0)))
        worst_s = max(worst_s, abs(o_s[i] - ref_s) / max(1.0, abs(ref_s)))
        assert o_s[i] == pytest.approx(ref_s, rel=1e-11, abs=1e-11), (kmax, k, ind)
    print("add kmax %d: %d chains, worst new-rate error %.2e rel, worst score error %.2e" % (kmax, len(recs), worst_r, worst_s))


@pytest.mark.parametrize("kmax", MS.SCORER_KMAX)
def test_remove_shift_over_every_lane(ops, kmax):
    """lr_rj_propose_score, remove move: every K in 2..kmax x every removed shift 1..K-1 in one launch against
    remove_shift_RJ_weighted_mean (pairwise distinct values: the reference deletes by value).  K' exact; what lies left
    of the edit and what the move shifts one lane down bit-equal to its input; the padding 0.0; the merged rate at
    rtol 1e-13, the score at rel = abs = 1e-11."""
    from oracle import literate_oracle as lo
    recs = MS.remove_records(kmax)
    rates, times, K, move, index, draws = MS.pack_scorer(recs, kmax, 2)
    o_r, o_t, o_k, o_s = [_np(x) for x in ops.rj_propose_score(rates, times, K, move, index, draws)]
    worst_r = worst_s = 0.0
    for i, r in enumerate(recs):
        k, idx = r["K"], r["idx"]
        ref_r, ref_t, ref_s = lo.remove_shift_RJ_weighted_mean(r["rates"], r["times"], idx)
        assert o_k[i] == k - 1 == len(ref_r) and len(ref_t) == k, (kmax, k, idx)
        assert np.array_equal(o_t[i, :idx], r["times"][:idx]), (kmax, k, idx, "times left of the edit")
        assert np.array_equal(o_t[i, idx:k], r["times"][idx + 1:]), (kmax, k, idx, "times shifted down")
        assert np.array_equal(o_t[i, :k], ref_t), (kmax, k, idx)
        assert np.array_equal(o_r[i, :idx - 1], r["rates"][:idx - 1]), (kmax, k, idx, "rates left of the edit")
        assert np.array_equal(o_r[i, idx:k - 1], r["rates"][idx + 1:]), (kmax, k, idx, "rates shifted down")
        assert not np.any(o_r[i, k - 1:]) and not np.any(o_t[i, k:]), (kmax, k, idx, "padding")
        assert np.allclose(o_r[i, idx - 1], ref_r[idx - 1], rtol=1e-13, atol=0.0), (kmax, k, idx)
        worst_r = max(worst_r, abs(o_r[i, idx - 1] / ref_r[idx - 1] - 1.0))
        worst_s = max(worst_s, abs(o_s[i] - ref_s) / max(1.0, abs(ref_s)))
        assert o_s[i] == pytest.approx(ref_s, rel=1e-11, abs=1e-11), (kmax, k, idx)
    print("remove kmax %d: %d chains, worst merged-rate error %.2e rel, worst score error %.2e" % (kmax, len(recs), worst_r, worst_s))


@pytest.mark.parametrize("kmax", MS.SCORER_KMAX)
def test_multiplier_over_every_lane(ops, kmax):
    """lr_rj_propose_score, multiplier move: every K in 1..kmax with the update mask all on, all off, alternating and
    only lane K - 1, against update_multiplier_freq: rates at rtol 1e-14, the Hastings term (a sum over up to 63 lanes
    through lr_wave_sum) at rel 1e-12 / abs 1e-14, lanes with the mask off bit-equal to their input, K and the times
    unchanged, the padding 0.0."""
    from oracle import literate_oracle as lo
    recs = MS.mult_records(kmax)
    rates, times, K, move, index, draws = MS.pack_scorer(recs, kmax, 0)
    o_r, o_t, o_k, o_s = [_np(x) for x in ops.rj_propose_score(rates, times, K, move, index, draws)]
    worst = 0.0
    for i, r in enumerate(recs):
        k = r["K"]
        ref_r, ref_h = lo.update_multiplier_freq(r["rates"], r["ff"], r["u"])
        off = r["ff"] == 0
        assert o_k[i] == k and np.array_equal(o_t[i, :k + 1], r["times"]), (kmax, k, r["mask"])
        assert np.array_equal(o_r[i, :k][off], r["rates"][off]), (kmax, k, r["mask"], "lanes the mask leaves alone")
        assert not np.any(o_r[i, k:]) and not np.any(o_t[i, k + 1:]), (kmax, k, r["mask"], "padding")
        assert np.allclose(o_r[i, :k], ref_r, rtol=1e-14, atol=0.0), (kmax, k, r["mask"])
        worst = max(worst, abs(o_s[i] - ref_h))
        assert o_s[i] == pytest.approx(ref_h, rel=1e-12, abs=1e-14), (kmax, k, r["mask"], o_s[i] - ref_h)
        if r["mask"] == "off":
            assert o_s[i] == 0.0
    print("multiplier kmax %d: %d chains, worst Hastings error %.2e abs" % (kmax, len(recs), worst))


@pytest.mark.parametrize("shape", MS.PRIOR_SHAPES)
def test_log_priors_over_every_lane(ops, shape):
    """lr_log_priors: every K in 1..63 at kmax = 63 and K = kmax at kmax 1, 16, 17, 33, rates log-uniform over
    1e-3..1e2, shape 2 and a non-integer one, against prior_gamma at rtol = atol = 1e-12; the Poisson term (the
    difference of the runs with and without it, as test_priors_golden takes it) against Poisson_prior at
    rtol = atol = 1e-11, at several Poisson rates."""
    from oracle import literate_oracle as lo
    worst_g = worst_p = 0.0
    for kmax, rec in MS.prior_records().items():
        rates, K, b = rec["rates"], rec["K"], rec["b"]
        ref = np.array([lo.prior_gamma(rates[i, :K[i]], shape, b[i]) for i in range(len(K))])
        base = _np(ops.log_priors(rates, K, shape, b))
        worst_g = max(worst_g, np.max(np.abs(base - ref) / np.maximum(1.0, np.abs(ref))))
        assert np.allclose(base, ref, rtol=1e-12, atol=1e-12), (kmax, shape, np.max(np.abs(base - ref)))
        for poi in MS.PRIOR_POISSON[1:]:
            got = _np(ops.log_priors(rates, K, shape, b, np.full(len(K), poi))) - base
            ref_p = np.array([lo.Poisson_prior(int(k), poi) for k in K])
            worst_p = max(worst_p, np.max(np.abs(got - ref_p) / np.maximum(1.0, np.abs(ref_p))))
            assert np.allclose(got, ref_p, rtol=1e-11, atol=1e-11), (kmax, shape, poi, np.max(np.abs(got - ref_p)))
    print("priors shape %g: worst gamma error %.2e, worst Poisson error %.2e (relative to max(1, |ref|))" % (shape, worst_g, worst_p))


@pytest.mark.parametrize("n_chains", (1, 300))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("n_bins", MS.EXPAND_BINS)
def test_expand_rates_over_every_lane(ops, n_bins, mode, n_chains):
    """lr_expand_rates at K in 1..63 (kmax = 63), floor and round mode, bin counts on both sides of its 128-thread block,
    one chain and 300: exactly rates[get_rate_index(...)], with two and three shifts in one bin (zero-width segments)
    and, in round mode, shifts and window ends on integers and on x.5 (half to even, both ways)."""
    case = MS.expand_case(n_bins, mode, n_chains)
    ref = MS.expand_reference(case)
    got = _np(ops.expand_rates(case["rates"], case["times"], case["K"], n_bins, mode))
    assert got.shape == ref.shape == (n_chains, n_bins)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (n_bins, mode, bad[:5], [int(case["K"][c]) for c, _ in bad[:5]])


@pytest.mark.parametrize("n_bins", MS.KEIDING_BINS)
def test_binned_keiding_against_the_plain_sum(ops, n_bins):
    """lr_binned_keiding on both sides of the 64-lane stride and at 1000 bins against numpy's sum, rel 1e-12."""
    c = MS.keiding_case(n_bins)
    ob, od = [_np(x) for x in ops.binned_keiding(c["birth"], c["death"], c["n_spec"], c["n_exti"], c["DT"])]
    ref_b = np.sum(np.log(c["birth"]) * c["n_spec"] - c["birth"] * c["DT"], axis=1)
    ref_d = np.sum(np.log(c["death"]) * c["n_exti"] - c["death"] * c["DT"], axis=1)
    assert np.allclose(ob, ref_b, rtol=1e-12, atol=0.0), (n_bins, ob - ref_b)
    assert np.allclose(od, ref_d, rtol=1e-12, atol=0.0), (n_bins, od - ref_d)


def test_scorers_refuse_what_does_not_fit(ops):
    """The sizes the ABI refuses (kmax = 64 and kmax = 1 for lr_rj_propose_score, kmax = 64 for lr_log_priors, 65536 chains
    for lr_expand_rates), and the K a host array may not carry: K > kmax, K < 1, an add at K = kmax - all ValueError,
    raised before any launch."""
    def scorer_args(kmax, C=2, K=1, move=1):
        return (np.ones((C, kmax)), np.tile(np.arange(kmax + 1.0), (C, 1)), np.full(C, K, np.int32), np.full(C, move, np.int32),
                np.full(C, 1 if move == 2 else 0, np.int32), np.full((C, 2 * kmax), 0.5))

    for kmax in (64, 1):
        with pytest.raises(ValueError, match="LR_ERR_SIZE"):
            ops.rj_propose_score(*scorer_args(kmax, move=0))
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        ops.log_priors(np.ones((2, 64)), np.full(2, 3, np.int32), 2.0, np.ones(2))
    with pytest.raises(ValueError, match="LR_ERR_SIZE"):
        ops.expand_rates(np.ones((65536, 1)), np.tile([0.0, 4.0], (65536, 1)), np.ones(65536, np.int32), 4)
    ops.rj_propose_score(*scorer_args(8, K=7, move=1))                   # an add into the last free lane
    ops.rj_propose_score(*scorer_args(8, K=8, move=2))
    for kw in (dict(K=8, move=1), dict(K=9, move=2), dict(K=9, move=0), dict(K=0, move=0)):
        with pytest.raises(ValueError, match="rj_propose_score"):
            ops.rj_propose_score(*scorer_args(8, **kw))
    for k in (0, 9):
        with pytest.raises(ValueError, match="log_priors"):
            ops.log_priors(np.ones((2, 8)), np.array([1, k], np.int32), 2.0, np.ones(2))
        with pytest.raises(ValueError, match="expand_rates"):
            ops.expand_rates(np.ones((2, 8)), np.tile(np.arange(9.0), (2, 1)), np.array([k, 2], np.int32), 8)


# ------------------------------------------------------------------------------------------------------------------
# part B
# ------------------------------------------------------------------------------------------------------------------
FORCED = {"launch": "launch", "packed": "packed", "persistent2": "persist2", "persistent4": "persist4", "spec": "spec"}


def _engine(name, general, model, engine, n_slots=MS.N_IT):
    from literate_amd.engine import ChainEngine
    ts, te = MS.lineages(name, general)
    eng = ChainEngine(ts, te, MS.C, model=model, seed=MS.SEED, s_freq=1, n_trace_slots=n_slots, engine=engine,
                      poisson_HP=MS.POISSON_HP)
    return ts, te, eng


def _reference_loglik(ts, te, t0, lam, mu, model, stats, pre):
    from oracle import literate_oracle as lo
    if model == 3:
        return lo.calc_likelihood(3, lam, mu, stats)
    return lo.per_lineage_loglik(ts, te, t0, lam, mu, model, stats["br"], pre=pre)


@pytest.mark.parametrize("name,general,model,engine", MS.engine_cases(),
                         ids=["%s-%s-m%d-%s" % (n, "gen" if g else "unit", m, e) for n, g, m, e in MS.engine_cases()])
def test_engines_from_many_shift_states(name, general, model, engine):
    """Every engine family from initial states with (KL, KM) = (31, 32), (24, 28) and (17, 16), poisson_HP = 200, 37
    chains, 400 iterations in two calls, s_freq = 1, on three table classes, unit and general times (jitter on the 2^-32
    grid: decisions must equal the oracle's).  Six chains row by row against run_mcmc(init=..., k_max=32): iteration and
    both K columns exact, the 13 head columns at rtol = atol = 1e-9, the per-segment rates and shift times of the trace
    row against the oracle's sp / ex rows at the same tolerance; every chain's final accepted state re-scored in fp64 by
    the oracle and by lr_bd_loglik_batch at rtol 1e-9; the warning word carries LR_WARN_KCAP iff an oracle-checked chain
    had an add refused at the cap (the word is per engine; test_many_shifts_host.py shows that one always has);
    kernel_name() names the forced family."""
    from literate_amd import _hip, ops
    from literate_amd.engine import split_trace_row
    from oracle import literate_oracle as lo
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: no ROCm device visible")
    refs = MS.oracle_runs(name, general, model)
    stats = MS.stats_of(name, general, model)
    n_bins = MS.window(name)[2]
    ts, te, eng = _engine(name, general, model, engine)
    try:
        assert eng.n_bins == n_bins and eng.unit_resolution == (not general)
        cell = E.kernel_cell(eng.kernel_name(), model, 0)
        assert cell == E.layout_cell(model, 0, n_bins, eng.layout), (eng.kernel_name(), cell)
        if engine in FORCED:
            assert cell[0] == FORCED[engine], (engine, cell)
        if model != 3 and cell[0] != "launch":
            assert cell[1] == MS.DATASETS[name][4], cell
        eng.init(*MS.initial_states(name))
        eng.steps(MS.N_IT // 2)
        eng.steps(MS.N_IT - MS.N_IT // 2)
        tr = eng.trace_rows()
        for c in MS.ORACLE_CHAINS:
            ref = refs[c][0]
            for i in range(MS.N_IT):
                head, sp_row, ex_row = split_trace_row(tr[i, c])
                r = ref["mcmc"][i]
                assert head[0] == r[0] and head[6] == r[6] and head[7] == r[7], (cell, c, i, head[:8], r[:8])
                assert np.allclose(head[:13], r[:13], rtol=1e-9, atol=1e-9), (cell, c, i, head, r)
                assert len(sp_row) == len(ref["sp"][i]) and len(ex_row) == len(ref["ex"][i])
                assert np.allclose(sp_row, ref["sp"][i], rtol=1e-9, atol=1e-9), (cell, c, i, sp_row, ref["sp"][i])
                assert np.allclose(ex_row, ref["ex"][i], rtol=1e-9, atol=1e-9), (cell, c, i, ex_row, ref["ex"][i])
        snap = eng.snapshot()
        assert np.all(snap["it"] == MS.N_IT) and np.all(np.isfinite(snap["likA"]))
        for c in MS.ORACLE_CHAINS:
            fin = refs[c][0]["final"]
            assert np.allclose(snap["L"][c], fin[0], rtol=1e-9) and np.allclose(snap["tM"][c], fin[3], rtol=1e-9)
        lam, mu = E.accepted_rates(snap, n_bins, MS.C)
        pre = lo.lineage_bins(ts, te, eng.t0, n_bins)
        ref = np.array([_reference_loglik(ts, te, eng.t0, lam[c], mu[c], model, stats, pre) for c in range(MS.C)])
        assert np.allclose(snap["likA"], ref, rtol=1e-9, atol=0.0), (cell, snap["likA"] - ref)
        lik = ops.bd_loglik_batch(eng.ts, eng.te, eng.t0, lam, mu, model, br_length=stats["br"],
                                  end_time=eng.end_time).cpu().numpy()
        assert np.allclose(lik, snap["likA"], rtol=1e-9, atol=0.0), (cell, lik - snap["likA"])
        refused = bool(MS.coverage(name, general, model)["refused_chains"])
        assert bool(eng.warnings() & _hip.LR_WARN_KCAP) == refused, (cell, eng.warnings(), refused)
    finally:
        eng.close()


@pytest.mark.parametrize("engine", ("persistent4", "launch"))
def test_checkpoint_while_chains_hold_more_than_sixteen_rates(engine, tmp_path):
    """save() after 150 iterations from the many-shift states, while chains hold more than 16 rates per process, load()
    into a fresh engine, continue: every trace row and the whole chain state bit-identical to the uninterrupted run, and
    the warning word too - the resumed run still reports the adds refused at the cap before the checkpoint."""
    import torch
    from literate_amd import _hip
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: no ROCm device visible")
    name, cut = "h264", 150
    init = MS.initial_states(name)
    _, _, a = _engine(name, False, 0, engine)
    _, _, b = _engine(name, False, 0, engine)
    _, _, c = _engine(name, False, 0, engine)
    try:
        a.init(*init); a.steps(cut); a.steps(MS.N_IT - cut)
        b.init(*init); b.steps(cut)
        snap = b.snapshot()
        assert np.sum((snap["K_l"] > 16) | (snap["K_m"] > 16)) >= 10, (snap["K_l"], snap["K_m"])
        b.save(tmp_path / "many_shifts.npz")
        c.load(tmp_path / "many_shifts.npz")
        assert c.warnings() == b.warnings()              # a resumed run keeps the cap's warning of the rows it resumes
        c.steps(MS.N_IT - cut)
        ta, tc = a.trace_rows(), c.trace_rows()
        assert ta.shape == tc.shape == (MS.N_IT, MS.C, ta.shape[2])
        assert np.array_equal(ta, tc, equal_nan=True)
        assert np.array_equal(a.state_f64.cpu().numpy(), c.state_f64.cpu().numpy(), equal_nan=True)
        assert np.array_equal(a.state_i32.cpu().numpy(), c.state_i32.cpu().numpy())
        assert a.warnings() == c.warnings() and a.warnings() & _hip.LR_WARN_KCAP
    finally:
        a.close(); b.close(); c.close()
