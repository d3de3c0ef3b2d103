"""The four-chain kernel's resident scan groups (lr_persist4_kernel's NR: a scanning lane keeps the decoded groups of its
first trips in registers for a whole launch and scores them as straight-line code, lr_resident_groups in csrc/lr_scan.h)
against the same build with LR_P4_RESIDENT=0, where every trip goes through the scan loop: bit equality of everything a
run leaves - the two state blocks, the snapshot() taken from them and every sampled trace row - after 400 iterations in two
launches of 150 + 250 (a launch cut with carried sums inside).  The resident form scores the same groups per lane in the
same order through the same operations, so there is no tolerance.

What can go wrong sits at the seams between the resident trips and the loop behind them, so the sizes are picked by the
number of packed groups n8 they give (ChainEngine.p4_resident() reads it back, and every case asserts the trip class it
is meant to hit: a change of the packing or of NR must not empty a case silently).  nh = 128 x the helper lanes' trips,
the twelve scanner waves stride 768 groups per trip over the n8 - nh groups behind the helpers' share:
  - 3,000 lineages on 24 bins (H = 40; model 3: 72): 225 groups (354), less than one trip and no helper share; most
    waves have no group
  - 60,000 lineages on 128 bins (H = 136): 6 trips per scanner lane (fewer than NR), 2 per helper lane; a ragged last trip
  - NR - 1 full trips and a ragged NR-th: the last resident trip runs on some waves only, lanes past the end inside it
  - at most one wave (64 groups) more than nh + 768 NR: the loop behind the resident trips runs on one wave only
  - 64 to 128 groups more than nh + 768 NR: the first two scanner waves enter the loop, for one trip
  - 100,000 lineages on 128 bins, the benchmark's size: 9 trips, one behind the resident ones on most waves.
p4_resident()[0] is what scanner waves 6..15 keep; waves 4 and 5, which also make the draws ahead, keep 4 trips, so their
seam lies at trip 4 in every case of four trips or more and behind their only trip (or none) in the shortest."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_IT, CUT = 400, 150
NR = 8              # resident trips per scanner lane the library ships (LR_P4_NR, csrc/lr_mcmc.hip)
RES_HELP = 5        # ... per helper lane (LR_P4_RES_HELP)
STRIDE = 768        # groups per trip of the twelve scanner waves
# lineages that give the group counts named above under synth.make_lineages(n, 128, n_shifts=3, seed=17)
N_RAGGED, N_ONE_WAVE, N_TWO_WAVES = 85_595, 94_378, 94_892

_DATA = {}


def _data(n, n_bins):
    if (n, n_bins) not in _DATA:
        from literate_amd import synth
        ts, te, _ = synth.make_lineages(n, n_bins=n_bins, n_shifts=3, seed=17)
        _DATA[(n, n_bins)] = (ts, te)
    return _DATA[(n, n_bins)]


def _engine(ts, te, chains, kw):
    from literate_amd.engine import ChainEngine
    return ChainEngine(ts, te, chains, seed=23, s_freq=7, n_trace_slots=N_IT // 7 + 2, engine="persistent4", **kw)


def _leavings(eng):
    import torch
    torch.cuda.synchronize()
    assert eng.layout.persistent == 2
    return dict(res=eng.p4_resident(), name=eng.kernel_name(), word=eng.p4_config(), H=eng.layout.table_stride, snap=eng.snapshot(),
                S=eng.state_f64.cpu().numpy().copy(), I=eng.state_i32.cpu().numpy().copy(), rows=eng.trace_rows().copy())


def _run(ts, te, chains, kw):
    """400 iterations in two launches -> what the run leaves"""
    eng = _engine(ts, te, chains, kw)
    eng.init()
    eng.steps(CUT)
    eng.steps(N_IT - CUT)
    out = _leavings(eng)
    eng.close()
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    # (trace rows pad with NaN: equal as float64 values where they are numbers, and the same bits everywhere)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(a.view(np.int64), b.view(np.int64))


def _assert_same_run(got, ref, chains):
    assert got["name"] == ref["name"] and got["word"] == ref["word"] and got["H"] == ref["H"]
    assert len(got["rows"]) == (N_IT + 6) // 7 and got["rows"].shape[1] == chains
    assert _same_bits(got["rows"], ref["rows"])
    assert _same_bits(got["S"], ref["S"]) and np.array_equal(got["I"], ref["I"])
    sg, sr = got["snap"], ref["snap"]
    assert set(sg) == set(sr)
    for k in sg:
        if isinstance(sg[k], list):
            assert len(sg[k]) == len(sr[k]) == chains and all(_same_bits(x, y) for x, y in zip(sg[k], sr[k])), k
        elif sg[k].dtype.kind == "f":
            assert _same_bits(sg[k], sr[k]), k
        else:
            assert np.array_equal(sg[k], sr[k]), k
    assert np.all(sg["it"] == N_IT) and sg["accepted"].min() > 0 and np.all(np.isfinite(sg["likA"]))


def _trips(res):
    """(scanner trips of the first wave, groups of the last of them, groups behind nh + 768 NR) of a p4_resident() tuple"""
    n8, nh = res[2], 128 * res[3]
    k_tot = -(-(n8 - nh) // STRIDE)
    return k_tot, (n8 - nh) - (k_tot - 1) * STRIDE, (n8 - nh) - NR * STRIDE


def _compare(monkeypatch, n, n_bins, chains, kw, H, shape):
    ts, te = _data(n, n_bins)
    monkeypatch.delenv("LR_P4_RESIDENT", raising=False)
    got = _run(ts, te, chains, kw)
    monkeypatch.setenv("LR_P4_RESIDENT", "0")
    ref = _run(ts, te, chains, kw)
    # which path ran: the helper-wave form both times, resident trips in the first run only, on the same groups and shares
    assert got["name"] == "lr_persist4_kernel<%d, false, false, true>" % H, got["name"]
    assert ref["res"][:2] == (0, 0) and ref["res"][2:] == got["res"][2:], (got["res"], ref["res"])
    k_tot, last, behind = _trips(got["res"])
    assert got["res"][0] == min(NR, k_tot) and got["res"][1] == min(RES_HELP, got["res"][3]), got["res"]
    if shape == "short":          # less than one trip, no helper share, at least half of the twelve waves without a group
        assert got["res"][3] == 0 and k_tot == 1 and last <= 6 * 64, got["res"]      # (225 groups; model 3: 354)
    elif shape == "six":          # 6 trips (fewer than NR unless NR <= 6), 2 helper trips, a ragged last trip
        assert got["res"][3] == 2 and k_tot == 6 and last % 64 != 0 and last < STRIDE - 64, got["res"]
    elif shape == "ragged":       # the NR-th trip is the last: some waves run it, some do not, one has lanes past the end
        assert k_tot == NR and 64 < last < STRIDE - 64 and last % 64 != 0, got["res"]
    elif shape == "one_wave":     # only the first scanner wave has a trip behind the resident ones
        assert 0 < behind <= 64, got["res"]
    elif shape == "two_waves":    # the first two scanner waves do, for one trip
        assert 64 < behind <= 128, got["res"]
    else:                         # the benchmark's size: trips behind the resident ones on most waves
        assert shape == "cfg4" and got["res"][0] == NR and behind > STRIDE // 2 and got["res"][1] == RES_HELP, got["res"]
    _assert_same_run(got, ref, chains)


@pytest.mark.parametrize("chains", [4, 6, 9])
def test_short_scan_full_block_ragged_pair_and_lone_chain(monkeypatch, chains):
    _compare(monkeypatch, 3000, 24, chains, dict(model=0), 40, "short")


@pytest.mark.parametrize("n,shape", [(60_000, "six"), (N_RAGGED, "ragged"), (N_ONE_WAVE, "one_wave"), (N_TWO_WAVES, "two_waves"),
                                     (100_000, "cfg4")])
def test_seams_between_resident_trips_and_the_loop(monkeypatch, n, shape):
    _compare(monkeypatch, n, 128, 9, dict(model=0), 136, shape)


@pytest.mark.parametrize("n,n_bins,H,shape", [(3000, 24, 40, "short"), (N_ONE_WAVE, 128, 136, "one_wave")])
def test_model_2(monkeypatch, n, n_bins, H, shape):
    _compare(monkeypatch, n, n_bins, 9, dict(model=2), H, shape)


def test_model_3_runs_the_generic_word(monkeypatch):
    # (model 3 keeps its extant block behind the death-side entries: 2 x (24 + 2) entries take the next table size)
    ts, te = _data(3000, 24)
    monkeypatch.delenv("LR_P4_RESIDENT", raising=False)
    eng = _engine(ts, te, 9, dict(model=3))
    eng.init()
    assert eng.p4_config() == 0
    eng.close()
    _compare(monkeypatch, 3000, 24, 9, dict(model=3), 72, "short")


@pytest.mark.parametrize("first", ["1", "0"])
def test_checkpoint_crosses_the_switch(monkeypatch, tmp_path, first):
    """A checkpoint taken under one setting of LR_P4_RESIDENT resumes under the other onto the bits of an uninterrupted
    run: the resident groups are a launch's registers, nothing of them is in the workspace."""
    ts, te = _data(N_TWO_WAVES, 128)
    kw = dict(model=0)
    monkeypatch.setenv("LR_P4_RESIDENT", "0")
    ref = _run(ts, te, 9, kw)
    monkeypatch.setenv("LR_P4_RESIDENT", first)
    eng = _engine(ts, te, 9, kw)
    eng.init()
    eng.steps(CUT)
    assert (eng.p4_resident()[0] > 0) == (first == "1")
    eng.save(tmp_path / "cut.npz")
    eng.close()
    monkeypatch.setenv("LR_P4_RESIDENT", "0" if first == "1" else "1")
    eng = _engine(ts, te, 9, kw)
    eng.load(tmp_path / "cut.npz")
    assert (eng.p4_resident()[0] > 0) == (first == "0"), eng.p4_resident()
    eng.steps(N_IT - CUT)
    got = _leavings(eng)
    eng.close()
    _assert_same_run(got, ref, 9)
