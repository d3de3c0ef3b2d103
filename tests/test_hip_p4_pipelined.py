"""The four-chain kernel's one-block form of the resident trips (lr_persist4_kernel's PIPE: a wave that runs ALL its
resident trips takes them as one block of straight-line code without the test and branch per trip,
lr_resident_trips_block in csrc/lr_scan.h) against the same build with LR_P4_PIPE=0, where every resident trip is a
block of its own behind a scalar test: bit equality of everything a run leaves - the two state blocks, the snapshot()
taken from them and every sampled trace row - after 400 iterations in two launches of 150 + 250.  Both forms score the
same groups per lane in the same order through the same operations on every accumulator, so there is no tolerance.

Which waves take the block is a matter of their trip counts, so the sizes are those of tests/test_hip_p4_resident.py
(its docstring derives them; the harness is that file's) and every case asserts, from p4_resident() and p4_pipe(), the
class it means to hit.  The ten scanner waves 6..15 keep NR = 8 trips, waves 4 and 5 (the draw duty) 4, the two helper
waves all of their 5:
  - 60,000 lineages on 128 bins: 6 trips - the ten waves stay trip by trip, waves 4 and 5 run all their four on the
    block, the helpers have 2 trips and stay
  - N_RAGGED: the NR-th trip is ragged - some of the ten waves take the block and some do not, in one block
  - N_ONE_WAVE: all twelve scanner waves and the helpers take the block, one wave in the loop behind
  - 3,000 lineages on 24 bins: no wave takes the block (models 0, 2 and 3, the generic word)
  - model 2 at the small size and at N_ONE_WAVE
  - a checkpoint written under one setting and resumed under the other."""
import numpy as np
import pytest

from test_hip_p4_resident import (CUT, N_IT, N_ONE_WAVE, N_RAGGED, NR, RES_HELP, _assert_same_run, _data, _engine,
                                  _leavings, _run, _trips)

pytestmark = pytest.mark.gpu

NR_DRAW = 4         # resident trips of waves 4, 5 (LR_P4_NR_DRAW, csrc/lr_mcmc.hip)


def _compare(monkeypatch, n, n_bins, chains, kw, H, shape):
    ts, te = _data(n, n_bins)
    monkeypatch.delenv("LR_P4_RESIDENT", raising=False)
    monkeypatch.delenv("LR_P4_PIPE", raising=False)
    eng = _engine(ts, te, chains, kw)
    eng.init()
    pipe = eng.p4_pipe()
    eng.close()
    got = _run(ts, te, chains, kw)
    monkeypatch.setenv("LR_P4_PIPE", "0")
    eng = _engine(ts, te, chains, kw)
    eng.init()
    assert eng.p4_pipe() == (0, 0, 0, 0)
    eng.close()
    ref = _run(ts, te, chains, kw)
    # which path ran: the helper-wave form with the same resident trips both times
    assert got["name"] == "lr_persist4_kernel<%d, false, false, true>" % H, got["name"]
    assert ref["res"] == got["res"], (got["res"], ref["res"])
    k_tot, last, behind = _trips(got["res"])
    assert pipe[0] == 1, pipe
    if shape == "none":           # less than one trip and no helper share: every wave trip by trip
        assert k_tot == 1 and got["res"][3] == 0 and pipe[1:] == (0, 0, 0), (got["res"], pipe)
    elif shape == "six":          # 6 trips: fewer than NR, at least NR_DRAW; 2 helper trips, fewer than RES_HELP
        assert NR_DRAW <= k_tot == 6 < NR and got["res"][3] == 2 and pipe[1:] == (0, 2, 0), (got["res"], pipe)
    elif shape == "ragged":       # the NR-th trip runs on some of the ten waves only
        assert k_tot == NR and 0 < pipe[1] < 10 and pipe[2] == 2, (got["res"], pipe)
    else:                         # every scanning wave takes the block, the first scanner wave alone in the loop behind
        assert shape == "one_wave" and 0 < behind <= 64 and got["res"][1] == RES_HELP and pipe[1:] == (10, 2, 2), (got["res"], pipe)
    _assert_same_run(got, ref, chains)


@pytest.mark.parametrize("n,shape,chains", [(60_000, "six", 9), (N_RAGGED, "ragged", 6), (N_ONE_WAVE, "one_wave", 9)])
def test_waves_with_all_their_resident_trips_and_without(monkeypatch, n, shape, chains):
    _compare(monkeypatch, n, 128, chains, dict(model=0), 136, shape)


@pytest.mark.parametrize("chains", [4, 7])
def test_no_wave_takes_the_block(monkeypatch, chains):
    _compare(monkeypatch, 3000, 24, chains, dict(model=0), 40, "none")


@pytest.mark.parametrize("n,n_bins,H,shape", [(3000, 24, 40, "none"), (N_ONE_WAVE, 128, 136, "one_wave")])
def test_model_2(monkeypatch, n, n_bins, H, shape):
    _compare(monkeypatch, n, n_bins, 9, dict(model=2), H, shape)


def test_model_3_runs_the_generic_word(monkeypatch):
    ts, te = _data(3000, 24)
    monkeypatch.delenv("LR_P4_RESIDENT", raising=False)
    monkeypatch.delenv("LR_P4_PIPE", raising=False)
    eng = _engine(ts, te, 9, dict(model=3))
    eng.init()
    assert eng.p4_config() == 0 and eng.p4_pipe()[0] == 1
    eng.close()
    _compare(monkeypatch, 3000, 24, 9, dict(model=3), 72, "none")


@pytest.mark.parametrize("first", ["1", "0"])
def test_checkpoint_crosses_the_switch(monkeypatch, tmp_path, first):
    """A checkpoint taken under one setting of LR_P4_PIPE resumes under the other onto the bits of an uninterrupted run."""
    ts, te = _data(N_ONE_WAVE, 128)
    kw = dict(model=0)
    monkeypatch.delenv("LR_P4_RESIDENT", raising=False)
    monkeypatch.setenv("LR_P4_PIPE", "0")
    ref = _run(ts, te, 9, kw)
    monkeypatch.setenv("LR_P4_PIPE", first)
    eng = _engine(ts, te, 9, kw)
    eng.init()
    eng.steps(CUT)
    assert (eng.p4_pipe()[0] > 0) == (first == "1")
    eng.save(tmp_path / "cut.npz")
    eng.close()
    monkeypatch.setenv("LR_P4_PIPE", "0" if first == "1" else "1")
    eng = _engine(ts, te, 9, kw)
    eng.load(tmp_path / "cut.npz")
    assert (eng.p4_pipe()[0] > 0) == (first == "0"), eng.p4_pipe()
    eng.steps(N_IT - CUT)
    got = _leavings(eng)
    eng.close()
    _assert_same_run(got, ref, 9)
