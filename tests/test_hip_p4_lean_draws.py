"""The four-chain kernel's lean draw duty (lr_persist4_kernel's LEAN, lr_spec_draw_lean in csrc/lr_step.h: waves 4 and 5
make a chain's state-independent draws one step ahead without the logarithm of the acceptance uniform - it rides in the
free lane 63 of the step's packed logarithm - and make the multiplier draws only for iterations that can read them)
against the same build with LR_P4_LEAN_DRAWS=0, which launches the kernel with lr_spec_draw_both: bit equality of
everything a run leaves - the two state blocks, the snapshot() taken from them and every sampled trace row - after 400
iterations in two launches of 150 + 250.  The Philox addresses, every value a step reads and every floating-point
operation on it are the same, so there is no tolerance.  The harness is that of tests/test_hip_p4_resident.py; every
case asserts from p4_draws() which form ran.

What can go wrong is a multiplier part skipped in an iteration that needs it (the step then multiplies by the stale
factor of an earlier iteration), and the logarithm taken from the wrong lane:
  - 3,000 lineages on 24 bins, 4, 7 and 9 chains from the initial state: every chain starts with ONE rate per process,
    where every selected multiplier move needs its draws whatever r_b is, and then gains and loses shifts - the
    transitions between "one rate" and "several" in the accepted state and in the pending proposal; the nine-chain case
    asserts from the trace that chains were sampled with one rate, with several and with one again
  - models 2 and 3 at that size (model 3 runs the generic word)
  - const_death_rate, where the birth moves reach up to r_a = 0.7 and the death process keeps one rate
  - initial states with LR_KMAX = 32 rates in the death process (tests/helpers/many_shifts.py, H = 264): lane 63 of the
    packed logarithm is taken by a rate and the step runs its second logarithm for the uniform
  - N_ONE_WAVE on 128 bins: waves 4 and 5 run the duty behind the one-block form of their resident trips
  - a checkpoint written under one setting and resumed under the other."""
import numpy as np
import pytest

from test_hip_p4_resident import CUT, N_IT, N_ONE_WAVE, _assert_same_run, _data, _engine, _leavings

pytestmark = pytest.mark.gpu

KMAX = 32           # LR_KMAX, include/literate_hip.h


def _run(ts, te, chains, kw, init=()):
    """400 iterations in two launches -> what the run leaves, and which draw duty made it"""
    eng = _engine(ts, te, chains, kw)
    eng.init(*init)
    draws = eng.p4_draws()
    eng.steps(CUT)
    eng.steps(N_IT - CUT)
    out = _leavings(eng)
    eng.close()
    out["draws"] = draws
    return out


def _compare(monkeypatch, ts, te, chains, kw, H, init=()):
    for name in ("LR_P4_RESIDENT", "LR_P4_PIPE", "LR_P4_LEAN_DRAWS"):
        monkeypatch.delenv(name, raising=False)
    got = _run(ts, te, chains, kw, init)
    monkeypatch.setenv("LR_P4_LEAN_DRAWS", "0")
    ref = _run(ts, te, chains, kw, init)
    assert got["draws"] == "lean" and ref["draws"] == "full", (got["draws"], ref["draws"])
    assert got["name"] == "lr_persist4_kernel<%d, false, false, true>" % H, got["name"]
    assert got["res"] == ref["res"], (got["res"], ref["res"])
    _assert_same_run(got, ref, chains)
    return got


def _k_paths(rows):
    """per chain and process, the sampled numbers of rates: [sample, chain, (KL, KM)]"""
    return rows[:, :, 6:8].astype(int)


@pytest.mark.parametrize("chains", [4, 7, 9])
def test_from_one_rate_per_process(monkeypatch, chains):
    ts, te = _data(3000, 24)
    got = _compare(monkeypatch, ts, te, chains, dict(model=0), 40)
    K = _k_paths(got["rows"])                          # (init() without arguments: one rate per process)
    if chains == 9:
        # some chain and process sampled at one rate, then at several, then at one again
        back = 0
        for c in range(chains):
            for p in range(2):
                k = K[:, c, p]
                up = np.flatnonzero(k >= 2)
                back += len(up) > 0 and bool(np.any(k[up[0]:] == 1))
        print("chains x processes that gained a shift and lost every one again:", back, "of", 2 * chains)
        assert back > 0, K[:, :, 0].T


@pytest.mark.parametrize("model,H", [(2, 40), (3, 72)])
def test_models_2_and_3(monkeypatch, model, H):
    ts, te = _data(3000, 24)
    got = _compare(monkeypatch, ts, te, 9, dict(model=model), H)
    assert got["word"] == (2 if model == 2 else 0), got["word"]        # (model 3: the generic word)


def test_const_death_rate(monkeypatch):
    ts, te = _data(3000, 24)
    got = _compare(monkeypatch, ts, te, 9, dict(model=0, const_death_rate=1), 40)
    K = _k_paths(got["rows"])
    assert np.all(K[:, :, 1] == 1) and np.any(K[:, :, 0] >= 2), K[-1]  # the death process keeps its one rate


def test_full_death_process(monkeypatch):
    """Chains 0, 3, 6, ... start with LR_KMAX death rates: no free lane in the packed logarithm."""
    from helpers import many_shifts as MS
    ts, te = MS.lineages("h264", False)
    init = MS.initial_states("h264")
    assert sum(len(m) == KMAX for m in init[1]) >= MS.C // 3
    got = _compare(monkeypatch, ts, te, MS.C, dict(model=0, poisson_HP=MS.POISSON_HP), 264, init)
    K = _k_paths(got["rows"])
    print("samples with a full death process:", int(np.sum(K[:, :, 1] == KMAX)), "of", K[:, :, 1].size)
    assert np.any(K[:, ::3, 1] == KMAX), K[0, :, 1]                    # ... and sampled with them


def test_behind_the_resident_block(monkeypatch):
    ts, te = _data(N_ONE_WAVE, 128)
    for name in ("LR_P4_RESIDENT", "LR_P4_PIPE", "LR_P4_LEAN_DRAWS"):
        monkeypatch.delenv(name, raising=False)
    eng = _engine(ts, te, 9, dict(model=0))
    eng.init()
    assert eng.p4_pipe() == (1, 10, 2, 2), eng.p4_pipe()               # waves 4, 5 take the block
    eng.close()
    _compare(monkeypatch, ts, te, 9, dict(model=0), 136)


def test_not_without_the_one_block_form(monkeypatch):
    """The lean duty is built into the one-block instantiations only: LR_P4_PIPE=0 runs the full duty."""
    ts, te = _data(3000, 24)
    monkeypatch.delenv("LR_P4_LEAN_DRAWS", raising=False)
    monkeypatch.setenv("LR_P4_PIPE", "0")
    eng = _engine(ts, te, 4, dict(model=0))
    eng.init()
    assert eng.p4_draws() == "full"
    eng.close()


@pytest.mark.parametrize("first", ["1", "0"])
def test_checkpoint_crosses_the_switch(monkeypatch, tmp_path, first):
    """A checkpoint taken under one setting of LR_P4_LEAN_DRAWS resumes under the other onto the bits of an uninterrupted
    run: the draw slots are a launch's LDS, nothing of them is in the workspace."""
    ts, te = _data(3000, 24)
    kw = dict(model=0)
    monkeypatch.delenv("LR_P4_RESIDENT", raising=False)
    monkeypatch.delenv("LR_P4_PIPE", raising=False)
    monkeypatch.setenv("LR_P4_LEAN_DRAWS", "0")
    ref = _run(ts, te, 9, kw)
    assert ref["draws"] == "full"
    monkeypatch.setenv("LR_P4_LEAN_DRAWS", first)
    eng = _engine(ts, te, 9, kw)
    eng.init()
    eng.steps(CUT)
    assert eng.p4_draws() == ("lean" if first == "1" else "full")
    eng.save(tmp_path / "cut.npz")
    eng.close()
    monkeypatch.setenv("LR_P4_LEAN_DRAWS", "0" if first == "1" else "1")
    eng = _engine(ts, te, 9, kw)
    eng.load(tmp_path / "cut.npz")
    assert eng.p4_draws() == ("lean" if first == "0" else "full"), eng.p4_draws()
    eng.steps(N_IT - CUT)
    got = _leavings(eng)
    eng.close()
    _assert_same_run(got, ref, 9)
