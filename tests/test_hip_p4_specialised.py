"""The four-chain kernel's specialised instantiations (lr_persist4_kernel's configuration word: the model class and the
default switches compiled into the stepper waves, the helper waves' table duty and the draw duty) against the generic
instantiation of the same build, forced by LR_P4_GENERIC=1: bit equality of everything a run leaves - the two state blocks
(accepted state, pending proposal, every scalar), the snapshot() taken from them and every sampled trace row - after 400
iterations in two launches of 150 + 250 (a launch cut with carried sums inside).  A specialised word is constant
propagation only, so there is no tolerance: the trajectories are chaotic, one differing bit in a sum ends up here.

Shapes: ~3,000 lineages on 24 bins (table size 40) at 4, 6 and 9 chains - a full block, a block with a ragged pair, a
block with one chain; that input is 240 packed groups, a single trip of the twelve scanner waves and no share for the
helper waves (they take one from ~43k lineages on: lr_set_shares), so two more sizes run 60,000 lineages - 6 trips per
scanner lane, 2 per helper lane - at table sizes 136 (128 bins) and 264 (200 bins)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_IT, CUT = 400, 150
GENERIC, BDI, KEIDING = 0, 1, 2


def _lineages(n, n_bins):
    from literate_amd import synth
    ts, te, _ = synth.make_lineages(n, n_bins=n_bins, n_shifts=3, seed=17)
    return ts, te


_DATA = {}


def _data(n, n_bins):
    if (n, n_bins) not in _DATA:
        _DATA[(n, n_bins)] = _lineages(n, n_bins)
    return _DATA[(n, n_bins)]


def _run(ts, te, chains, kw):
    """400 iterations in two launches -> (configuration word, kernel name, table size, state blocks, snapshot, trace rows)"""
    import torch
    from literate_amd.engine import ChainEngine
    eng = ChainEngine(ts, te, chains, seed=23, s_freq=7, n_trace_slots=N_IT // 7 + 2, engine="persistent4", **kw)
    eng.init()
    eng.steps(CUT)
    eng.steps(N_IT - CUT)
    torch.cuda.synchronize()
    assert eng.layout.persistent == 2
    out = dict(word=eng.p4_config(), name=eng.kernel_name(), H=eng.layout.table_stride, snap=eng.snapshot(),
               S=eng.state_f64.cpu().numpy().copy(), I=eng.state_i32.cpu().numpy().copy(), rows=eng.trace_rows().copy())
    eng.close()
    return out


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    # (trace rows pad with NaN: equal as float64 values where they are numbers, and the same bits everywhere)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(a.view(np.int64), b.view(np.int64))


def _compare(monkeypatch, n, n_bins, chains, kw, word, H):
    ts, te = _data(n, n_bins)
    monkeypatch.delenv("LR_P4_GENERIC", raising=False)
    got = _run(ts, te, chains, kw)
    monkeypatch.setenv("LR_P4_GENERIC", "1")
    ref = _run(ts, te, chains, kw)
    # which instantiation ran: the helper-wave form both times (the kernel name carries no word), the word beside it
    assert got["name"] == ref["name"] == "lr_persist4_kernel<%d, false, false, true>" % H, (got["name"], ref["name"])
    assert got["H"] == H and ref["word"] == GENERIC and got["word"] == word, (got["H"], got["word"], ref["word"])
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


@pytest.mark.parametrize("chains", [4, 6, 9])
@pytest.mark.parametrize("model,word", [(0, BDI), (1, BDI), (2, KEIDING)])
def test_specialised_word_equals_generic_bit_for_bit(monkeypatch, model, word, chains):
    _compare(monkeypatch, 3000, 24, chains, dict(model=model), word, 40)


# (model 3 keeps its extant block behind the death-side entries: 2 x (24 + 2) entries take the next table size)
@pytest.mark.parametrize("kw,H", [(dict(model=3), 72), (dict(model=0, const_rates=1), 40), (dict(model=2, use_rate_HP=0), 40),
                                  (dict(model=0, poisson_HP=1.5), 40)],
                         ids=["model3", "const_rates", "rate_HP_off", "poisson_HP"])
def test_other_settings_run_the_generic_instantiation(monkeypatch, kw, H):
    _compare(monkeypatch, 3000, 24, 6, kw, GENERIC, H)


@pytest.mark.parametrize("n_bins,H,model,word", [(128, 136, 0, BDI), (128, 136, 2, KEIDING), (200, 264, 1, BDI),
                                                 (200, 264, 2, KEIDING)])
def test_specialised_word_with_a_helper_share_at_other_table_sizes(monkeypatch, n_bins, H, model, word):
    _compare(monkeypatch, 60_000, n_bins, 9, dict(model=model), word, H)
