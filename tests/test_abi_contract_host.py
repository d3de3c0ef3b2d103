"""The host side of the buffer-contract tests (tests/helpers/abi_cases.py, tests/test_hip_abi_contract.py), no GPU:

  - the harness against fake entry points on CPU tensors: it passes a well-behaved fake and fails, with the right kind of
    violation, on one that writes a byte into either guard, leaves a defined element unwritten, reads what its buffers held
    into its result, behaves differently on dirty buffers, or writes although it returns an error;
  - the case table against include/literate_hip.h: every entry point that takes a workspace, every *_workspace_bytes and
    every other function whose last argument is the stream has a case, and every case is run by the GPU test file;
  - the host-only size queries over the shapes of the case table: a positive size, and one byte less refused by the
    call's own host-side check (which runs before anything touches a device)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from helpers import abi_cases as A
from helpers import edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the harness against fakes -----------------------------------------------------------------
def _namespace():
    ns = types.SimpleNamespace()
    ns.alloc_workspace = lambda nbytes, device, zero=False, cached=False: torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    ns.alloc_output = lambda shape, dtype, device, zero=False: torch.empty(shape, dtype=dtype, device=device)
    return ns


def _storage_bytes(t):
    """(all bytes of the allocation t lives in, byte offset of t in it)"""
    whole = torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage())
    return whole, t.storage_offset() * t.element_size()


class Fake:
    """An entry point with a 64-byte workspace and an output of five doubles, and the ways it can go wrong."""

    def __init__(self, ns, fault=None):
        self.ns, self.fault = ns, fault

    def __call__(self, error=None):
        ws = self.ns.alloc_workspace(64, "cpu")
        out = self.ns.alloc_output(5, torch.float64, "cpu")
        if ws.numel() < 64:
            if self.fault != "ignores the size":
                raise ValueError("fake: LR_ERR_WORKSPACE")
            return out
        if error:
            if self.fault == "writes before it refuses":
                out[4] = 1.0
            if self.fault == "clears its workspace before it refuses":
                ws.zero_()
            raise ValueError("fake: " + error)
        first, held = int(ws[0]), int(ws[1])
        ws[0] = 0                                    # (its ticket; the rest of the workspace it neither needs nor clears)
        out.copy_(torch.arange(5, dtype=torch.float64))
        whole, off = _storage_bytes(out)
        if self.fault == "writes before its output" and off > 0:
            whole[off - 1] = 0
        if self.fault == "writes behind its output" and off + 40 < whole.numel():
            whole[off + 40] = 0
        if self.fault == "writes far behind its workspace":
            w, o = _storage_bytes(ws)
            if o + 64 + A.GUARD <= w.numel():
                w[o + 64 + A.GUARD - 1] = 0
        if self.fault == "leaves an element unwritten":
            out2 = self.ns.alloc_output(5, torch.float64, "cpu")          # a second output: element 3 is never written
            out2[:3] = 1.0
            out2[4] = 1.0
            return out, out2
        if self.fault == "reads what its workspace held":
            out[2] = float(held)
        if self.fault == "remembers the last call":
            out[1] = 1.0 if first == 7 else 2.0
            ws[0] = 7
        return out


def test_the_harness_passes_a_well_behaved_entry_point():
    ns = _namespace()
    fake = Fake(ns)
    got = A.contract(ns, torch, fake, label="fake")
    assert got.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    A.refuses(ns, torch, fake, "LR_ERR_WORKSPACE", short=1, label="fake")
    A.refuses(ns, torch, lambda: fake("LR_ERR_SIZE"), "LR_ERR_SIZE", label="fake")
    assert ns.alloc_workspace.__name__ == "<lambda>"          # the seam is put back


@pytest.mark.parametrize("fault,kind", [("writes before its output", "guard"), ("writes behind its output", "guard"),
                                        ("writes far behind its workspace", "guard"), ("leaves an element unwritten", "fill"),
                                        ("reads what its workspace held", "fill"), ("remembers the last call", "dirty")])
def test_the_harness_fails_on_a_fake_that(fault, kind):
    ns = _namespace()
    with pytest.raises(A.ContractViolation) as e:
        A.contract(ns, torch, Fake(ns, fault), label="fake")
    assert e.value.kind == kind, e.value
    assert ns.alloc_workspace.__name__ == "<lambda>"


@pytest.mark.parametrize("fault,kind", [("writes before it refuses", "error-wrote"), ("clears its workspace before it refuses", "error-wrote")])
def test_the_harness_fails_on_a_fake_that_refuses_but(fault, kind):
    ns = _namespace()
    fake = Fake(ns, fault)
    with pytest.raises(A.ContractViolation) as e:
        A.refuses(ns, torch, lambda: fake("LR_ERR_SIZE"), "LR_ERR_SIZE", label="fake")
    assert e.value.kind == kind, e.value


def test_the_harness_fails_on_a_fake_that_takes_a_short_workspace_or_returns_another_error():
    ns = _namespace()
    with pytest.raises(A.ContractViolation) as e:
        A.refuses(ns, torch, Fake(ns, "ignores the size"), "LR_ERR_WORKSPACE", short=1, label="fake")
    assert e.value.kind == "accepted"
    with pytest.raises(A.ContractViolation) as e:
        A.refuses(ns, torch, lambda: Fake(ns)("LR_ERR_MODEL"), "LR_ERR_SIZE", label="fake")
    assert e.value.kind == "accepted"


def test_a_partial_extent_needs_its_header_sentence_and_guards_every_byte():
    ns = _namespace()

    def prefix():
        out = ns.alloc_output(8, torch.int64, "cpu")
        out[:3] = 5
        return out[:3]
    with pytest.raises(AssertionError):
        A.contract(ns, torch, prefix, partial="short", label="fake")
    with pytest.raises(A.ContractViolation):
        A.contract(ns, torch, prefix, label="fake")                      # the whole payload is compared without it
    got = A.contract(ns, torch, prefix, partial="elements beyond the count the call reports are not defined", label="fake")
    assert got.tolist() == [5, 5, 5]
    g = A.Guarded(torch, 0xFF, short=1)
    ws, out = g.workspace(100, "cpu"), g.output((2, 3), torch.float64, "cpu")
    assert ws.numel() == 99 and out.shape == (2, 3) and bool(torch.isnan(out).all()) and bool((ws == 0xFF).all())
    assert all(b.whole.numel() == b.nbytes + 2 * A.GUARD and A.GUARD % 4096 == 0 for b in g.bufs)
    g.check_guards()
    g.check_untouched()
    for b in g.bufs:
        for at in (0, A.GUARD - 1, A.GUARD + b.nbytes, b.whole.numel() - 1):
            b.whole[at] = 0
            with pytest.raises(A.ContractViolation):
                g.check_guards()
            b.whole[at] = A.GUARD_BYTE
    g.check_guards()


# ---- the case table against the header -----------------------------------------------------------
def _declarations():
    with open(os.path.join(ROOT, "include", "literate_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|int64_t)\s+(lr_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        out[m.group(1)] = [" ".join(a.split()) for a in m.group(2).split(",")]
    return out


def test_every_entry_point_with_a_workspace_or_a_stream_has_a_case():
    decl = _declarations()
    assert len(decl) > 40 and "lr_bd_loglik_batch" in decl and "lr_mcmc_create" in decl
    need = {n for n, args in decl.items()
            if n.endswith("_workspace_bytes") or "void* workspace" in args or args[-1] == "void* stream"}
    assert {"lr_simulate_bd", "lr_shift_prior", "lr_mcmc_steps", "lr_mcmc_create", "lr_psis_rows_workspace_bytes"} <= need
    covered = {e for eps in A.COVERS.values() for e in eps}
    assert covered <= set(decl), covered - set(decl)
    assert not need - covered, "entry points without a case in tests/helpers/abi_cases.py: %s" % sorted(need - covered)


def test_every_case_is_run_by_the_gpu_test_file():
    import test_hip_abi_contract as T
    assert set(A.COVERS) == set(A.CASES)
    ran = {c[0] for c in T.CHILDREN}
    assert ran == set(A.CASES), set(A.CASES) ^ ran
    runs = {tuple(c[1:]) for c in T.CHILDREN if c[0] == "engine"}
    assert runs == {tuple(r) for r in A.ENGINE_RUNS}
    for name, (kw, chains, want) in A.ENGINES.items():
        assert any(r[0] == name for r in A.ENGINE_RUNS)


# ---- the host-only size queries over the case shapes ------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from literate_amd import _hip
    return _hip.load()


BUF = (C.c_double * 64)()
P = C.c_void_p(C.addressof(BUF))          # a valid host address for every pointer: the calls below return before they use one
WS = -4


@pytest.mark.parametrize("model", [0, 1, 2, 3])
@pytest.mark.parametrize("tiled", [False, True])
def test_loglik_query_covers_every_case_shape(lib, model, tiled):
    shapes = A.loglik_shapes(lib, model, tiled)
    assert len(shapes) > 20
    for n, c, nb in shapes:
        need = lib.lr_bd_loglik_workspace_bytes(n, nb, c, model)
        assert need > 0, (n, c, nb)
        assert lib.lr_bd_loglik_batch(P, P, n, 3.0, nb, P, P, c, model, P, 0.0, P, P, need - 1, None) == WS, (n, c, nb)
    if model == 3 and not tiled:
        top = A.max_bins_model3(lib, 513, 65)
        assert lib.lr_bd_loglik_workspace_bytes(513, top + 1, 65, 3) < 0 < lib.lr_bd_loglik_workspace_bytes(513, top, 65, 3)
        assert (513, 65, top) in shapes


def test_binning_queries_cover_every_case_shape(lib):
    for n, w in A.BIN_EVENTS_SHAPES:
        need = lib.lr_bin_events_workspace_bytes(n, w)
        assert need > 0 and lib.lr_bin_events(P, P, n, P, P, w, P, P, P, P, need - 1, None) == WS, (n, w)
    assert A.ub_edges() == A.BIN_UNIT_BINS
    for nb in A.BIN_UNIT_BINS:
        for n in A.BIN_UNIT_N:
            need = lib.lr_bin_unit_events_workspace_bytes(n, nb)
            assert need == 256 + 8 * (5 * nb + 4)
            assert lib.lr_bin_unit_events(P, P, n, 3.0, nb, P, P, P, P, need - 1, None) == WS, (n, nb)


def test_waic_and_loo_queries_cover_every_case_shape(lib, monkeypatch):
    for model, bins in A.WAIC_BINS.items():
        for nb in bins:
            if nb is None:
                nb = A.max_bins(lambda b: lib.lr_waic_workspace_bytes(A.WAIC_N[1], b, A.WAIC_DRAWS, model))
                assert nb < A.LR_MAX_BINS
            for n in A.WAIC_N:
                sizes = []
                for sl in A.WAIC_SLICES:
                    monkeypatch.setenv("LR_WAIC_SLICES", sl)
                    need = lib.lr_waic_workspace_bytes(n, nb, A.WAIC_DRAWS, model)
                    assert need > 0, (model, nb, n, sl)
                    assert lib.lr_waic_pointwise(P, P, n, 3.0, nb, P, P, A.WAIC_DRAWS, model, P, 0.0, P, P, P, need - 1, None) == WS
                    sizes.append(need)
                assert sizes[1] > sizes[0]                  # several slices keep a state per slice and lineage
    monkeypatch.delenv("LR_WAIC_SLICES")
    for model in (0, 2, 3):
        for S in A.LOO_DRAWS:
            for batch in (None, "4"):
                if batch:
                    monkeypatch.setenv("LR_LOO_BATCH", batch)
                need = lib.lr_loo_workspace_bytes(A.LOO_N, A.LOO_BINS, S, model)
                assert need > 0
                assert lib.lr_loo_pointwise(P, P, A.LOO_N, 3.0, A.LOO_BINS, P, P, S, model, P, 0.0, P, P, P, need - 1, None) == WS
                monkeypatch.delenv("LR_LOO_BATCH", raising=False)
    for S in A.LOO_DRAWS:
        for n in (1, 5):
            need = lib.lr_psis_rows_workspace_bytes(n, S)
            assert need > 0 and lib.lr_psis_rows(P, n, S, P, P, P, need - 1, None) == WS, (n, S)


def test_simulator_and_ess_queries_cover_every_case_shape(lib):
    for R, nb, spb, cap in A.SIMBATCH_SHAPES + [(3, 4, 3, 50)]:
        for q, call in ((lib.lr_simulate_bd_batch_workspace_bytes,
                         lambda k: lib.lr_simulate_bd_batch(P, P, R, nb, spb, P, cap, 1, P, P, P, k, None)),
                        (lib.lr_simulate_dd_batch_workspace_bytes,
                         lambda k: lib.lr_simulate_dd_batch(P, P, 2, 2, R, nb, spb, P, cap, 1, P, P, P, k, None))):
            need = q(R, nb, spb, cap)
            assert need >= 256 and call(need - 1) == WS, (R, nb, spb, cap)
    assert lib.lr_simulate_bd(P, P, 12, 0, 0., 0., 1., 1., 3, 3, 1, P, P, P, None, P, 63, None) == WS      # "workspace: 64 bytes"
    cols = (C.c_int32 * 3)(0, 1, 2)
    for n in A.ESS_ROWS:
        for c in (1, 3):
            need = lib.lr_ess_summary_workspace_bytes(n, c, 3, cols, 3, 0.0, 64)
            assert need > 0, (n, c)
            assert lib.lr_ess_summary(P, n, c, 3, cols, 3, 0.0, 64, P, P, P, P, need - 1, None) == WS, (n, c)


def test_engine_layout_covers_every_engine_of_the_case_table(lib, monkeypatch):
    from literate_amd import _hip
    monkeypatch.setenv("LR_DEVICE_CUS", "256")
    for name, (kw, chains, want) in A.ENGINES.items():
        for unit in (True, False):
            if (name, "unit" if unit else "general", "rj") not in A.ENGINE_RUNS:
                continue
            cfg = E.make_config(0, 0, unit, A.N_BINS, chains, A.N_LINEAGES, E.ENGINES[kw["engine"]])
            cfg.team_request = kw.get("team", 0)
            lay = _hip.McmcLayout()
            assert lib.lr_mcmc_query_layout(C.byref(cfg), C.byref(lay)) == 0
            for k, v in want.items():
                assert getattr(lay, k) == v, (name, unit, k, getattr(lay, k))
            h = C.c_void_p()
            assert lay.total_bytes > 0
            assert lib.lr_mcmc_create(C.byref(cfg), P, P, P, P, lay.total_bytes - 1, C.byref(h)) == WS, (name, unit)
            assert not h.value
