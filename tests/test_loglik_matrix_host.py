"""The host side of the value matrix of lr_bd_loglik_batch (tests/helpers/loglik_cases.py, loglik_ref.py;
tests/test_hip_loglik_matrix.py runs it on the device), no GPU - the cases mean what they claim, by the references alone:

  - the restated plan puts every case on the kernel it names, the named kernels are the full list, and where the library is
    built the restatement equals lr_bd_loglik_plan (host arithmetic);
  - family C's n give the stated last-tile lengths; family D's runs give, by the restated wave map, uniform and non-uniform
    trips, uniform trips outside the window on both sides and cached-bin switches between consecutive uniform trips;
  - the edge block holds every configuration it lists, both table classes of model 3 are populated, the special rate set
    is finite / -inf / nan where it is meant to be;
  - the gather reference and the binned reference agree wherever both are defined;
  - the reference alone stays inside the tolerance: a plain float64 evaluation summed sequentially, forwards and backwards;
  - the tolerance can see a defect: every applicable mutation of the reference moves a chain by >= 100 tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import loglik_cases as K
from helpers import loglik_ref as R
from oracle import literate_oracle as lo

CASES = K.all_cases()
FAMS = "ABCDEF"
LD = np.longdouble


def of(fam):
    return [c for c in CASES if c.family == fam]


@functools.lru_cache(maxsize=None)
def ref(i):
    return CASES[i].reference()


def reference(c):
    return ref(CASES.index(c))


# ---- the census --------------------------------------------------------------------------------
def test_every_case_reaches_the_kernel_it_names():
    for c in CASES:
        assert c.reached() == c.kernel, (c.name, c.reached())
        assert K.FAMILY_ENV[c.family] == c.env
    assert len({(c.family, c.name) for c in CASES}) == len(CASES)
    assert {c.kernel for c in of("A")} == set(K.TILED_KERNELS) and len(K.TILED_KERNELS) == 25
    for kern in K.TILED_KERNELS:                      # every applicable model at each kernel
        models = {c.model for c in of("A") if c.kernel == kern}
        assert models == ({3} if kern.endswith("x2") else {0, 1, 2}), kern
    bins = {c.n_bins for c in of("A") if c.model < 3}
    assert {38, 39, 70, 71, 128, 129, 256, 257, 382, 383, 766, 767, K.LR_MAX_BINS} <= bins
    assert {94, 95, 190, 191, 382, 383, K.MODEL3_MAX_BINS} <= {c.n_bins for c in of("A") if c.model == 3}
    assert {c.t0 for c in CASES} == {3, -7, 1950}
    assert {c.kernel for c in of("F")} == {"fast<8,40>", "fast<8,72>", "fast<8,136>"}
    for c in of("F"):
        assert K.plan(c.n, c.C, c.n_bins, c.model, False).groups in (8, 9)
    assert {c.kernel for c in of("E")} >= {"small", "fast<1,40>", "wide<40>", "generic<1>x1", "generic<1>x2", "generic<8>x2"}
    # no other process gives lr_scan_fast_kernel<8, H> more than one group
    for c in CASES:
        if c.family != "F" and c.kernel.startswith("fast<8"):
            assert K.plan(c.n, c.C, c.n_bins, c.model).groups == 1


def test_size_limits_of_the_restatement():
    assert K.plan(401, 1, K.LR_MAX_BINS + 1, 2) == K.ERR_SIZE != K.plan(401, 1, K.LR_MAX_BINS, 2)
    assert K.plan(401, 1, K.MODEL3_MAX_BINS + 1, 3) == K.ERR_SIZE != K.plan(401, 1, K.MODEL3_MAX_BINS, 3)
    # the one-launch kernel's three boundaries
    assert K.small(1 << 18, 8, 30, 2) and not K.small((1 << 18) + 1, 1, 30, 2)
    assert K.small(2000, 64, 30, 2) and not K.small(2000, 65, 30, 2)
    assert K.small(401, 2, 1918, 2) and not K.small(401, 2, 1919, 2) and K.small(401, 2, 958, 3) and not K.small(401, 2, 959, 3)


@pytest.fixture(scope="module")
def lib():
    from literate_amd import _hip
    return _hip.load()


def test_restated_plan_equals_the_library(lib, monkeypatch):
    monkeypatch.delenv("LR_SCAN_WIDE", raising=False)
    monkeypatch.delenv("LR_SCAN_BLOCKS", raising=False)
    out = (C.c_int32 * 4)()
    shapes = {(c.n, c.C, c.n_bins, c.model) for c in CASES if c.family != "F"}
    shapes |= {(n, c, nb, m) for n in (1, 2047, 2049, 70001) for c in (1, 3, 8, 9, 33, 128) for nb in (1, 38, 39, 128, 129, 256, 257, 383, 767)
               for m in (2, 3)}
    for n, c, nb, m in sorted(shapes):
        p = K.plan(n, c, nb, m)
        assert lib.lr_bd_loglik_plan(n, nb, c, m, out) == 0
        assert tuple(out) == (p.cb, p.tiles, p.H, p.groups), (n, c, nb, m)
    assert lib.lr_bd_loglik_workspace_bytes(401, K.LR_MAX_BINS + 1, 1, 2) == K.ERR_SIZE
    assert lib.lr_bd_loglik_workspace_bytes(401, K.MODEL3_MAX_BINS + 1, 1, 3) == K.ERR_SIZE
    assert lib.lr_bd_loglik_workspace_bytes(401, K.MODEL3_MAX_BINS, 1, 3) > 0


def test_family_B_chain_counts():
    for kern, cb, nb, m in K.B_FAMILIES:
        cs = [c for c in of("B") if c.kernel == kern]
        plans = [K.plan(c.n, c.C, c.n_bins, c.model) for c in cs]
        assert [p.cb for p in plans] == [cb] * 5 and [p.groups for p in plans] == [1, 2, 8, 9, 16]
        assert cs[1].C % cb == cb - 1                                   # a ragged last group
        assert all(p.tiles >= 2 for p in plans)                         # (group, tile) pairs to permute
        assert plans[2].groups & 7 == 0 and plans[4].groups & 7 == 0    # lr_xcd_remap's first branch


def test_family_C_last_tiles():
    for kern, Cn, nb, T in K.C_KERNELS:
        cs = [c for c in of("C") if c.kernel == kern]
        want = [1, 2, 3, 1, 2, 3, 2 * T - 1, 2 * T, 2 * T + 1] + ([4 * T - 1, 4 * T + 1, 6 * T + 1] if T == 512 else [])
        assert [c.last for c in cs if not c.offset] == want == [c.last for c in cs if c.offset]
        for c in cs:
            p = K.plan(c.n, c.C, c.n_bins, c.model)
            assert p.threads == T and K.last_tile(c.n, p) == c.last and (p.tiles == 1) == (c.n <= 3)
        if T == 512:     # trips of the wide kernel's two-deep prefetch in the last tile: pairs at i, i + 2T, i + 4T, i + 6T
            assert sorted({-(-c.last // (2 * T)) for c in cs}) == [1, 2, 3, 4]


def test_family_D_trips():
    for kern, Cn, nb in K.D_KERNELS:
        runs, shuffled, moved = [c for c in of("D") if c.kernel == kern]
        d = runs.data()
        assert np.all(np.diff(d["ts"][:-1]) >= 0)
        tr = K.trips(runs)
        cen = K.trip_census(tr, nb)
        assert cen["uniform"] >= 4 and cen["nonuniform"] >= 4 and cen["before"] >= 1 and cen["after"] >= 1, cen
        assert cen["consecutive"] >= 1, cen
        lens = np.diff(np.flatnonzero(np.diff(np.floor(d["ts"][:-1])) != 0))
        assert {1, 64, 127, 128, 129, 300} <= set(lens.tolist())
        # a run boundary inside a wave's 128 lineages, and the two neighbours of the sorted case
        assert any(not t[3] for t in tr)
        assert K.trip_census(K.trips(moved), nb)["uniform"] == cen["uniform"] - 1
        dm = moved.data()
        assert int(np.sum(dm["ts"] != d["ts"])) == 1
        assert K.trip_census(K.trips(shuffled), nb)["uniform"] == 0
        assert np.array_equal(np.sort(shuffled.data()["ts"]), np.sort(d["ts"]))


# ---- the lineages and the rates ------------------------------------------------------------------
def test_edge_block_holds_every_configuration():
    seen_end = set()
    for c in CASES:
        if c.layout or c.n < K.N_EDGE3 or c.masked_last_bin:
            continue
        d = c.data()
        t0, W = float(c.t0), c.n_bins
        k = K.N_EDGE3 if c.model == 3 else K.N_EDGE2
        s, e = d["ts"][:k], d["te"][:k]
        inw = lambda x: (x >= t0) & (x < t0 + W)          # noqa: E731
        whole = lambda x: x == np.floor(x)                 # noqa: E731
        conf = dict(ts_edge=whole(s) & inw(s) & ~whole(e), te_edge=whole(e) & (e > t0) & (e <= t0 + W) & ~whole(s),
                    same_edge=(s == e) & whole(s), same_inside=(s == e) & ~whole(s), ts_before=(s < t0) & inw(e), ts_t0=s == t0,
                    ts_end=s == t0 + W, te_t0=e == t0, te_end=e == t0 + W, te_beyond=inw(s) & (e > t0 + W),
                    before=e < t0, after=s > t0 + W, spanning=(s < t0) & (e > t0 + W), far_neg18=s == -1e18, far_pos18=e == 1e18,
                    far_neg300=s == -1e300, far_pos300=e == 1e300)
        if c.model == 3:
            x = c.end_time
            conf.update(te_at_end=e == x, te_below_end=e == np.nextafter(x, -np.inf), te_above_end=e > x)
            seen_end.add((c.end, x == np.floor(x), x < t0, x > t0 + W))
            extant = d["te"] >= x
            if c.end in (None, "frac"):
                assert 0.1 <= extant.mean() <= 0.9, (c.name, extant.mean())
            elif c.end == "before":
                assert np.sum(~extant) <= 3 and extant[K.N_EDGE3:].all()
            else:
                assert np.sum(extant) <= 6 and not extant[K.N_EDGE3:].any()
        for name, m in conf.items():
            assert m.any(), (c.name, name)
    assert seen_end == {(None, True, False, False), ("frac", False, False, False), ("before", True, True, False),
                        ("beyond", False, False, True)}


def test_special_rate_sets():
    sp = [c for c in CASES if c.special]
    assert {c.model for c in sp if c.family == "A"} == {0, 1, 2, 3} == {c.model for c in sp if c.family == "E"}
    for c in sp:
        d = c.data()
        js, _, je, _ = lo.lineage_bins(d["ts"], d["te"], float(c.t0), c.n_bins)
        assert not np.any(je == K.NO_DEATH_BIN + 1) and d["mu"][0, K.NO_DEATH_BIN] == 0
        assert np.any(js == K.ZERO_BIRTH_BIN + 1) and d["lam"][1, K.ZERO_BIRTH_BIN] == 0
        want = reference(c)[0]
        assert np.isfinite(want[0]) and want[1] == -np.inf and np.isnan(want[2]) and np.isfinite(want[3:]).all()
        if c.model < 2:
            assert d["br"][K.ZERO_BR_BIN] == 0 and np.any(js == K.ZERO_BR_BIN + 1) and np.any(je == K.ZERO_BR_BIN + 1)
            assert d["br"][K.NAN_BIN] > 0


# ---- the references --------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMS)
def test_gather_and_binned_references_agree(fam):
    done = 0
    for c in of(fam):
        if c.n * c.n_bins > 2e6:
            continue
        d = c.data()
        b = R.binned(d["ts"], d["te"], c.t0, d["lam"], d["mu"], c.model, d["br"], c.end_time)
        if b is None:
            assert (c.special or c.masked_last_bin) and c.model < 2
            continue
        want, tol, L, A = reference(c)
        out, scale = b
        fin = np.isfinite(out)
        assert fin.sum() >= (c.C - 3 if c.special else c.C), c.name
        bound = tol + R.binned_tolerance(scale, c.n, c.n_bins)
        err = np.abs(out[fin].astype(LD) - want[fin]).astype(np.float64)
        assert np.all(err <= bound[fin]), (c.name, float((err / bound[fin]).max()))
        done += 1
    assert done >= (4 if fam != "F" else 3)


@pytest.mark.parametrize("fam", FAMS)
def test_reference_alone_stays_inside_the_tolerance(fam):
    worst = 0.0
    for c in of(fam):
        d = c.data()
        want, tol, L, A = reference(c)
        Lp, cst = R.plain(d["ts"], d["te"], c.t0, d["lam"], d["mu"], c.model, d["br"], c.end_time)
        for rev in (False, True):
            r = R.ratios(R.seq_sum(Lp, cst, rev), want, tol)
            assert r.max() <= 1.0, (c.name, rev, r.max())
            worst = max(worst, r.max())
    print("family %s: plain float64, sequential: worst error / tolerance %.3f" % (fam, worst))


def mutation_lineage(c, d, side):
    js, _, je, _ = lo.lineage_bins(d["ts"], d["te"], float(c.t0), c.n_bins)
    j = js if side == "birth_bin" else je
    ok = (j >= 1) & (j <= c.n_bins - 1)
    if c.model == 3 and side == "death_bin":
        ok &= d["te"] < c.end_time
    idx = np.flatnonzero(ok)
    return int(idx[-1]) if len(idx) else None


@pytest.mark.parametrize("fam", FAMS)
def test_tolerance_sees_every_mutation(fam):
    seen = set()
    for c in of(fam):
        d = c.data()
        want, tol, L, A = reference(c)
        fin = np.isfinite(want.astype(np.float64))
        p = K.plan(c.n, c.C, c.n_bins, c.model, c.env.get("LR_SCAN_WIDE") != "0")
        applied = 0
        for mut in R.MUTATIONS:
            kw = {}
            if mut in ("birth_bin", "death_bin"):
                kw["lineage"] = mutation_lineage(c, d, mut)
            if mut == "swap_chains" and c.kernel != "small" and p.groups >= 2 and fin[0] and fin[p.cb]:
                kw["swap"] = (0, p.cb)
            res = R.plain(d["ts"], d["te"], c.t0, d["lam"], d["mu"], c.model, d["br"], c.end_time, mutate=mut, **kw)
            if res is None:
                continue
            Lm, cst = res
            with np.errstate(invalid="ignore"):
                got = np.sum(Lm.astype(LD), axis=0) + cst
                moved = np.abs(got - want).astype(np.float64)[fin] / tol[fin]
            moved = np.where(np.isnan(moved), np.inf, moved)
            assert moved.max() >= 100.0, (c.name, mut, float(moved.max()))
            applied += 1
            seen.add(mut)
        assert applied >= 1, c.name
    print("family %s: mutations applied: %s" % (fam, sorted(seen)))
    if fam == "A":                                   # (its chain counts make one group: the swap belongs to B and F)
        assert seen == set(R.MUTATIONS) - {"swap_chains"}
    if fam in "BF":
        assert "swap_chains" in seen
