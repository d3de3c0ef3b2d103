"""The case tables of lr_ade_classes and lr_ade_profile, shared by tests/test_ade_host.py (the restatement against itself)
and tests/test_hip_ade.py, whose GPU cases run here, each in a child process of its own (under the test's time limit):

    python tests/helpers/ade_cases.py CASE [ARGS...]

A case prints its figures, asserts, and exits 0 - or raises.  The yardstick is tests/helpers/ade_ref.py.

Classes: counts, compared with np.array_equal.  Shapes: a trip of the kernel takes TILE = 1024 lineages (n around 64, 256 and
1024, and 4097: five trips); the class table is counted in LDS up to 64 bins and by atomics on the table itself from 65.
Profile: tolerances as the issue sets them - |l^ - l^_ref| <= 1e-9 sum n |class term| at the reference optimum, c^ within 1e-7
relative where it is finite and positive.  A thread keeps its first four classes in registers, so more than 1024 classes
(`a65`, `a512`) take the kernel's other path; `a1` .. `a3` are the smallest tables."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import ade_ref as ref  # noqa: E402
from helpers import ppc_age_cases as P  # noqa: E402  (its lineages: the edge ones first, year resolution or continuous)

T0 = P.T0
TILE = 1024
LL_TOL, C_TOL = 1e-9, 1e-7
CLASS_N = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
CLASS_BINS = (1, 2, 3, 40, 64, 65, 512)


def say(*a):
    print(*a)
    sys.stdout.flush()


def grid(G):
    """G shapes: 1; 1/8 and 8; or equally spaced in log shape over 1/8 .. 8 (odd G: the middle one is 1)"""
    if G == 1:
        return np.array([1.0])
    if G == 2:
        return np.array([0.125, 8.0])
    g = 2.0 ** np.linspace(-3.0, 3.0, G)
    assert g[0] == 0.125 and g[-1] == 8.0 and g[G // 2] == 1.0
    return g


def rates(rng, S, n_bins, scale=1.0):
    """S draws of death rates, log-normal around 0.2"""
    return np.exp(rng.normal(size=(S, n_bins)) * 0.7 - 1.5) * scale


# name -> (lineages, n_bins, draws S, shapes G, kind, factor on the rates, seed)
PROFILE = {
    "a1": (50, 1, 1, 1, "continuous", 1.0, 201),
    "a2": (200, 2, 2, 2, "year", 1.0, 202),
    "a3": (300, 3, 3, 65, "continuous", 1.0, 203),
    "a40": (4097, 40, 33, 2, "year", 1.0, 204),
    "a40_tiny": (4097, 40, 2, 65, "year", 1e-12, 204),
    "a40_huge": (4097, 40, 2, 65, "year", 1e6, 204),
    "a65": (30000, 65, 2, 129, "continuous", 1.0, 205),
    "a512": (20000, 512, 3, 2, "year", 1.0, 206),
    "a512_one": (20000, 512, 1, 1, "continuous", 1.0, 207),
}
GROUPS = {"small": ("a1", "a2", "a3", "a40"), "scaled": ("a40_tiny", "a40_huge"), "large": ("a65", "a512", "a512_one")}
assert sorted(sum(GROUPS.values(), ())) == sorted(PROFILE)


def profile_inputs(name):
    """(dead, cens, mu [S, A], shapes [G]) of a case; the rates of the scaled cases are a40's own times the factor"""
    n, A, S, G, kind, f, seed = PROFILE[name]
    rng = np.random.default_rng(seed)
    ts, te = P.lineages(rng, n, A, kind)
    dead, cens, _ = ref.classes(ts, te, T0, A)
    return dead, cens, rates(rng, S, A) * f, grid(G)


def check_profile(label, got, want, mag):
    """got (ll, c, flag) against the restatement's, and `mag` = sum n |class term| at its optimum"""
    ll, c, flag = (np.asarray(x) for x in got)
    wll, wc, wflag = want
    assert np.array_equal(flag, wflag), (label, flag, wflag)
    assert np.array_equal(np.isnan(ll), np.isnan(wll)) and np.array_equal(np.isnan(c), np.isnan(wc)), label
    ok = ~np.isnan(wll)
    err = np.abs(ll[ok] - wll[ok])
    bound = LL_TOL * mag[ok]
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0))) if ok.any() else 0.0
    fin = ok & np.isfinite(wc) & (wc > 0)
    rel = np.abs(c[fin] / wc[fin] - 1.0)
    say("%s: %d pairs, worst |dl| / bound %.3g (worst |dl| %.3g), worst relative error of c %.3g"
        % (label, int(ok.sum()), worst, float(err.max()) if ok.any() else 0.0, float(rel.max()) if fin.any() else 0.0))
    assert (err <= bound).all(), (label, err.max())
    assert (rel <= C_TOL).all(), (label, rel.max())
    assert np.array_equal(c[ok & ~fin], wc[ok & ~fin]), label               # 0 and +inf: exactly


# ------------------------------------------------------------------------------------------------
# the GPU cases
# ------------------------------------------------------------------------------------------------
def same(what, got, want_):
    ok = got == want_ if isinstance(got, (list, bytes)) else np.array_equal(np.asarray(got), np.asarray(want_))
    say("%s: %s" % (what, "identical" if ok else "DIFFER"))
    assert ok, (what, got, want_)


def bits(ts):
    return [np.ascontiguousarray(t.cpu().numpy()).tobytes() for t in ts]


def dev_profile(dead, cens, mu, shapes, out=None):
    import torch
    from literate_amd import ops
    return ops.ade_profile(torch.as_tensor(dead, device="cuda"), torch.as_tensor(cens, device="cuda"),
                           torch.as_tensor(mu, device="cuda"), torch.as_tensor(shapes, device="cuda"), out=out)


def host(out):
    return tuple(t.cpu().numpy() for t in out)


def case_classes():
    """every (n, bins, kind) of the table against the restatement, and a second call on the dirtied outputs"""
    import torch
    from literate_amd import ops
    rng = np.random.default_rng(301)
    for A in CLASS_BINS:
        for n in CLASS_N:
            for kind in ("year", "continuous"):
                ts, te = P.lineages(rng, n, A, kind)
                want = ref.classes(ts, te, T0, A)
                ts_d, te_d = torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda")
                out = ops.ade_classes(ts_d, te_d, T0, A)
                got = host(out)
                ok = all(np.array_equal(g, w) for g, w in zip(got, want))
                for t, fill in zip(out, (-7, 1 << 40, 3)):
                    t.fill_(fill)
                again = ops.ade_classes(ts_d, te_d, T0, A, out=out)
                assert again[0].data_ptr() == out[0].data_ptr()
                ok2 = all(np.array_equal(g, w) for g, w in zip(host(again), want))
                say("bins %d n %d %s: used %d, dead %d, censored %d: %s, dirty outputs %s"
                    % (A, n, kind, want[2][0], want[0].sum(), want[1].sum(), "identical" if ok else "DIFFER",
                       "identical" if ok2 else "DIFFER"))
                assert ok and ok2, (A, n, kind)
                assert want[0].sum() + want[1].sum() == want[2][0] and want[2].sum() == n
    # the edge lineages alone, one by one
    es, ee = P.edge_lineages(40)
    got = host(ops.ade_classes(es, ee, T0, 40))
    want = ref.classes(es, ee, T0, 40)
    same("edge lineages", [g.tolist() for g in got], [w.tolist() for w in want])
    assert want[2].tolist() == [7, 8] and want[0][0, 39] == 1 and want[1][0] == 2 and want[1][39] == 2


def case_profile(group):
    """every case of the group against the restatement; the same bits from a second call on the dirtied outputs; in the
    scaled group also the device against itself: rates times f give c^ / f and the same l^"""
    base = None
    for name in GROUPS[group]:
        dead, cens, mu, shapes = profile_inputs(name)
        want = ref.profile(dead, cens, mu, shapes, with_scale=True)
        out = dev_profile(dead, cens, mu, shapes)
        got = host(out)
        say("%s: %d classes, %d deaths" % (name, int((dead > 0).sum()), int(dead.sum())))
        check_profile(name, got, want[:3], want[3])
        assert not want[2].any() and np.isfinite(got[0]).all()
        first = bits(out)
        for t, fill in zip(out, (float("nan"), 1e300, 7)):
            t.fill_(fill)
        again = dev_profile(dead, cens, mu, shapes, out=out)
        assert again[0].data_ptr() == out[0].data_ptr()
        same(name + " second call on dirty outputs", bits(again), first)
        if group == "scaled":
            f = PROFILE[name][5]
            if base is None:
                base = host(dev_profile(dead, cens, mu / f, shapes))
            dl = np.abs(got[0] - base[0]) / (LL_TOL * want[3])
            dc = np.abs(got[1] * f / base[1] - 1.0)
            say("%s against the unscaled rates on the device: worst |dl| / bound %.3g, worst relative error of c f %.3g"
                % (name, dl.max(), dc.max()))
            assert (dl <= 1.0).all() and (dc <= C_TOL).all()


BIG_SHIFT, BIG_SHAPES = 28, (0.125, 1.0, 8.0)


def case_big_counts():
    """counts beyond 32 bits: a40's table times 2^28 against the table itself.  A power of two scales every product and sum
    of the likelihood exactly and the iteration works on log c, which does not move: the same c^ bit for bit, l^ times 2^28
    exactly.  A profile that read a count clamped to 32 bits would fail both."""
    dead, cens, mu, _ = profile_inputs("a40")
    mu, shapes = mu[:2], np.array(BIG_SHAPES)
    big_dead, big_cens = dead << BIG_SHIFT, cens << BIG_SHIFT
    most = int((big_cens + big_dead.sum(axis=1)).max())
    say("largest number of lineages of one birth bin: %d, largest class: %d" % (most, int(big_dead.max())))
    assert most > 2 ** 31 - 1
    base, big = host(dev_profile(dead, cens, mu, shapes)), host(dev_profile(big_dead, big_cens, mu, shapes))
    assert np.isfinite(base[0]).all() and (base[1] > 0).all()
    same("flags", [base[2].tolist(), big[2].tolist()], [[0, 0], [0, 0]])
    same("c of the scaled table", big[1].tobytes(), base[1].tobytes())
    same("l of the scaled table against 2^%d l" % BIG_SHIFT, big[0], float(1 << BIG_SHIFT) * base[0])


def case_degenerate():
    """no observed death: c = 0, l = 0; three deaths in the one class of one bin and nothing censored: c = +inf, l = 0"""
    rng = np.random.default_rng(311)
    A = 12
    ts = T0 + rng.random(200) * A
    dead, cens, tot = ref.classes(ts, np.full(200, np.inf), T0, A)
    assert dead.sum() == 0 and cens.sum() == 200
    mu = rates(rng, 3, A)
    got = host(dev_profile(dead, cens, mu, grid(65)))
    same("no deaths", [g.tolist() for g in got], [np.zeros((3, 65)).tolist(), np.zeros((3, 65)).tolist(), [0, 0, 0]])
    ts = T0 + np.array([0.1, 0.2, 0.3])
    dead, cens, tot = ref.classes(ts, ts + 0.05, T0, 1)
    assert dead.tolist() == [[3]] and cens.tolist() == [0]
    got = host(dev_profile(dead, cens, np.array([[0.3], [2.0]]), grid(2)))
    want = ref.profile(dead, cens, np.array([[0.3], [2.0]]), grid(2))
    same("three deaths in one bin, nothing censored", [g.tolist() for g in got], [w.tolist() for w in want])
    assert np.isinf(got[1]).all() and (got[0] == 0).all()


def case_flags():
    """NaN, inf, a negative rate, a zero rate in a bin that holds a death: NaN rows, flag 1, and the other draws' rows the
    bits they are in a call without the flagged draws; a zero rate in a bin without a death is no flag; a shape that is not
    finite or <= 0 is a NaN column and leaves the others alone"""
    rng = np.random.default_rng(321)
    n, A, S = 1500, 20, 9
    ts, te = P.lineages(rng, n, A, "continuous")
    last = (te <= T0 + A) & (np.floor(te - T0) >= A - 1)
    te[last] += 2.0                                              # nobody dies in the last bin
    dead, cens, _ = ref.classes(ts, te, T0, A)
    assert dead.sum() > 100 and not np.any([dead[jb, A - 1 - jb] for jb in range(A)])
    good = rates(rng, S, A)
    shapes = grid(5)
    base = host(dev_profile(dead, cens, good, shapes))
    assert not base[2].any() and np.isfinite(base[0]).all()
    je = int(np.nonzero(dead[0])[0][0])
    mu = good.copy()
    for s, (b, v) in zip((0, 3, 5, 8), ((3, np.nan), (A - 1, np.inf), (0, -1e-300), (je, 0.0))):
        mu[s, b] = v
    mu[6, A - 1] = 0.0                                           # a zero rate where nobody died: the draw stays
    got = host(dev_profile(dead, cens, mu, shapes))
    want = ref.profile(dead, cens, mu, shapes)
    same("flags", got[2].tolist(), [1, 0, 0, 1, 0, 1, 0, 0, 1])
    same("flags of the restatement", want[2].tolist(), got[2].tolist())
    keep = got[2] == 0
    assert np.isnan(got[0][~keep]).all() and np.isnan(got[1][~keep]).all() and np.isfinite(got[0][keep]).all()
    for s in (1, 2, 4, 7):
        same("draw %d beside flagged draws" % s, [got[0][s].tobytes(), got[1][s].tobytes()], [base[0][s].tobytes(), base[1][s].tobytes()])
    alone = host(dev_profile(dead, cens, mu[keep], shapes))
    same("the kept draws in a call of their own", bits_np(alone[:2]), bits_np([got[0][keep], got[1][keep]]))
    assert not np.array_equal(got[0][6], base[0][6])             # (the zero rate did change that draw's likelihood)
    bad = np.array([0.5, np.nan, 1.0, 0.0, -1.0, np.inf, 2.0])
    got = host(dev_profile(dead, cens, good, bad))
    ok = np.array([True, False, True, False, False, False, True])
    assert np.isnan(got[0][:, ~ok]).all() and np.isnan(got[1][:, ~ok]).all() and not got[2].any()
    clean = host(dev_profile(dead, cens, good, bad[ok]))
    same("the good shapes beside the bad ones", bits_np([got[0][:, ok], got[1][:, ok]]), bits_np(clean[:2]))


def bits_np(arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


def case_arguments():
    """every refusal returns its code, in the documented order, and leaves the outputs untouched"""
    import torch
    from literate_amd import _hip, ops
    lib = _hip.load()
    E, P_ = _hip, _hip.ptr
    n, A, S, G = 10, 20, 8, 5
    ts = torch.rand(n, dtype=torch.float64, device="cuda") + T0
    te = ts + 1.0
    dead = torch.full((A, A), 123, dtype=torch.int64, device="cuda")
    cens = torch.full((A,), 123, dtype=torch.int64, device="cuda")
    tot = torch.full((2,), 123, dtype=torch.int64, device="cuda")

    def classes(**kw):
        a = dict(ts=P_(ts), te=P_(te), n=n, t0=T0, nb=A, dead=P_(dead), cens=P_(cens), tot=P_(tot))
        a.update(kw)
        return _hip.launch(lib.lr_ade_classes, ts.device, a["ts"], a["te"], a["n"], a["t0"], a["nb"], a["dead"], a["cens"], a["tot"])

    for kw, code in ((dict(ts=None), E.LR_ERR_NULL), (dict(te=None), E.LR_ERR_NULL), (dict(dead=None), E.LR_ERR_NULL),
                     (dict(cens=None), E.LR_ERR_NULL), (dict(tot=None), E.LR_ERR_NULL), (dict(n=0), E.LR_ERR_SIZE),
                     (dict(n=-2), E.LR_ERR_SIZE), (dict(nb=0), E.LR_ERR_SIZE), (dict(nb=E.LR_ADE_MAX_BINS + 1), E.LR_ERR_SIZE),
                     (dict(t0=T0 + 0.5), E.LR_ERR_T0), (dict(t0=float("nan")), E.LR_ERR_T0),
                     (dict(ts=None, n=0, t0=0.5), E.LR_ERR_NULL), (dict(n=0, t0=0.5), E.LR_ERR_SIZE)):
        rc = classes(**kw)
        say("lr_ade_classes %s -> %d" % (sorted(kw), rc))
        assert rc == code, (kw, rc, code)
    torch.cuda.synchronize()
    assert bool((dead == 123).all()) and bool((cens == 123).all()) and bool((tot == 123).all())
    assert classes() == 0
    torch.cuda.synchronize()
    assert tot.tolist() == [n, 0] and int(dead.sum() + cens.sum()) == n

    mu = torch.rand(S, A, dtype=torch.float64, device="cuda") + 0.1
    sh = torch.as_tensor(grid(G), device="cuda")
    ll = torch.full((S, G), 123.0, dtype=torch.float64, device="cuda")
    c = torch.full((S, G), 123.0, dtype=torch.float64, device="cuda")
    flag = torch.full((S,), 123, dtype=torch.int32, device="cuda")
    need = lib.lr_ade_profile_workspace_bytes(A, S, G)
    assert need > 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")

    def profile(**kw):
        a = dict(dead=P_(dead), cens=P_(cens), nb=A, mu=P_(mu), S=S, sh=P_(sh), G=G, ll=P_(ll), c=P_(c), flag=P_(flag), ws=P_(ws),
                 wsb=need)
        a.update(kw)
        return _hip.launch(lib.lr_ade_profile, ts.device, a["dead"], a["cens"], a["nb"], a["mu"], a["S"], a["sh"], a["G"], a["ll"],
                           a["c"], a["flag"], a["ws"], a["wsb"])

    for kw, code in ((dict(dead=None), E.LR_ERR_NULL), (dict(cens=None), E.LR_ERR_NULL), (dict(mu=None), E.LR_ERR_NULL),
                     (dict(sh=None), E.LR_ERR_NULL), (dict(ll=None), E.LR_ERR_NULL), (dict(c=None), E.LR_ERR_NULL),
                     (dict(flag=None), E.LR_ERR_NULL), (dict(ws=None), E.LR_ERR_NULL), (dict(S=0), E.LR_ERR_SIZE),
                     (dict(S=-1), E.LR_ERR_SIZE), (dict(G=0), E.LR_ERR_SIZE), (dict(nb=0), E.LR_ERR_SIZE),
                     (dict(nb=E.LR_ADE_MAX_BINS + 1), E.LR_ERR_SIZE), (dict(S=1 << 16, G=1 << 15), E.LR_ERR_SIZE),
                     (dict(wsb=need - 1), E.LR_ERR_WORKSPACE), (dict(wsb=0), E.LR_ERR_WORKSPACE),
                     (dict(dead=None, S=0, wsb=0), E.LR_ERR_NULL), (dict(S=0, wsb=0), E.LR_ERR_SIZE)):
        rc = profile(**kw)
        say("lr_ade_profile %s -> %d" % (sorted(kw), rc))
        assert rc == code, (kw, rc, code)
    assert lib.lr_ade_profile_workspace_bytes(A, 1 << 16, 1 << 15) == E.LR_ERR_SIZE
    assert lib.lr_ade_profile_workspace_bytes(A, (1 << 16) - 1, 1 << 15) > 0
    assert lib.lr_ade_profile_workspace_bytes(0, S, G) == E.LR_ERR_SIZE and lib.lr_ade_profile_workspace_bytes(A, S, 0) == E.LR_ERR_SIZE
    torch.cuda.synchronize()
    assert bool((ll == 123.0).all()) and bool((c == 123.0).all()) and bool((flag == 123).all()) and bool((ws == 0x5A).all())
    assert profile() == 0
    torch.cuda.synchronize()
    assert not flag.any() and bool(torch.isfinite(ll).all()) and bool((c > 0).all())
    for call, what in ((lambda: ops.ade_classes(ts, te, T0 + 0.25, A), "lr_ade_classes: LR_ERR_T0"),
                       (lambda: ops.ade_classes(ts, te, T0, E.LR_ADE_MAX_BINS + 1), "lr_ade_classes: LR_ERR_SIZE"),
                       (lambda: ops.ade_profile(dead, cens, mu[:0], sh), "LR_ERR_SIZE")):
        try:
            call()
        except ValueError as ex:
            assert what in str(ex), (what, ex)
        else:
            raise AssertionError(what)


def case_contract():
    """the buffer contract (helpers.abi_cases.contract / refuses) for the two entry points: workspace and outputs of exactly
    the queried and documented size, fills 0x00 and 0xFF, guards intact, a second call on the dirty buffers, a workspace one
    byte short, one argument error"""
    import torch
    from literate_amd import ops
    from helpers.abi_cases import contract, refuses
    rng = np.random.default_rng(331)
    for A, n, S, G in ((1, 1, 1, 1), (40, TILE + 1, 3, 5), (64, TILE - 1, 2, 2), (65, 6000, 2, 3), (512, 2 * TILE + 1, 2, 2)):
        ts, te = P.lineages(rng, n, A, "continuous" if A % 2 else "year")
        ts_d, te_d = torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda")
        want = ref.classes(ts, te, T0, A)
        label = "ade_classes bins %d n %d" % (A, n)
        out = contract(ops, torch, lambda: ops.ade_classes(ts_d, te_d, T0, A), label=label)
        same(label, [t.tolist() for t in host(out)], [w.tolist() for w in want])
        refuses(ops, torch, lambda: ops.ade_classes(ts_d, te_d, T0 + 0.5, A), "LR_ERR_T0", label=label, entry="lr_ade_classes")
        mu_d, sh_d = torch.as_tensor(rates(rng, S, A), device="cuda"), torch.as_tensor(grid(G), device="cuda")
        label = "ade_profile bins %d draws %d shapes %d" % (A, S, G)
        contract(ops, torch, lambda: ops.ade_profile(out[0], out[1], mu_d, sh_d), label=label)
        refuses(ops, torch, lambda: ops.ade_profile(out[0], out[1], mu_d, sh_d), "LR_ERR_WORKSPACE", short=1, label=label,
                entry="lr_ade_profile")
        say(label + ": contract kept")


# the recovery case of tests/test_ade_host.py: 30 bins, 100 births per bin, rates 0.05 / 0.15 / 0.3 by thirds
REC_BINS, REC_BIRTHS, REC_SEED = 30, 100, 20261018
REC_MU = np.repeat([0.05, 0.15, 0.3], 10)


def recovery_data(k, c):
    return ref.simulate(np.random.default_rng(REC_SEED), REC_BINS, REC_BIRTHS, REC_MU, k, c)


def case_recovery():
    """fit_rates on the device against fit_rates on the restatement, on the host test's recovery data.  An error d in l^
    moves the coarse parabola's vertex by about h d / |second difference|: d <= 1e-9 x 1e4, h = 0.065 and a second difference
    of (h / se)^2 ~ 10 give 1e-7 in log shape, and the fine grid's ends and nodes move with it: 1e-6 relative is the bound"""
    from literate_amd import ade
    ts, te = recovery_data(0.6, 1.5)
    mu = np.stack([REC_MU, REC_MU])
    want = ade.fit_rates(ts, te, 0.0, mu, profile=ref.Restated())
    got = ade.fit_rates(ts, te, 0.0, mu)
    for k in ade.FIT_INTS:
        assert got.fit[k] == want.fit[k], k
    for k in ("shape_mean", "shape_median", "shape_q025", "shape_q975", "shape_ml_mean", "const_shape_ml", "const_shape_q025",
              "const_shape_q975", "const_scale", "const_mean_longevity", "lr_mean", "const_lr"):
        say("   %s: device %.15g, restatement %.15g" % (k, got.fit[k], want.fit[k]))
        assert abs(got.fit[k] / want.fit[k] - 1.0) <= 1e-6, k
    assert got.fit["shape_q025"] <= 0.6 <= got.fit["shape_q975"]
    assert abs(got.fit["edge_mass"] - want.fit["edge_mass"]) <= 1e-6 and abs(got.fit["p_shape_lt_1"] - want.fit["p_shape_lt_1"]) <= 1e-6


# ------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------
N_IT, S_FREQ, CH, DRAWS = 2000, 10, 4, 50
OTHER = ["--ppc_age", "0.2", "--ppc_age_draws", "20", "--waic", "0.2", "--waic_draws", "32"]
OTHER_FILES = ("_PPC_age.tsv", "_PPC_age_fit.tsv", "_WAIC.tsv", "_WAIC_pointwise.npz")


def _run_cli(script, data, extra, with_ade=True):
    cmd = [sys.executable, os.path.join(ROOT, script), "-d", data, "-TBP", "-n", str(N_IT), "-s", str(S_FREQ), "-p", "1000",
           "-seed", "31", "--chains", str(CH)] + (["--ade", "0.2", "--ade_draws", str(DRAWS)] if with_ade else []) + extra
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_PPC_AGE_SLICES", "LR_WAIC_SLICES"):
        env.pop(k, None)
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=280, env=env).stdout
    line = [l for l in out.splitlines() if l.startswith("ADE:")]
    say(line)
    if with_ade:
        assert len(line) == 1 and "_ADE.tsv" in line[0] and "_ADE_shape.tsv" in line[0] and "%d draws" % DRAWS in line[0]
        assert "edge_mass" in line[0]
    else:
        assert not line


def _check_files(stem, n_lineages):
    from literate_amd import ade
    with open(stem + "_ADE.tsv") as f:
        head, vals = [l.rstrip("\n").split("\t") for l in f]
    assert head == ade.FIT_HEAD and all("." not in vals[head.index(k)] for k in ade.FIT_INTS)
    with open(stem + "_ADE_shape.tsv") as f:
        rows = [l.rstrip("\n").split("\t") for l in f]
    assert rows[0] == ade.SHAPE_HEAD and [r[0] for r in rows[1:]] == ["coarse"] * ade.N_COARSE + ["fine"] * ade.N_FINE
    fit, shape = ade.read_tables(stem)
    say("fit row: %s" % fit)
    assert all(np.isfinite(fit[k]) for k in ade.FIT_HEAD) and np.isfinite(np.array([r[1:] for r in shape])).all()
    assert fit["draws"] == DRAWS and fit["draws_flagged"] == 0 and fit["lineages"] == n_lineages
    assert fit["lineages_used"] + fit["lineages_unused"] == n_lineages and fit["deaths"] + fit["censored"] == fit["lineages_used"]
    assert 0.0 <= fit["edge_mass"] <= 1.0 and 0.0 <= fit["p_shape_lt_1"] <= 1.0 and fit["deaths"] > 0
    assert 0.125 <= fit["shape_q025"] <= fit["shape_median"] <= fit["shape_q975"] <= 8.0 and fit["lr_mean"] >= 0.0
    assert fit["lr_hpd_low"] <= fit["lr_hpd_high"] and fit["const_lr"] >= 0.0
    for grid_name, n in (("coarse", ade.N_COARSE), ("fine", ade.N_FINE)):
        w = np.array([r[2] for r in shape if r[0] == grid_name])
        assert len(w) == n and abs(w.sum() - 1.0) <= 1e-12
    assert [r[1] for r in shape[:ade.N_COARSE]] == ade.coarse_shapes().tolist()


def _with_and_without(script, data, stem, extra, n_lineages):
    _run_cli(script, data, extra + OTHER)
    _check_files(stem, n_lineages)
    beside = {k: open(stem + k, "rb").read() for k in OTHER_FILES}
    for k in OTHER_FILES + ("_ADE.tsv", "_ADE_shape.tsv"):
        os.remove(stem + k)
    _run_cli(script, data, extra + OTHER, with_ade=False)
    assert not os.path.exists(stem + "_ADE.tsv") and not os.path.exists(stem + "_ADE_shape.tsv")
    for k in OTHER_FILES:
        same("%s beside --ade and without it" % k, beside[k], open(stem + k, "rb").read())


def case_cli_lrf():
    from helpers import waic_cases as W
    from literate_amd import logs
    with tempfile.TemporaryDirectory() as tmp:
        data = W._data(tmp)
        n = len(W._lrf_lineages(data)[0])
        stem = logs.log_paths(data, 2)[1]["div"][:-len("_div.log")]
        _with_and_without("LiteRateForward.py", data, stem, ["-model_BDI", "2"], n)


def case_cli_dd():
    from helpers import waic_cases as W
    from literate_amd.ddrate import model_suffix
    with tempfile.TemporaryDirectory() as tmp:
        data = W._data(tmp)
        n = len(W._dd_setup(data)[0])
        _with_and_without("DDRate.py", data, os.path.join(tmp, "example_31" + model_suffix(2, 2)), ["-m_birth", "2", "-m_death", "2"], n)


def case_cli_trend():
    from helpers import waic_cases as W
    from literate_amd.trendrate import model_suffix
    with tempfile.TemporaryDirectory() as tmp:
        data = W._data(tmp)
        n_bins = W._dd_setup(data)[3]
        n = len(W._dd_setup(data)[0])
        raw = 3.0 + np.sin(np.arange(n_bins + 1) / 4.0) + np.arange(n_bins + 1) / 10.0
        trend_file = os.path.join(tmp, "trend.tsv")
        with open(trend_file, "w") as f:
            f.write("year\tcovariate\n" + "".join("%d\t%r\n" % (i, float(v)) for i, v in enumerate(raw)))
        _with_and_without("trend_rate.py", data, os.path.join(tmp, "example_31" + model_suffix(False, False)) + "_1",
                          ["-trend_data", trend_file, "-trend_index", "1"], n)


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
