"""The case table of lr_ppc_age, shared by tests/test_ppc_age_host.py (the restatement against itself) and
tests/test_hip_ppc_age.py, whose GPU cases run here, each in a child process of its own (under the test's time limit):

    python tests/helpers/ppc_age_cases.py CASE [ARGS...]

A case prints its figures, asserts, and exits 0 - or raises.  The yardstick is tests/helpers/ppc_age_ref.py; every
comparison of counts is np.array_equal.  Every entry of TABLE must hold no fragile pair under the restatement (the host
test asserts it): only then is bit equality with the device the definition's own consequence.

Shapes: the smallest at which the kernel can go wrong.  A tile holds TILE = 1024 lineages (n = 1, TILE - 1, TILE, TILE + 1,
2 TILE + 1); a chunk of draws in LDS is min(64, 32768 // (24 n_bins + 8)) draws (n_bins 1: 64, so 65 draws are two chunks;
64: 21, so 23 draws are two; 682 | 683: two draws | one; 1365 | 1366: the last size of one draw within 32 KiB | above it;
2730 | 2731: 64 KiB of LDS | the raised LDS attribute; LR_MAX_BINS: 96 KiB); draws 1, 2, 3 and 65 over 4 forced slices
(17, 17, 17, 14)."""
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

from helpers import ppc_age_ref as ref  # noqa: E402

TILE = 1024
T0 = 5.0
LR_MAX_BINS = 4094


def say(*a):
    print(*a)
    sys.stdout.flush()


def chunk_of(n_bins, n_draws):
    """draws per LDS chunk of lr_age.hip, restated"""
    return max(1, min(64, 32768 // (24 * n_bins + 8), n_draws))


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def edge_lineages(n_bins):
    """(ts, te) of the hand-made lineages every case with room for them begins with"""
    tc = T0 + n_bins
    up = np.nextafter(tc, np.inf)
    rows = [(T0, T0 + 0.25),                      # born exactly at t0
            (T0, tc),                             # ... and dead exactly at T_c: te == T_c counts as dead
            (T0, up),                             # ... te just above T_c: censored
            (tc - 0.5, tc - 0.25),                # born in the last bin, dead in it
            (tc - 1.0, tc + 3.0),                 # born at the left edge of the last bin, censored
            (tc - 0.5, up),
            (tc, tc + 1.0),                       # ts >= T_c: unused
            (tc + 2.5, tc + 3.0),
            (T0 - 0.5, T0 + 2.0),                 # ts < t0: unused
            (np.nextafter(T0, -np.inf), T0 + 1.0),
            (T0 + 0.5, T0 + 0.5),                 # te <= ts: unused
            (T0 + 0.75, T0 + 0.25),
            (T0 + 0.5, np.nan),                   # NaN: unused
            (np.nan, T0 + 1.0),
            (T0 + 0.5, np.inf)]                   # never dies: censored
    a = np.array(rows)
    return a[:, 0], a[:, 1]


def lineages(rng, n, n_bins, kind):
    """n lineages around the window [T0, T0 + n_bins): year resolution (fs = 0, te = y + 0.5) or continuous times; some born
    before the window or after it; with room for them the edge lineages come first"""
    span = n_bins + 2.0
    ts = T0 - 1.0 + rng.random(n) * span
    life = rng.exponential(min(4.0, 0.5 * n_bins + 0.5), n)
    if kind == "year":
        ts = np.floor(ts)
        te = ts + np.floor(life) + 0.5
    else:
        te = ts + 0.001 + life
    if n == 1:
        ts[0], te[0] = (T0, T0 + 0.5) if kind == "year" else (T0 + 0.375, T0 + 0.875)
    es, ee = edge_lineages(n_bins)
    if n >= 2 * len(es):
        ts[:len(es)], te[:len(es)] = es, ee
    return ts, te


def rates(rng, S, n_bins, flags=True):
    """S draws of death rates: log-normal around 0.2, runs of zero bins in every other draw (in the first bins of some: a
    zero rate in the birth bin), and by position - when there are that many draws - an all-zero draw (1), 1e-300 throughout
    (3), 1e300 in one bin (5), and with `flags` the four kinds of flagged draw between good ones: NaN (2), negative (6),
    +inf (9), a sum that overflows (12; with one bin only: -0.0 is fine, so a second negative)"""
    mu = np.exp(rng.normal(size=(S, n_bins)) * 0.7 - 1.5)
    for s in range(0, S, 2):
        a = int(rng.integers(0, n_bins))
        mu[s, a:a + 1 + int(rng.integers(0, max(n_bins // 3, 1)))] = 0.0
        if s % 4 == 0:
            mu[s, :1 + n_bins // 8] = 0.0
    if S > 1:
        mu[1] = 0.0
    if S > 3:
        mu[3] = 1e-300
    if S > 5:
        mu[5, n_bins // 2] = 1e300
    if flags and S > 12:
        mu[2, n_bins // 3] = np.nan
        mu[6, n_bins - 1] = -0.125
        mu[9, 0] = np.inf
        if n_bins >= 2:
            mu[12, 0] = mu[12, n_bins - 1] = 1.5e308
        else:
            mu[12, 0] = -1e-300
    return mu


# name -> (n, draws, n_bins, kind, seed of the inputs, Philox seed, forced slices or None)
TABLE = {
    "n1": (1, 3, 7, "continuous", 101, 7, None),
    "n1_year": (1, 2, 7, "year", 102, 8, None),
    "tile_minus": (TILE - 1, 3, 7, "continuous", 103, 9, None),
    "tile": (TILE, 3, 7, "year", 104, 10, None),
    "tile_plus": (TILE + 1, 3, 7, "continuous", 105, 11, None),
    "two_tiles_plus": (2 * TILE + 1, 3, 7, "year", 106, (1 << 63) + 12345, None),
    "draws1": (300, 1, 12, "year", 111, 13, None),
    "draws2": (300, 2, 12, "continuous", 112, 14, None),
    "draws3": (300, 3, 12, "year", 113, 15, None),
    "draws65_slices4": (200, 65, 5, "continuous", 114, 16, 4),
    "bins1": (130, 65, 1, "continuous", 121, 17, None),
    "bins2": (700, 16, 2, "year", 122, 18, None),
    "bins64": (700, 23, 64, "continuous", 123, 19, None),
    "bins65": (700, 16, 65, "year", 124, 20, None),
    "bins682": (130, 3, 682, "continuous", 125, 21, None),
    "bins683": (130, 3, 683, "continuous", 126, 22, None),
    "bins1365": (130, 3, 1365, "year", 127, 23, None),
    "bins1366": (130, 3, 1366, "continuous", 128, 24, None),
    "bins2730": (130, 3, 2730, "continuous", 129, 25, None),
    "bins2731": (130, 3, 2731, "year", 130, 26, None),
    "bins_max": (700, 3, LR_MAX_BINS, "continuous", 131, 27, None),
}
GROUPS = {"lineages": ("n1", "n1_year", "tile_minus", "tile", "tile_plus", "two_tiles_plus"),
          "draws": ("draws1", "draws2", "draws3", "draws65_slices4"),
          "bins": ("bins1", "bins2", "bins64", "bins65"),
          "lds": ("bins682", "bins683", "bins1365", "bins1366", "bins2730", "bins2731", "bins_max")}
assert sorted(sum(GROUPS.values(), ())) == sorted(TABLE)


def inputs(name):
    """(ts, te, mu, Philox seed, forced slices) of a case"""
    n, S, nb, kind, seed_in, seed, slices = TABLE[name]
    rng = np.random.default_rng(seed_in)
    ts, te = lineages(rng, n, nb, kind)
    return ts, te, rates(rng, S, nb), seed, slices


_want = {}


def want(name):
    """the restatement of a case, computed once"""
    if name not in _want:
        ts, te, mu, seed, _ = inputs(name)
        _want[name] = ref.ppc_age(ts, te, T0, mu, seed)
    return _want[name]


# the distribution check: everybody born at t0 under one constant rate
DIST_N, DIST_S, DIST_BINS, DIST_MU, DIST_SEED = 4096, 64, 12, 0.3, 20260131


def dist_inputs():
    ts = np.full(DIST_N, T0)
    return ts, ts + 0.5, np.full((DIST_S, DIST_BINS), DIST_MU)


def check_distribution(rep):
    """rep [S, 2, A] of dist_inputs: the pooled count of every class with N S p_a >= 50, and of the survivors, within
    5 sqrt(N S p (1 - p)) + 1 of N S p: p_a = e^{-mu a} (1 - e^{-mu}) below the top class, e^{-mu (A - 1)} - e^{-mu A} in
    it (it is clamped, but everybody is censored at A), e^{-mu A} for the survivors"""
    A, mu, NS = DIST_BINS, DIST_MU, DIST_N * DIST_S
    rep = np.asarray(rep)
    assert rep.shape == (DIST_S, 2, A) and (rep >= 0).all() and (rep.sum(axis=(1, 2)) == DIST_N).all()
    dead, alive = rep[:, 0].sum(axis=0), rep[:, 1].sum(axis=0)
    assert alive[:A - 1].sum() == 0                                  # born at t0: every survivor is censored in the top class
    checked = 0
    for what, got, p in [("class %d" % a, dead[a], np.exp(-mu * a) - np.exp(-mu * (a + 1))) for a in range(A)] + \
                        [("survivors", alive[A - 1], np.exp(-mu * A))]:
        bound = 5.0 * np.sqrt(NS * p * (1.0 - p)) + 1.0
        say("   %s: %d, expected %.1f, bound %.1f" % (what, got, NS * p, bound))
        if NS * p >= 50:
            assert abs(got - NS * p) <= bound, (what, got, NS * p, bound)
            checked += 1
    assert checked == A + 1


# ------------------------------------------------------------------------------------------------
# the GPU cases
# ------------------------------------------------------------------------------------------------
def same(what, got, want_):
    ok = got == want_ if isinstance(got, (list, bytes)) else np.array_equal(np.asarray(got), np.asarray(want_))
    say("%s: %s" % (what, "identical" if ok else "DIFFER"))
    assert ok, (what, got, want_)


def device(ts, te, mu, seed, out=None):
    import torch
    from literate_amd import ops
    obs, rep, tot, plan = ops.ppc_age(torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda"), T0,
                                      torch.as_tensor(mu, device="cuda"), seed, out=out)
    return obs, rep, tot, plan


def case_against(group):
    """every case of the group against the restatement: the plan's slices (or the case's forced ones), then 1, 2 and the
    draw count; then a second call into the same outputs, dirtied"""
    import torch
    from literate_amd import ops
    for name in GROUPS[group]:
        ts, te, mu, seed, forced = inputs(name)
        w = want(name)
        S, nb = mu.shape
        first = None
        for sl in [forced, 1, 2, S]:
            if sl is None:
                os.environ.pop("LR_PPC_AGE_SLICES", None)
            else:
                os.environ["LR_PPC_AGE_SLICES"] = str(sl)
            obs, rep, tot, plan = device(ts, te, mu, seed)
            assert plan == ops.ppc_age_plan(len(ts), nb, S) and plan[0] == TILE and plan[3] == -(-len(ts) // TILE)
            assert plan[1] * (plan[2] - 1) < S <= plan[1] * plan[2]
            if sl is not None:
                dps = -(-S // min(sl, S))
                assert plan[1] == dps and plan[2] == -(-S // dps), plan
            label = "%s plan %s" % (name, plan)
            same(label + " obs", obs.cpu().numpy(), w["obs"])
            same(label + " rep", rep.cpu().numpy(), w["rep"])
            same(label + " totals", tot.cpu().numpy(), w["totals"])
            first = first or (obs, rep, tot)
        os.environ.pop("LR_PPC_AGE_SLICES", None)
        for t, fill in zip(first, (-7, 1 << 40, 3)):
            t.fill_(fill)
        obs, rep, tot, _ = device(ts, te, mu, seed, out=first)
        assert obs.data_ptr() == first[0].data_ptr() and rep.data_ptr() == first[1].data_ptr()
        same(name + " dirty outputs, second call", [obs.cpu().numpy().tolist(), rep.cpu().numpy().tolist(), tot.cpu().numpy().tolist()],
             [w["obs"].tolist(), w["rep"].tolist(), w["totals"].tolist()])
        torch.cuda.synchronize()


def case_flags():
    """a flagged draw is -1 throughout and leaves the rows of the other draws what they are without it"""
    rng = np.random.default_rng(141)
    n, S, nb = 1500, 9, 20
    ts, te = lineages(rng, n, nb, "continuous")
    good = rates(rng, S, nb, flags=False)
    base = device(ts, te, good, 31)
    base_rep = base[1].cpu().numpy()
    same("no flag: rep", base_rep, ref.ppc_age(ts, te, T0, good, 31)["rep"])
    assert (base_rep >= 0).all() and base[2].cpu().numpy().tolist() == [int(ref.lineage_terms(ts, te, T0, nb)[0].sum()),
                                                                        n - int(ref.lineage_terms(ts, te, T0, nb)[0].sum()), S, 0]
    for s, (b, v) in zip((0, 4, 7, 8), ((3, np.nan), (0, -1e-300), (nb - 1, np.inf), (5, -np.inf))):
        mu = good.copy()
        mu[s, b] = v
        obs, rep, tot, _ = device(ts, te, mu, 31)
        rep = rep.cpu().numpy()
        assert (rep[s] == -1).all()
        same("draw %d flagged (%r): the other draws' rows" % (s, v), np.delete(rep, s, axis=0), np.delete(base_rep, s, axis=0))
        same("   obs", obs.cpu().numpy(), base[0].cpu().numpy())
        assert tot.cpu().numpy().tolist()[2:] == [S - 1, 1]
    mu = good.copy()
    mu[2, 1] = mu[2, 7] = 1.2e308                   # finite rates, a sum that overflows
    mu[:2] = np.nan
    rep = device(ts, te, mu, 31)[1].cpu().numpy()
    assert (rep[:3] == -1).all()
    same("three flagged draws: the other rows", rep[3:], base_rep[3:])


def case_arguments():
    """every refusal returns its code, in the documented order, and leaves the outputs untouched"""
    import torch
    from literate_amd import _hip, ops
    lib = _hip.load()
    n, nb, S = 10, 20, 8
    ts = torch.rand(n, dtype=torch.float64, device="cuda") + T0
    te = ts + 1.0
    mu = torch.rand(S, nb, dtype=torch.float64, device="cuda") + 0.1
    obs = torch.full((2, nb), 123, dtype=torch.int64, device="cuda")
    rep = torch.full((S, 2, nb), 123, dtype=torch.int64, device="cuda")
    tot = torch.full((4,), 123, dtype=torch.int64, device="cuda")
    need = lib.lr_ppc_age_workspace_bytes(n, nb, S)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    P = _hip.ptr

    def call(**kw):
        a = dict(ts=P(ts), te=P(te), n=n, t0=T0, nb=nb, mu=P(mu), S=S, obs=P(obs), rep=P(rep), tot=P(tot), ws=P(ws), wsb=need)
        a.update(kw)
        return _hip.launch(lib.lr_ppc_age, ts.device, a["ts"], a["te"], a["n"], a["t0"], a["nb"], a["mu"], a["S"], 5, a["obs"],
                           a["rep"], a["tot"], a["ws"], a["wsb"])

    E = _hip
    for kw, code in ((dict(ts=None), E.LR_ERR_NULL), (dict(te=None), E.LR_ERR_NULL), (dict(mu=None), E.LR_ERR_NULL),
                     (dict(obs=None), E.LR_ERR_NULL), (dict(rep=None), E.LR_ERR_NULL), (dict(tot=None), E.LR_ERR_NULL),
                     (dict(ws=None), E.LR_ERR_NULL), (dict(n=0), E.LR_ERR_SIZE), (dict(n=-3), E.LR_ERR_SIZE),
                     (dict(S=0), E.LR_ERR_SIZE), (dict(S=-1), E.LR_ERR_SIZE), (dict(nb=0), E.LR_ERR_SIZE),
                     (dict(nb=E.LR_MAX_BINS + 1), E.LR_ERR_SIZE), (dict(n=1 << 59), E.LR_ERR_SIZE),
                     (dict(t0=T0 + 0.5), E.LR_ERR_T0), (dict(t0=float("nan")), E.LR_ERR_T0),
                     (dict(wsb=need - 1), E.LR_ERR_WORKSPACE), (dict(wsb=0), E.LR_ERR_WORKSPACE),
                     # the order: NULL before SIZE before T0 before WORKSPACE
                     (dict(ts=None, n=0, t0=0.5, wsb=0), E.LR_ERR_NULL), (dict(n=0, t0=0.5, wsb=0), E.LR_ERR_SIZE),
                     (dict(t0=0.5, wsb=0), E.LR_ERR_T0)):
        rc = call(**kw)
        say("%s -> %d" % (sorted(kw), rc))
        assert rc == code, (kw, rc, code)
    # n n_draws >= 2^62 is refused, one below is a matter of the workspace only
    assert lib.lr_ppc_age_workspace_bytes(1 << 59, nb, 8) == E.LR_ERR_SIZE
    assert lib.lr_ppc_age_workspace_bytes((1 << 59) - 1, nb, 8) == need
    assert lib.lr_ppc_age_workspace_bytes(n, nb, 0) == E.LR_ERR_SIZE and lib.lr_ppc_age_workspace_bytes(n, 0, S) == E.LR_ERR_SIZE
    import ctypes as C
    assert lib.lr_ppc_age_plan(n, nb, S, None) == E.LR_ERR_NULL
    assert lib.lr_ppc_age_plan(0, nb, S, (C.c_int32 * 4)()) == E.LR_ERR_SIZE
    torch.cuda.synchronize()
    assert bool((obs == 123).all()) and bool((rep == 123).all()) and bool((tot == 123).all())       # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert tot.cpu().numpy().tolist() == [n, 0, S, 0] and int(obs.sum()) == n and bool((rep.sum(dim=(1, 2)) == n).all())
    for bad, code in ((dict(t0=T0 + 0.25), "LR_ERR_T0"),):
        try:
            ops.ppc_age(ts, te, bad["t0"], mu, 5)
        except ValueError as ex:
            assert code in str(ex) and str(ex).startswith("lr_ppc_age:")
        else:
            raise AssertionError(bad)
    try:
        ops.ppc_age(ts, te, T0, mu[:0], 5)
    except ValueError as ex:
        assert "LR_ERR_SIZE" in str(ex)
    else:
        raise AssertionError("no draws")


def case_distribution():
    """the distribution check of the host test on the device's counts"""
    ts, te, mu = dist_inputs()
    obs, rep, tot, plan = device(ts, te, mu, DIST_SEED)
    say("plan", plan)
    check_distribution(rep.cpu().numpy())
    assert tot.cpu().numpy().tolist() == [DIST_N, 0, DIST_S, 0] and int(obs[0, 0]) == DIST_N


def case_contract():
    """the buffer contract of include/literate_hip.h (helpers.abi_cases.contract / refuses) for lr_ppc_age at the tile-edge
    and slice-edge shapes: workspace and outputs of exactly the queried and documented size, fills 0x00 and 0xFF, guards
    intact, a second call on the dirty buffers, a workspace one byte short, one argument error"""
    import torch
    from literate_amd import _hip, ops
    from helpers.abi_cases import contract, refuses
    lib = _hip.load()
    rng = np.random.default_rng(151)

    def caller(ts_d, te_d, mu_d, t0=T0):
        return lambda: ops.ppc_age(ts_d, te_d, t0, mu_d, 77)[:3]

    S, nb = 6, 9
    mu = rates(rng, S, nb)
    mu_d = torch.as_tensor(mu, device="cuda")
    for n in (1, TILE - 1, TILE, TILE + 1):
        ts, te = lineages(rng, n, nb, "continuous")
        ts_d, te_d = torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda")
        w = ref.ppc_age(ts, te, T0, mu, 77)
        for sl in ("1", "4", "6"):                    # 6, 2 + 2 + 2 and six single draws
            os.environ["LR_PPC_AGE_SLICES"] = sl
            plan = ops.ppc_age_plan(n, nb, S)
            assert plan[2] == (3 if sl == "4" else int(sl)) and plan[3] == -(-n // TILE), plan
            assert lib.lr_ppc_age_workspace_bytes(n, nb, S) > 0
            label = "ppc_age n %d plan %s" % (n, plan)
            obs, rep, tot = contract(ops, torch, caller(ts_d, te_d, mu_d), label=label)
            same(label, [obs.cpu().numpy().tolist(), rep.cpu().numpy().tolist(), tot.cpu().numpy().tolist()],
                 [w["obs"].tolist(), w["rep"].tolist(), w["totals"].tolist()])
            refuses(ops, torch, caller(ts_d, te_d, mu_d), "LR_ERR_WORKSPACE", short=1, label=label, entry="lr_ppc_age")
    refuses(ops, torch, caller(ts_d, te_d, mu_d, T0 + 0.5), "LR_ERR_T0", label="ppc_age t0", entry="lr_ppc_age")
    # the largest table (a draw takes 96 KiB of LDS), two tiles
    os.environ.pop("LR_PPC_AGE_SLICES")
    ts, te = lineages(rng, TILE + 1, LR_MAX_BINS, "year")
    big = caller(torch.as_tensor(ts, device="cuda"), torch.as_tensor(te, device="cuda"),
                 torch.as_tensor(rates(rng, 3, LR_MAX_BINS), device="cuda"))
    contract(ops, torch, big, label="ppc_age %d bins" % LR_MAX_BINS)
    refuses(ops, torch, big, "LR_ERR_WORKSPACE", short=1, label="ppc_age %d bins" % LR_MAX_BINS, entry="lr_ppc_age")


# ------------------------------------------------------------------------------------------------
# the command lines
# ------------------------------------------------------------------------------------------------
OTHER = ["--ppc", "0.2", "--ppc_draws", "20", "--ppc_scale", "10", "--waic", "0.2", "--waic_draws", "32", "--loo", "0.2",
         "--loo_draws", "32"]
OTHER_FILES = ("_PPC.tsv", "_PPC_fit.tsv", "_WAIC.tsv", "_WAIC_pointwise.npz", "_LOO.tsv", "_LOO_pointwise.npz")


def _run_cli(script, data, extra, age=True):
    from helpers import waic_cases as W
    cmd = [sys.executable, os.path.join(ROOT, script), "-d", data, "-TBP", "-n", str(W.N_IT), "-s", str(W.S_FREQ), "-p", "1000",
           "-seed", "31", "--chains", str(W.CH)] + (["--ppc_age", "0.2", "--ppc_age_draws", str(W.DRAWS)] if age else []) + extra
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LR_PPC_AGE_SLICES", "LR_WAIC_SLICES"):
        env.pop(k, None)
    out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=280, env=env).stdout
    line = [l for l in out.splitlines() if l.startswith("PPC age:")]
    say(line)
    if age:
        assert len(line) == 1 and "_PPC_age.tsv" in line[0] and "_PPC_age_fit.tsv" in line[0] and "%d draws" % W.DRAWS in line[0]
    else:
        assert not line


def _read_tsv(path):
    with open(path) as f:
        rows = [l.rstrip("\n").split("\t") for l in f]
    return rows[0], rows[1:]


def _check_files(stem, ts, te, t0, mu, seed):
    """<stem>_PPC_age.tsv and _PPC_age_fit.tsv against the restatement's counts and summary on the rates of the logs, the
    lineages in the engine's order.  Everything is compared with ==: counts, observed values, HPD ends (picks of the same
    doubles), p_ge, and the means - the restatement adds a column in lr_col_summary's own order (ppc_age_ref.device_mean), so
    the means of the ratio statistics (hazard, mean class at death) have the device's bits too."""
    from helpers import waic_cases as W
    from literate_amd import ppc_age
    o = W._engine_order(ts, te)
    ts, te = ts[o], te[o]
    w = ref.ppc_age(ts, te, t0, mu, seed)
    frag = ref.fragile(ts, te, t0, mu, seed, base=w)
    say("%s: %d lineages (%d used), %d draws, %d bins, %d fragile pairs" % (os.path.basename(stem), len(ts), w["totals"][0],
                                                                            mu.shape[0], mu.shape[1], len(frag)))
    assert len(frag) == 0 and w["totals"][3] == 0
    sm = ref.summary(w["obs"], w["rep"])
    A = mu.shape[1]
    head, rows = _read_tsv(stem + "_PPC_age.tsv")
    assert head == ppc_age.AGE_HEAD and len(rows) == A
    assert all("." not in r[0] and "." not in r[1] for r in rows)
    got = np.array([[float(v) for v in r] for r in rows])
    same("age, at_risk_obs", got[:, :2], np.stack([np.arange(A), sm["at_risk_obs"]], axis=1))

    def stats(what, g, wnt):
        g, wnt = np.asarray(g, float), np.asarray(wnt, float)
        for c in range(5):
            assert np.array_equal(g[:, c], wnt[:, c], equal_nan=True), (what, ppc_age.STATS[c], g[:, c], wnt[:, c])
        say("%s: obs, mean, HPD ends, p_ge identical" % what)
    stats("deaths", got[:, 2:7], sm["deaths"])
    stats("hazard", got[:, 7:12], sm["hazard"])
    assert np.isfinite(got[0, 7:12]).all() and got[:, 2].sum() == w["obs"][0].sum() > 0
    head, rows = _read_tsv(stem + "_PPC_age_fit.tsv")
    assert head == ppc_age.FIT_HEAD and len(rows) == 1
    fit = dict(zip(head, rows[0]))
    ints = ppc_age.FIT_INTS + ["hazard_classes_extreme"]
    assert all("." not in fit[k] for k in ints)
    assert [int(fit[k]) for k in ints] == [mu.shape[0], 0, len(ts), int(w["totals"][0]), int(w["totals"][1]), A,
                                           sm["hazard_classes_extreme"]]
    for k, name in enumerate(ppc_age.FIT_STATS):
        stats(name, [[float(fit["%s_%s" % (name, s)]) for s in ppc_age.STATS]], sm["overall"][k:k + 1])
    for k in ("coverage_deaths", "coverage_hazard"):
        assert float(fit[k]) == sm[k], (k, fit[k], sm[k])
    say("fit row: %s" % fit)


def case_cli_lrf():
    """LiteRateForward.py --ppc_age against the restatement fed the death rates of the logs the same run wrote; then the
    same run with --ppc --waic --loo, once beside --ppc_age and once without it: the other flags' files byte for byte"""
    from helpers import waic_cases as W
    from literate_amd import logs
    model = 2
    with tempfile.TemporaryDirectory() as tmp:
        data = W._data(tmp)
        _run_cli("LiteRateForward.py", data, ["-model_BDI", str(model)])
        stem = logs.log_paths(data, model)[1]["div"][:-len("_div.log")]
        ts, te = W._lrf_lineages(data)
        t0, n_bins = float(int(ts.min())), int(te.max()) - int(ts.min())
        per_chain = []
        for c in range(W.CH):
            paths = logs.log_paths(data, model, chain=c)[1]
            mc = np.loadtxt(paths["mcmc"], skiprows=1)
            ex_rows = [np.array(l.split(), float) for l in open(paths["ex_rates"])]
            per_chain.append([logs.rates_per_bin(b[:(len(b) + 1) // 2], b[(len(b) + 1) // 2:], m[8], n_bins)
                              for m, b in zip(mc, ex_rows)])
        mu = np.array(W._draw_rows(per_chain))
        _check_files(stem, ts, te, t0, mu, 31)
        age = {k: open(stem + k, "rb").read() for k in ("_PPC_age.tsv", "_PPC_age_fit.tsv")}
        _run_cli("LiteRateForward.py", data, ["-model_BDI", str(model)] + OTHER)
        beside = {k: open(stem + k, "rb").read() for k in OTHER_FILES}
        assert {k: open(stem + k, "rb").read() for k in age} == age              # and --ppc_age's own do not depend on them
        for k in list(age) + list(OTHER_FILES):
            os.remove(stem + k)
        _run_cli("LiteRateForward.py", data, ["-model_BDI", str(model)] + OTHER, age=False)
        assert not os.path.exists(stem + "_PPC_age.tsv")
        for k in OTHER_FILES:
            same("%s beside --ppc_age and without it" % k, beside[k], open(stem + k, "rb").read())


def _dd_mu(paths, n_bins, first_col):
    """the m_i columns of the drawn log rows (the logs hold the shortest round-trip digits of what draw_rates recomputes)"""
    from helpers import waic_cases as W
    rows = np.array(W._log_rows(paths))
    return rows[:, first_col + n_bins:first_col + 2 * n_bins].copy()


def case_cli_dd():
    """DDRate.py --ppc_age against the restatement on the death rates its logs hold"""
    from helpers import waic_cases as W
    from literate_amd.ddrate import model_suffix
    with tempfile.TemporaryDirectory() as tmp:
        data = W._data(tmp)
        ts, te, origin, n_bins, DT = W._dd_setup(data)
        _run_cli("DDRate.py", data, ["-m_birth", "2", "-m_death", "2"])
        stem = os.path.join(tmp, "example_31" + model_suffix(2, 2))
        mu = _dd_mu(["%s_c%d.log" % (stem, c) for c in range(W.CH)], n_bins, 14)
        _check_files(stem, ts, te, origin, mu, 31)


def case_cli_trend():
    """trend_rate.py --ppc_age with a synthetic covariate against the restatement on the death rates its logs hold"""
    from helpers import waic_cases as W
    from literate_amd.trendrate import model_suffix
    with tempfile.TemporaryDirectory() as tmp:
        data = W._data(tmp)
        ts, te, origin, n_bins, DT = W._dd_setup(data)
        raw = 3.0 + np.sin(np.arange(n_bins + 1) / 4.0) + np.arange(n_bins + 1) / 10.0
        trend_file = os.path.join(tmp, "trend.tsv")
        with open(trend_file, "w") as f:
            f.write("year\tcovariate\n" + "".join("%d\t%r\n" % (i, float(v)) for i, v in enumerate(raw)))
        _run_cli("trend_rate.py", data, ["-trend_data", trend_file, "-trend_index", "1"])
        stem = os.path.join(tmp, "example_31" + model_suffix(False, False))
        mu = _dd_mu(["%s_c%d_1.trendrate.log" % (stem, c) for c in range(W.CH)], n_bins, 12)
        _check_files(stem + "_1", ts, te, origin, mu, 31)


CASES = {k[5:]: v for k, v in list(globals().items()) if k.startswith("case_")}

if __name__ == "__main__":
    CASES[sys.argv[1]](*sys.argv[2:])
    print("case %s ok" % " ".join(sys.argv[1:]))
