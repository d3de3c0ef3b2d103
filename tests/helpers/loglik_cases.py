"""The value matrix of lr_bd_loglik_batch: one case (at least) per kernel the entry point can launch, each compared with
tests/helpers/loglik_ref.py under its derived bound (tests/test_hip_loglik_matrix.py runs a family per child process,
because LR_LOGLIK_SMALL and LR_SCAN_WIDE are read once per process; tests/test_loglik_matrix_host.py proves on the CPU that
the cases mean what they claim):

    python tests/helpers/loglik_cases.py FAMILY        (A B C D E F)

    A  every tiled kernel, every applicable model, both sides of every table-class edge         LR_LOGLIK_SMALL=0
    B  chain counts per kernel family: full, ragged, 8 groups (the XCD remap), 9, 16; each chain also alone    "
    C  the last tile's length around 1, 2, 2T and (wide) 4T, 6T; ts / te aligned and 8 bytes off                "
    D  the birth-bin cache: sorted runs placed by the lineage-to-wave map, shuffled, one lineage moved           "
    E  the one-launch kernel and its three boundaries; ops.LoglikSession zero-copy               (nothing set)
    F  lr_scan_fast_kernel<8, H> at 8 and 9 chain groups                       LR_LOGLIK_SMALL=0 LR_SCAN_WIDE=0

plan() restates lr_plan_scan(unit_res = 0, wide = 1) and small() the lr_loglik_small predicate of csrc/lr_loglik.hip; every
case names the kernel it is meant to reach and the restatement must agree (here, and with lr_bd_loglik_plan)."""
import ctypes as CT
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import loglik_ref as R  # noqa: E402

FAMILY_ENV = {"A": {"LR_LOGLIK_SMALL": "0"}, "B": {"LR_LOGLIK_SMALL": "0"}, "C": {"LR_LOGLIK_SMALL": "0"},
              "D": {"LR_LOGLIK_SMALL": "0"}, "E": {}, "F": {"LR_LOGLIK_SMALL": "0", "LR_SCAN_WIDE": "0"}}

# ------------------------------------------------------------------------------------------------
# the launch plan, restated (csrc/lr_loglik.hip, csrc/lr_internal.h)
# ------------------------------------------------------------------------------------------------
LR_MAX_BINS = 4094
MODEL3_MAX_BINS = 2398           # LR_SCAN_LDS_MAX / (2 classes x 2 sides x 16 bytes) - 2
SCAN_T, WIDE_T, SMALL_T = 256, 512, 1024
LDS_BUDGET, LDS_MAX, LDS_WIDE = 48 * 1024, 150 * 1024, 72 * 1024
FAST_H = (40, 72, 136, 264)
ERR_SIZE = -2

Plan = namedtuple("Plan", "H fast n_cls cb threads groups tiles chunk")


def bins_per_lane(H):
    return 1 if H <= 40 else (2 if H <= 136 else (4 if H <= 264 else 8))


def plan(n, C, n_bins, model, wide_env=True):
    """-> Plan, or ERR_SIZE"""
    if n < 1 or C < 1 or n_bins < 1 or n_bins > LR_MAX_BINS:
        return ERR_SIZE
    n_cls = 2 if model == 3 else 1
    H, fast = n_bins + 2, 0
    if n_cls == 1:
        for h in FAST_H:
            if n_bins + 2 <= h and n_bins <= 64 * bins_per_lane(h):
                H, fast = h, 1
                break
    per_chain = n_cls * 2 * H * 16
    cb = 8
    while cb > 1 and per_chain * cb > LDS_BUDGET:
        cb >>= 1
    if wide_env and fast and C > 8 and per_chain * 16 <= LDS_WIDE:
        cb = 16
    if per_chain * cb > LDS_MAX:
        return ERR_SIZE
    while cb > 1 and cb // 2 >= C:
        cb >>= 1
    threads = WIDE_T if cb == 16 else SCAN_T
    groups = -(-C // cb)
    unit = 2 * threads
    tiles = -(-1024 // groups)
    if threads == WIDE_T and tiles < 256:
        tiles = 256
    tiles = max(1, min(tiles, -(-n // (4 * unit))))
    chunk = -(-(-(-n // tiles)) // unit) * unit
    return Plan(H, fast, n_cls, cb, threads, groups, -(-n // chunk), chunk)


def small(n, C, n_bins, model, small_env=True):
    """the one-launch kernel takes the call: few states on few lineages, and both table classes within 60 KiB of LDS"""
    return bool(small_env and n <= (1 << 18) and C <= 64 and n * C <= (1 << 21)
                and (2 if model == 3 else 1) * 2 * (n_bins + 2) * 16 <= 60 * 1024)


def kernel(n, C, n_bins, model, env):
    """the kernel the call launches under a family's environment, by the restatement"""
    if small(n, C, n_bins, model, env.get("LR_LOGLIK_SMALL") != "0"):
        return "small"
    p = plan(n, C, n_bins, model, env.get("LR_SCAN_WIDE") != "0")
    if p == ERR_SIZE:
        return "LR_ERR_SIZE"
    if p.fast:
        return "wide<%d>" % p.H if p.cb == 16 else "fast<%d,%d>" % (p.cb, p.H)
    return "generic<%d>x%d" % (p.cb, p.n_cls)


def depth(n, C, n_bins, model, env):
    """additions on the longest path from a term to out[c]"""
    if kernel(n, C, n_bins, model, env) == "small":
        return -(-n // SMALL_T) + 7 + SMALL_T // 64 + 1       # per thread, the wave's scan, the 16 waves, + constant
    p = plan(n, C, n_bins, model, env.get("LR_SCAN_WIDE") != "0")
    per_thread = -(-min(p.chunk, n) // p.threads)
    per_thread += per_thread & 1                              # a thread scores whole pairs
    block = (p.cb + p.threads // p.cb) if p.fast else (7 + SCAN_T // 64)
    return per_thread + block + (8 + 16 + 16) + 1             # lr_reduce_partials_kernel, + constant


def last_tile(n, p):
    return n - (p.tiles - 1) * p.chunk


def find_n(r, C, n_bins, model, env, min_tiles=2):
    """the smallest n whose plan has >= min_tiles tiles, the last of r lineages"""
    wide_env = env.get("LR_SCAN_WIDE") != "0"
    unit = 2 * plan(10 ** 5, C, n_bins, model, wide_env).threads
    for m in range(1, 200):
        n = m * unit + r
        p = plan(n, C, n_bins, model, wide_env)
        if p.tiles >= min_tiles and last_tile(n, p) == r:
            return n
    raise AssertionError("no n with a last tile of %d" % r)


# ------------------------------------------------------------------------------------------------
# lineages and rates
# ------------------------------------------------------------------------------------------------
def edge_block(t0, W, end_time=None):
    """[(ts, te)]: the fixed head of every lineage set.  The first three are plain in-window lineages (n = 1, 2, 3 take them)."""
    t0, W = float(t0), int(W)
    rows = [(t0 + 1, t0 + 1.5),                      # ts on a bin edge
            (t0 + 0.5, t0 + 2),                      # te on a bin edge: the bin it closes
            (t0 + 2.25, t0 + 2.25),                  # ts == te inside a bin
            (t0 + 2, t0 + 2),                        # ts == te on an edge
            (t0 - 1.5, t0 + 0.5), (t0, t0 + 0.75), (t0 + W, t0 + W + 0.5),              # ts < t0, == t0, == t0 + n_bins
            (t0 - 2, t0), (t0 + W - 0.5, t0 + W), (t0 + 1.5, t0 + W + 3.25),            # te == t0, == t0 + n_bins, beyond
            (t0 - 5, t0 - 3.5), (t0 + W + 1, t0 + W + 2.5), (t0 - 1.25, t0 + W + 1.25),  # before, after, spanning
            (-1e18, t0 + 1.5), (t0 + 1.5, 1e18), (-1e300, 1e300), (-1e300, -1e18), (1e18, 1e300)]
    if end_time is not None:
        e = float(end_time)
        rows += [(e - 2.5, e), (e - 2.5, float(np.nextafter(e, -np.inf))), (e - 2.5, e + 0.75)]
    return rows


N_EDGE2, N_EDGE3 = len(edge_block(0, 40)), len(edge_block(0, 40, 20.0))
NO_DEATH_BIN, ZERO_BIRTH_BIN, NAN_BIN, ZERO_BR_BIN = 5, 2, 7, 1       # of the special rate set


class Case:
    """family, name, kernel: the kernel it is meant to reach.  end: None (model 3: t0 + round(0.6 W)), or one of 'frac',
    'before', 'beyond'.  special: the rate set with zeros and a nan.  layout: None, or ('runs' | 'shuffled' | 'moved') of
    family D.  offset: ts / te 8 bytes off 16-byte alignment.  pair: name of the case whose shared chains must agree.
    masked_last_bin (models 0 / 1): lineages and rates of the window one bin shorter, and a last bin with br_length 0 - it
    scores nothing, so the case computes the number of the shorter window on the other side of a bin-count boundary."""

    def __init__(self, family, name, kern, n, C, n_bins, model, t0=3, seed=0, end=None, special=False, layout=None,
                 offset=False, alone=False, pair=None, session=0, extra_before=0, masked_last_bin=False):
        self.family, self.name, self.kernel, self.n, self.C, self.n_bins, self.model = family, name, kern, n, C, n_bins, model
        self.t0, self.seed, self.end, self.special, self.layout, self.offset = t0, seed, end, special, layout, offset
        self.alone, self.pair, self.session, self.extra_before, self.masked_last_bin = alone, pair, session, extra_before, masked_last_bin
        self.env = FAMILY_ENV[family]
        self._data = None

    @property
    def end_time(self):
        if self.model != 3:
            return 0.0
        W, t0 = self.n_bins, float(self.t0)
        return {None: t0 + round(0.6 * W), "frac": t0 + round(0.6 * W) + 0.37, "before": t0 - 60.0, "beyond": t0 + W + 7.5}[self.end]

    def reached(self):
        return kernel(self.n, self.C, self.n_bins, self.model, self.env)

    def depth(self):
        return depth(self.n, self.C, self.n_bins, self.model, self.env)

    def data(self):
        if self._data is None:
            self._data = make_data(self)
        return self._data

    def reference(self):
        """(want [C] longdouble, tol [C], L, A)"""
        d = self.data()
        want, L, A = R.loglik(d["ts"], d["te"], self.t0, d["lam"], d["mu"], self.model, d["br"], self.end_time)
        cst = R.constant(d["lam"], self.model, d["br"]) if self.model == 1 else None
        return want, R.tolerance(L, A, self.depth(), self.n_bins, cst), L, A


def run_bins(c):
    """family D: the birth bin of every lineage - a run born before the window, runs in ascending bins whose lengths cycle
    through {300, 1, 64, 127, 128, 129} with a run of 300 between them, a run born after the window; then one unsorted
    lineage inside the window (a dropped last lineage must show)"""
    W, lens, out, b, j, n = c.n_bins, (1, 64, 127, 128, 129, 300), [np.full(300, -1)], 0, 0, c.n - 1
    while b < W and sum(len(x) for x in out) < n - 300:
        for ln in (300, lens[j % 6]):
            if b >= W:
                break
            out.append(np.full(ln, b))
            b += 1
        j += 1
    bins = np.concatenate(out)[:n - 300]
    return np.concatenate((bins, np.full(c.n - len(bins), W)))      # (the last of them becomes an in-window lineage)


def make_data(c):
    rng = np.random.default_rng(1000 + c.seed)
    t0, W, n, model = float(c.t0), c.n_bins - c.masked_last_bin, c.n, c.model
    e_t = c.end_time
    edge = np.array(edge_block(t0, W, e_t if model == 3 else None))
    k = max(n - c.extra_before - len(edge), 0)
    if c.layout:
        bins = run_bins(c)
        ts = t0 + bins + rng.uniform(0.0, 1.0, n)
        ts = np.sort(np.minimum(ts, t0 + bins + 0.999))      # (the bins ascend: sorting keeps every lineage in its run)
        te = ts + rng.exponential(W / 4.0, n)
        ts[-1], te[-1] = t0 + 3.3, t0 + 0.5 * W + 0.4
        if c.layout == "moved":
            i = moved_lineage(c)
            ts[i] += 1.0
            te[i] += 1.0
        if c.layout == "shuffled":
            p = np.concatenate((rng.permutation(n - 1), [n - 1]))
            ts, te = ts[p], te[p]
    else:
        ts = rng.uniform(t0 - 2.0, t0 + W + 1.0, k)
        far = rng.uniform(size=k) < 0.03
        ts[far] -= 40.0
        te = ts + rng.exponential(W / 4.0, k)
        if model == 3 and c.end is None or c.end == "frac":
            at = (rng.uniform(size=k) < 0.2) & (ts < e_t)            # the extant lineages of real data: te == end_time
            te[at] = e_t
        if c.end == "beyond":                                    # nobody but the far-away lineages of the edge block is extant
            te = np.minimum(te, np.maximum(ts, t0 + W + 7.0))
        if c.special:
            dying = (te > t0 + NO_DEATH_BIN) & (te <= t0 + NO_DEATH_BIN + 1)
            te[dying] += 1.0
        # (lineages wholly before the window, behind the edge block: every term is 0 - the larger case of a pair)
        xs, xe = np.full(c.extra_before, t0 - 9.0), np.full(c.extra_before, t0 - 8.5)
        ts, te = np.concatenate((edge[:, 0], xs, ts))[:n], np.concatenate((edge[:, 1], xe, te))[:n]
        if n > len(edge):                                          # the last lineage of the last tile counts: in the window
            ts[-1], te[-1] = t0 + 3.3, t0 + 0.5 * W + 0.4
    assert len(ts) == n and np.all(te >= ts)
    rr = np.random.default_rng(77 + c.seed // 1000)                  # (the cases of a pair share their rates)
    Cmax = max(c.C, 65) if c.pair or c.family == "E" else c.C
    lam = np.exp(rr.uniform(np.log(.05), np.log(.6), (Cmax, W)))[:c.C]
    mu = np.exp(rr.uniform(np.log(.02), np.log(.3), (Cmax, W)))[:c.C]
    br = None
    if model < 2:
        br = R.unit_stats(ts, te, t0, c.n_bins)[2]
    if c.masked_last_bin:
        lam, mu = np.concatenate((lam, np.full((c.C, 1), .3)), axis=1), np.concatenate((mu, np.full((c.C, 1), .1)), axis=1)
        br[-1] = 0.0
    if c.special:
        assert c.C >= 4
        mu[0, NO_DEATH_BIN] = 0.0          # nobody dies there: finite
        lam[1, ZERO_BIRTH_BIN] = 0.0       # someone is born there: -inf
        mu[2, NAN_BIN] = np.nan
        if model < 2:
            br[ZERO_BR_BIN] = 0.0          # holds events: the k > 0 mask drops them
    return dict(ts=ts, te=te, lam=lam, mu=mu, br=br)


# ---- family D's lineage-to-wave map -------------------------------------------------------------
def trips(c, ts=None):
    """[(tile, wave, trip, uniform, bin)] in the order a wave runs them: wave w of a tile scores the pairs of lineages
    start + 2 T k + 128 w .. + 127 at trip k (the aligned loop: whole pairs only; a trailing odd lineage is scored alone)."""
    p = plan(c.n, c.C, c.n_bins, c.model, c.env.get("LR_SCAN_WIDE") != "0")
    ts = c.data()["ts"] if ts is None else ts
    a = np.clip(np.floor(ts) - c.t0, -1, c.n_bins).astype(np.int64)
    out = []
    for tile in range(p.tiles):
        start, end = tile * p.chunk, min((tile + 1) * p.chunk, c.n)
        for w in range(p.threads // 64):
            k = 0
            while True:
                lo_ = start + 2 * p.threads * k + 128 * w
                hi_ = min(lo_ + 128, end - ((end - lo_) & 1))
                if hi_ <= lo_:
                    break
                out.append((tile, w, k, bool(np.all(a[lo_:hi_] == a[lo_])), int(a[lo_])))
                k += 1
    return out


def trip_census(tr, n_bins):
    uni = [t for t in tr if t[3]]
    switches = consecutive = 0
    last = {}
    for t in tr:
        key = t[:2]
        if t[3]:
            if key in last and last[key][1] != t[4]:
                switches += 1
                consecutive += last[key][0] == t[2] - 1
            last[key] = (t[2], t[4])
    return dict(uniform=len(uni), nonuniform=len(tr) - len(uni), before=sum(t[4] == -1 for t in uni),
                after=sum(t[4] == n_bins for t in uni),
                switches=switches, consecutive=consecutive)


def moved_lineage(c):
    """a lineage in the middle of a uniform trip of the sorted layout, inside the window"""
    base = Case(c.family, "", c.kernel, c.n, c.C, c.n_bins, c.model, c.t0, c.seed, layout="runs")
    p = plan(c.n, c.C, c.n_bins, c.model)
    for tile, w, k, u, b in trips(base):
        if u and 0 <= b < c.n_bins - 1 and k >= 1:
            return tile * p.chunk + 2 * p.threads * k + 128 * w + 64
    raise AssertionError("no uniform trip")


# ------------------------------------------------------------------------------------------------
# the families
# ------------------------------------------------------------------------------------------------
T0S = (3, -7, 1950)


def n_for(n_bins):
    return 5003 if n_bins < 383 else (1201 if n_bins < 2000 else 401)


def family_A():
    cases, s = [], 0

    def add(kern, C, nb, model, **kw):
        nonlocal s
        s += 1
        cases.append(Case("A", "%s C=%d m%d b%d%s" % (kern, C, model, nb, "".join(" %s=%s" % i for i in kw.items())), kern, n_for(nb), C, nb,
                          model, t0=T0S[s % 3], seed=s, **kw))
    bins_of = {40: (20, 38), 72: (39, 70), 136: (71, 128), 264: (129, 256)}
    for H in FAST_H:
        for cb in ((1, 2, 4, 8) if H < 264 else (1, 2, 4)):
            for m in (0, 1, 2):
                add("fast<%d,%d>" % (cb, H), cb, bins_of[H][m & 1], m)
            add("fast<%d,%d>" % (cb, H), cb, bins_of[H][1], 2 * ((cb + H // 8) & 1))
            add("fast<%d,%d>" % (cb, H), cb, bins_of[H][0], 1)
        if H < 264:
            for m in (0, 1, 2):
                add("wide<%d>" % H, 16, bins_of[H][m & 1], m)
            add("wide<%d>" % H, 9, bins_of[H][1], 2)
            add("wide<%d>" % H, 16, bins_of[H][0], 1)
    for cb, (b0, b1) in ((4, (257, 382)), (2, (383, 766)), (1, (767, LR_MAX_BINS))):
        for m in (0, 1, 2):
            add("generic<%d>x1" % cb, cb, (b0, b1)[m & 1], m)
        add("generic<%d>x1" % cb, cb, b1, 2)
        add("generic<%d>x1" % cb, cb, b0, 1)
    ends = (None, "frac", "before", "beyond")
    for cb, (b0, b1) in ((8, (40, 94)), (4, (95, 190)), (2, (191, 382)), (1, (383, MODEL3_MAX_BINS))):
        for j, nb in enumerate((b0, b1)):
            add("generic<%d>x2" % cb, cb, nb, 3, end=ends[(cb + j) % 2])
        add("generic<%d>x2" % cb, cb, b0, 3, end=ends[2 + (cb == 4 or cb == 1)])
    add("generic<8>x2", 8, 94, 3, end="before")
    add("generic<2>x2", 2, 191, 3, end="beyond")
    # the special rate set, once per model
    add("fast<4,40>", 4, 38, 0, special=True)
    add("wide<72>", 16, 70, 1, special=True)
    add("fast<8,136>", 8, 128, 2, special=True)
    add("generic<4>x2", 4, 95, 3, special=True)
    return cases


B_FAMILIES = (("fast<4,264>", 4, 256, 2), ("wide<136>", 16, 128, 2), ("generic<4>x1", 4, 257, 2), ("generic<8>x2", 8, 94, 3))


def family_B():
    cases = []
    for j, (kern, cb, nb, m) in enumerate(B_FAMILIES):
        for i, C in enumerate((cb, 2 * cb - 1, 8 * cb, 8 * cb + 1, 16 * cb)):
            cases.append(Case("B", "%s C=%d" % (kern, C), kern, 5003, C, nb, m, t0=T0S[(i + j) % 3], seed=100 + 10 * j + i, alone=True))
    return cases


C_KERNELS = (("fast<4,40>", 4, 38, 256), ("generic<4>x1", 4, 257, 256), ("wide<72>", 16, 70, 512))


def family_C():
    cases, s = [], 200
    for kern, C, nb, T in C_KERNELS:
        tails = [1, 2, 3, 2 * T - 1, 2 * T, 2 * T + 1] + ([4 * T - 1, 4 * T + 1, 6 * T + 1] if T == 512 else [])
        ns = [(1, 1), (2, 2), (3, 3)] + [(find_n(r, C, nb, 2, FAMILY_ENV["C"]), r) for r in tails]
        for n, r in ns:
            s += 1
            for off in (False, True):
                c = Case("C", "%s n=%d last=%d%s" % (kern, n, r, " off8" if off else ""), kern, n, C, nb, 2, t0=T0S[s % 3], seed=s, offset=off)
                c.last = r
                cases.append(c)
    return cases


D_KERNELS = (("fast<4,72>", 4, 70), ("fast<8,136>", 8, 128), ("wide<40>", 16, 38))


def family_D():
    cases = []
    for j, (kern, C, nb) in enumerate(D_KERNELS):
        for lay in ("runs", "shuffled", "moved"):
            cases.append(Case("D", "%s %s" % (kern, lay), kern, 6501, C, nb, 2, t0=T0S[j], seed=300 + j, layout=lay))
    return cases


def family_E():
    cases, s = [], 400
    for n in (1, 2, 1023, 1024, 1025):
        for C in (1, 64):
            for m in range(4):
                s += 1
                cases.append(Case("E", "small n=%d C=%d m%d" % (n, C, m), "small", n, C, 30, m, t0=T0S[s % 3], seed=s,
                                  end=(None, "frac")[s & 1] if m == 3 else None))
    for m in range(4):
        cases.append(Case("E", "small special m%d" % m, "small", 1025, 64, 30, m, t0=T0S[m % 3], seed=450 + m, special=True))
    # the three boundaries, both sides; the cases of a pair share lineages and rates so that the shared chains must agree
    N = 1 << 18
    cases.append(Case("E", "n=2^18 C=8", "small", N, 8, 30, 2, seed=1460))
    cases.append(Case("E", "n=2^18+1 C=1", "fast<1,40>", N + 1, 1, 30, 2, seed=1460, extra_before=1, pair="n=2^18 C=8"))
    cases.append(Case("E", "n=2^21/64 C=64", "small", (1 << 21) // 64, 64, 30, 2, seed=2461))
    cases.append(Case("E", "n=2^21/64+1 C=64", "wide<40>", (1 << 21) // 64 + 1, 64, 30, 2, seed=2461, extra_before=1, pair="n=2^21/64 C=64"))
    for m in (0, 2, 3):
        cases.append(Case("E", "C=64 m%d" % m, "small", 2000, 64, 30, m, seed=3462 + m))
        cases.append(Case("E", "C=65 m%d" % m, "generic<8>x2" if m == 3 else "wide<40>", 2000, 65, 30, m, seed=3462 + m, pair="C=64 m%d" % m))
    # (a window one bin longer is another likelihood: these pairs are compared with their references - but in models 0 / 1 a
    # last bin with br_length 0 scores nothing: the masked case computes the 1918-bin number on the tiled path)
    cases.append(Case("E", "bins=1918 m0", "small", 401, 2, 1918, 0, seed=4470))
    cases.append(Case("E", "bins=1919 m0", "generic<1>x1", 401, 2, 1919, 0, seed=5470))
    cases.append(Case("E", "bins=1919 m0 last bin masked", "generic<1>x1", 401, 2, 1919, 0, seed=4470, masked_last_bin=True, pair="bins=1918 m0"))
    cases.append(Case("E", "bins=1918 m2", "small", 401, 2, 1918, 2, seed=4471))
    cases.append(Case("E", "bins=1919 m2", "generic<1>x1", 401, 2, 1919, 2, seed=5471))
    cases.append(Case("E", "bins=958 m3", "small", 401, 2, 958, 3, seed=4472))
    cases.append(Case("E", "bins=959 m3", "generic<1>x2", 401, 2, 959, 3, seed=5472, end="frac"))
    for st in (1, 4):
        cases.append(Case("E", "session %d general m3" % st, "small", 3001, st, 60, 3, seed=480 + st, end="frac", session=2))
        cases.append(Case("E", "session %d edge m3" % st, "small", N_EDGE3, st, 60, 3, seed=490 + st, session=2))
    return cases


def family_F():
    cases = []
    for j, (H, nb) in enumerate(((40, 38), (72, 70), (136, 128))):
        for C in (64, 65):
            cases.append(Case("F", "fast<8,%d> C=%d" % (H, C), "fast<8,%d>" % H, 5003, C, nb, 2, t0=T0S[j], seed=500 + 2 * j + (C & 1), alone=False))
    return cases


FAMILIES = dict(A=family_A, B=family_B, C=family_C, D=family_D, E=family_E, F=family_F)

TILED_KERNELS = (["fast<%d,%d>" % (cb, H) for H in FAST_H for cb in ((1, 2, 4, 8) if H < 264 else (1, 2, 4))]
                 + ["wide<%d>" % H for H in (40, 72, 136)] + ["generic<%d>x1" % cb for cb in (4, 2, 1)]
                 + ["generic<%d>x2" % cb for cb in (8, 4, 2, 1)])


def all_cases():
    return [c for f in "ABCDEF" for c in FAMILIES[f]()]


# ------------------------------------------------------------------------------------------------
# the child
# ------------------------------------------------------------------------------------------------
def say(*a):
    print(*a)
    sys.stdout.flush()


def main(argv):
    fam = argv[0]
    env = FAMILY_ENV[fam]
    for k in ("LR_LOGLIK_SMALL", "LR_SCAN_WIDE"):
        assert os.environ.get(k) == env.get(k), "family %s runs with %s=%r" % (fam, k, env.get(k))
    import torch
    from literate_amd import _hip, ops
    lib = _hip.load()
    dev = torch.device("cuda")
    worst, got_by_name = 0.0, {}

    def dev_pair(d, offset):
        n = len(d["ts"])
        out = []
        for x in (d["ts"], d["te"]):
            buf = torch.empty(n + 2, dtype=torch.float64, device=dev)
            t = buf[1:n + 1] if offset else buf[:n]
            t.copy_(torch.as_tensor(x))
            assert t.data_ptr() % 16 == (8 if offset else 0) and t.is_contiguous()
            out.append(t)
        return out

    def check(c, label, got, want, tol):
        nonlocal worst
        r = R.ratios(got, want, tol)
        say("%-44s %-16s n=%-7d C=%-3d error / tolerance = %.3f" % (label, c.reached(), c.n, len(got), r.max()))
        worst = max(worst, float(r.max()))
        return r

    failed = []
    for c in FAMILIES[fam]():
        assert c.reached() == c.kernel, (c.name, c.reached(), c.kernel)
        if c.kernel != "small":
            p = plan(c.n, c.C, c.n_bins, c.model, env.get("LR_SCAN_WIDE") != "0")
            out = (CT.c_int32 * 4)()
            assert lib.lr_bd_loglik_plan(c.n, c.n_bins, c.C, c.model, out) == 0
            assert tuple(out) == (p.cb, p.tiles, p.H, p.groups), (c.name, tuple(out), p)
        d = c.data()
        want, tol, L, A = c.reference()
        ts, te = dev_pair(d, c.offset)
        if c.session:
            ses = ops.LoglikSession(ts, te, c.t0, c.n_bins, c.C, c.model, d["br"], c.end_time)
            assert ses.zero_copy
            for call in range(c.session):
                got = np.array(ses(d["lam"], d["mu"]), dtype=np.float64)
                assert ses.zero_copy, "the zero-copy result did not arrive by polling"
                r = check(c, "%s call %d" % (c.name, call), got, want, tol)
                if r.max() > 1.0:
                    failed.append(c.name)
        else:
            got = ops.bd_loglik_batch(ts, te, c.t0, d["lam"], d["mu"], c.model, d["br"], c.end_time).cpu().numpy()
            r = check(c, c.name, got, want, tol)
            if r.max() > 1.0:
                failed.append(c.name)
        got_by_name[c.name] = (got, tol)
        if c.offset:                                  # the aligned twin ran just before: the same summation order
            twin = got_by_name[c.name[:-5]][0]
            assert twin.tobytes() == got.tobytes(), "%s: aligned and offset results differ" % c.name
        if c.pair:
            g0, t0_ = got_by_name[c.pair]
            m = min(len(g0), len(got))
            fin = np.isfinite(g0[:m])
            assert np.all(np.abs(g0[:m][fin] - got[:m][fin]) <= (t0_[:m] + tol[:m])[fin]), "%s and %s disagree" % (c.name, c.pair)
        if c.alone:
            dpt = depth(c.n, 1, c.n_bins, c.model, env)
            cst = R.constant(d["lam"], c.model, d["br"]) if c.model == 1 else None
            tol1 = R.tolerance(L, A, dpt, c.n_bins, cst)
            lam_d, mu_d = torch.as_tensor(d["lam"]).to(dev), torch.as_tensor(d["mu"]).to(dev)
            one = np.array([float(ops.bd_loglik_batch(ts, te, c.t0, lam_d[k:k + 1], mu_d[k:k + 1], c.model, d["br"], c.end_time)[0])
                            for k in range(c.C)])
            r = check(c, c.name + " each alone", one, want, tol1)
            if r.max() > 1.0:
                failed.append(c.name + " alone")
    if fam == "A":
        assert lib.lr_bd_loglik_workspace_bytes(401, LR_MAX_BINS + 1, 1, 2) == ERR_SIZE
        assert lib.lr_bd_loglik_workspace_bytes(401, MODEL3_MAX_BINS + 1, 1, 3) == ERR_SIZE
        assert lib.lr_bd_loglik_workspace_bytes(401, MODEL3_MAX_BINS, 1, 3) > 0
    torch.cuda.synchronize()
    assert not failed, "outside the bound: %s" % failed
    say("family %s ok: worst ratio %.3f" % (fam, worst))


if __name__ == "__main__":
    main(sys.argv[1:])
