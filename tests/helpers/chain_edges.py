"""The chain engine at its chain-count edges.

The number of chains decides the table grouping cb, the kernel family, its block shape, the partitions of the launches
and which slots of the last block, team or pair group stay empty.  A CASE is (configuration, engine, kwargs, chains); a
SIGNATURE names the class a chain count falls in for a (configuration, engine): tests/test_chain_edges_host.py walks the
planner over the chain counts on the host for every configuration and engine and pins where the signature changes, and
tests/test_hip_chain_edges.py runs every case against the oracle loops and checks that each signature of the walk was run
(the pairs without a case: EXCLUDED).
"""
import collections
import contextlib
import functools
import os

import numpy as np

from helpers import edges as E

N_IT, FIRST, SEED = 60, 25, 7117
HOST_CUS = 256

Config = collections.namedtuple("Config", "model sampler general n_bins n")
# (model, sampler, general times, bins, synthetic lineages): what each reaches is in DESIGN.md's testing notes
CONFIGS = {
    "A": Config(0, 0, False, 24, 3000),       # H = 40
    "B": Config(0, 0, True, 24, 3000),        # pair-general tables, the wide scan
    "C": Config(3, 0, False, 24, 3000),       # H = 72 with the extant block; the generic scan under `launch`
    "D": Config(2, 0, False, 300, 3000),      # H = 520: persistent kernels and the packed scan at two pairs per block only
    "E": Config(2, 1, False, 24, 3000),       # DDRate (m_birth = m_death = 2): the parametric kernels
    "F": Config(2, 2, True, 24, 3000),        # trend_rate on pair-general tables
    "G": Config(0, 0, False, 24, 25000),      # more than 1536 groups: lr_spec_kernel mode 3, 1024-thread lr_persist_kernel
}
KIND = {1: "dd", 2: "trend"}
RJ_ENGINES = ("auto", "launch", "packed", "persistent2", "persistent4", "spec")
WALK = tuple(range(1, 73)) + (255, 256, 257, 258, 511, 512, 513, 514, 1023, 1024, 1025, 1026, 1027)


def data(name):
    cfg = CONFIGS[name]
    return E.lineages(cfg.n_bins, cfg.general, True, cfg.n)


def n_lineages(name):
    return len(data(name)[0])


# ---- the planner on the host ----------------------------------------------------------------------------------------
def query(name, engine, kwargs, n_chains, cus=HOST_CUS):
    """lr_mcmc_query_layout for a case (kwargs: ChainEngine's team / chains_per_team; chain_offset and env do not reach
    the layout call's arguments - env is the caller's to set)."""
    cfg = CONFIGS[name]
    rc, lay = E.query(cfg.model, cfg.sampler, not cfg.general, cfg.n_bins, n_chains, n_lineages(name), E.ENGINES[engine],
                      cus=cus, team=kwargs.get("team", 0), chains_per_team=kwargs.get("chains_per_team", 0))
    assert rc == 0, (name, engine, kwargs, n_chains, rc)
    return lay


def half_stride(lay):
    return lay.table_stride // (2 if lay.table_mode == 2 else 1)


def packscan_pairs(H, n_chains):
    """lr_packscan_pairs (csrc/lr_packscan.hip): chain pairs per block of the packed scan - four, while the block's
    LR_UNIT_PLANES (6) planes of H double2 entries per pair fit 120 KB of LDS and half of them would not hold all pairs."""
    n_pairs, pairs = (n_chains + 1) // 2, 4
    while pairs > 1 and (pairs * 6 * H * 16 > 120 * 1024 or pairs // 2 >= n_pairs):
        pairs >>= 1
    return pairs


Sig = collections.namedtuple("Sig", "engine family cb table_mode packed threads team cpb extra")


def signature(lay, engine, n_chains):
    """The class a chain count falls in: what the layout says of the kernel, its tables and its block shape, for the
    launches also their partitions, and what the layout does not carry - the packed scan's pairs per block and the
    residue of the chain count that decides which slots of the last block (quad, pair, team) stay empty."""
    extra = ()
    if lay.persistent == 0:
        extra += (("parts", lay.n_parts), ("pipelined", lay.pipelined))
    if lay.packed_scan:
        extra += (("PAIRS", packscan_pairs(half_stride(lay), n_chains)), ("mod2", n_chains % 2))
    elif lay.persistent == 2:
        extra += (("mod4", n_chains % 4),)
    elif lay.persistent in (1, 3):
        extra += (("mod2", n_chains % 2),)
    return Sig(engine, lay.persistent, lay.chains_per_block, lay.table_mode, lay.packed_scan, lay.reserved1, lay.team_blocks,
               lay.spec_chains_per_team, extra)


def engine_kwargs(kwargs):
    return {k: v for k, v in kwargs.items() if k in ("team", "chains_per_team", "chain_offset")}


def walk(name, engine, kwargs, counts=WALK, cus=HOST_CUS):
    """{chains: signature} over the chain counts of the walk (the caller has set the case's environment)."""
    return {c: signature(query(name, engine, kwargs, c, cus), engine, c) for c in counts}


def boundaries(sigs, field):
    """Chain counts of a walk {chains: value} at which field(value) differs from the count before it in the walk."""
    keys = sorted(sigs)
    return [(c, field(sigs[c])) for p, c in zip(keys, keys[1:]) if field(sigs[p]) != field(sigs[c])]


# ---- the cases ------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "config engine kwargs chains")


def team_cap(cus, k, cpb):
    """Most chains a forced team of k blocks with cpb chains runs: a team per block slot of the cus compute units."""
    return cpb * (cus // k)


class Count(collections.namedtuple("Count", "k cpb add")):
    """A chain count that follows the device: add chains beside cpb * floor(CUs / k) - k = 1: cpb x the compute units;
    else the cap of a forced team of k blocks with cpb chains."""

    def __add__(self, n):
        return Count(self.k, self.cpb, self.add + n)

    def __sub__(self, n):
        return Count(self.k, self.cpb, self.add - n)

    def __str__(self):
        head = ("%dCUs" % self.cpb if self.cpb > 1 else "CUs") if self.k == 1 else "cap"
        return head + ("%+d" % self.add if self.add else "")


def resolve(chains, cus):
    return team_cap(cus, chains.k, chains.cpb) + chains.add if isinstance(chains, Count) else int(chains)


def resolved(case, cus=HOST_CUS):
    """The case with its chain count as a number on a device of `cus` compute units."""
    return case._replace(chains=resolve(case.chains, cus))


N_CASES = 442      # 352 from the counts listed for each engine + 90 for the classes of the walk those leave out


def cases():
    """Every (configuration, engine, kwargs, chains); kwargs: team, chains_per_team, chain_offset of the engine, env =
    {variable: value} to set around the planner and the engine; chains: a number or a Count that follows the device."""
    out = []
    cus, cus2 = Count(1, 1, 0), Count(1, 2, 0)

    def add(configs, engine, counts, **kw):
        for name in configs:
            for c in counts:
                out.append(Case(name, engine, dict(kw), c))

    add("A", "launch", (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 48, 49, 65))
    add("B", "launch", (1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 33))
    add("CEF", "launch", (1, 2, 3, 5, 8, 9, 17))
    add("ABE", "persistent4", (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 18, 19))
    add("A", "persistent4", (1023, 1024, 1025, 1027))
    add("CDF", "persistent4", (3, 5, 6, 7, 9, 17))
    add("ACDE", "persistent2", (2, 3, 4, 5, 8, 9, 16, 17))
    add("G", "persistent2", (2, 3, 511, 512, 513, 514))
    add("ABCEF", "spec", (1, 2, 3, 4, 5, 8, 9, 16, 17))
    add("AB", "spec", (cus - 1, cus, cus + 1, cus + 2, cus2 - 1, cus2, cus2 + 1))
    add("G", "spec", (1, 2, 3))
    for k in (2, 4, 8):
        for cpb in (1, 2):
            cap = Count(k, cpb, 0)
            add("A", "spec", (1, 2, 3, cap - 1, cap, cap + 1), team=k, chains_per_team=cpb)
            if k == 4:
                add("B", "spec", (1, 2, 3, cap - 1, cap, cap + 1), team=k, chains_per_team=cpb)
    add("ABCE", "packed", (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17))
    add("D", "packed", (3, 4, 5, 7, 8, 9))
    add("AB", "packed", (9, 15, 16, 17, 23, 24, 25), env={"LR_PACKED_PARTS": "2"})
    add("ABE", "auto", (1, 2, 3, cus, cus + 1, cus2, cus2 + 1))
    add("G", "auto", (1024, 1025))
    for engine in RJ_ENGINES:
        add("A", engine, (6,), chain_offset=3)
    for engine in ("persistent4", "spec"):
        add("A", engine, (7,), chain_offset=5)
    # The classes of the host walk (WALK) that the counts above leave out, each at its smallest count - written out, not
    # derived from the walk: a planner threshold that moves must fail the coverage test, not move the cases with it.
    add("E", "launch", (32, 49))                                      # pipelined halves, two partitions
    add("F", "launch", (25,))
    add("CD", "persistent4", (1, 2, 4, 8, 16, 18, 19))                # unit tables for a lone chain: the two-chain kernel
    add("F", "persistent4", (4,))
    add("ACDEG", "persistent2", (1,))                                 # A, E, G: the launches; C, D: a half-filled block
    add("G", "persistent2", (4, 5, 8))
    add("CEF", "spec", (cus + 1, cus + 2, cus2 + 1))               # a team per pair; beyond it the launches
    add("G", "spec", (4, 5, 8, 9, 16, cus + 1, cus + 2, cus2 + 1))
    for k in (2, 4, 8):
        for cpb in (1, 2):
            add("A", "spec", (4, 5, 8), team=k, chains_per_team=cpb)
    add("A", "spec", (49,), team=8, chains_per_team=1)                # beyond the cap: the launches in two partitions
    add("D", "packed", (1, 2))
    add("AE", "auto", (4, 5, 33, cus2 + 2))
    add("E", "auto", (8,))
    add("B", "auto", (cus2 + 2, 1023, 1024))
    add("G", "auto", (1, 2, 3, 4, 5, 8, 32, 33, cus + 1, cus + 2, cus2 + 1, cus2 + 2, 1023, 1026))
    return out


def case_id(case):
    kw = case.kwargs
    tag = case.engine
    if kw.get("team"):
        tag += "-k%dx%d" % (kw["team"], kw["chains_per_team"])
    if kw.get("env"):
        tag += "-" + "-".join("%s%s" % (k.split("_")[-1].lower(), v) for k, v in sorted(kw["env"].items()))
    if kw.get("chain_offset"):
        tag += "-off%d" % kw["chain_offset"]
    return "%s-%s-%s" % (case.config, tag, case.chains)


def variant(case):
    """What a walk is made for: the case without its chain count and offset (the layout does not see the offset)."""
    kw = case.kwargs
    return (case.config, case.engine, kw.get("team", 0), kw.get("chains_per_team", 0), tuple(sorted(kw.get("env", {}).items())))


def variant_kwargs(v):
    return dict(team=v[2], chains_per_team=v[3], env=dict(v[4]))


@contextlib.contextmanager
def environment(kwargs):
    """A case's environment variables around the planner and the engine (the planner reads LR_PACKED_PARTS per call)."""
    env = kwargs.get("env", {})
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def case_signature(case, cus=HOST_CUS):
    """The planner's class for a case (its chain count a number: resolved())."""
    with environment(case.kwargs):
        return signature(query(case.config, case.engine, case.kwargs, case.chains, cus), case.engine, case.chains)


# What the host walk covers beside every (configuration, engine) as it stands: the forced teams and the environment the
# cases use, written out so that the walk does not follow the cases.
WALKED_VARIANTS = tuple([("A", "spec", k, cpb, ()) for k in (2, 4, 8) for cpb in (1, 2)] +
                        [("B", "spec", 4, cpb, ()) for cpb in (1, 2)] +
                        [(name, "packed", 0, 0, (("LR_PACKED_PARTS", "2"),)) for name in "AB"])
# (configuration, engine) pairs that have NO case, with the number of classes the walk finds for each (81 in all): the
# pairs beyond the ones the cases were asked for.  Covering them takes about 81 more cases, and the case count is held
# at N_CASES.  tests/test_chain_edges_host.py holds this list to the walk: a pair cannot lose its cases unseen, and an
# excluded pair whose classes change shows up.
EXCLUDED = {("B", "persistent2"): 7, ("C", "auto"): 12, ("D", "auto"): 8, ("D", "launch"): 4, ("D", "spec"): 4,
            ("F", "auto"): 8, ("F", "packed"): 6, ("F", "persistent2"): 7, ("G", "launch"): 7, ("G", "packed"): 6,
            ("G", "persistent4"): 12}


def walked(cus=HOST_CUS):
    """{(configuration, engine): {signature: smallest chain count}} of the host walk over EVERY configuration and engine
    (and the variants of WALKED_VARIANTS), whatever cases there are."""
    variants = [(name, engine, 0, 0, ()) for name in sorted(CONFIGS) for engine in RJ_ENGINES] + list(WALKED_VARIANTS)
    out = {}
    for v in variants:
        kw = variant_kwargs(v)
        with environment(kw):
            sigs = walk(v[0], v[1], kw, cus=cus)
        known = out.setdefault((v[0], v[1]), {})
        for c in sorted(sigs, reverse=True):
            known[sigs[c]] = min(c, known.get(sigs[c], c))
    return out


def uncovered(ran, cus=HOST_CUS):
    """What coverage asks of ran = {(configuration, engine): signatures with a case}: the pairs without any are exactly
    EXCLUDED, with the class counts written there, and every class of every other pair is in ran.  Returns the failures."""
    bad = {}
    for pair, sigs in walked(cus).items():
        if pair in EXCLUDED:
            if ran.get(pair) or len(sigs) != EXCLUDED[pair]:
                bad[pair] = "excluded with %d classes, the walk finds %d, cases: %d" % (EXCLUDED[pair], len(sigs), len(ran.get(pair, ())))
        else:
            missing = sorted((c, s) for s, c in sigs.items() if s not in ran.get(pair, ()))
            if missing:
                bad[pair] = missing
    return bad


def followed(n_chains):
    """Local indices of the chains a case follows row by row."""
    return sorted({c for c in (0, 1, n_chains // 2, n_chains - 2, n_chains - 1) if 0 <= c < n_chains})


# ---- what a case is meant to hit ------------------------------------------------------------------------------------
AUTO_BEYOND = {"A": (1, 1), "B": (2, 2), "E": (1, 1), "G": (2, 1)}      # engine="auto" above 2 CUs chains: up to 1024, above


def expected_family(case, cus=HOST_CUS):
    """The kernel family (layout.persistent; "packed" for the packed scan, "launch" for the launches on ts / te) a case
    is meant to run, restated from the planner's rules for the configurations above.  A forced engine that cannot run
    a count falls back, and the case says to what:
      persistent4  needs cb >= 4, which general times always have (the pair-general layout, cb 4); at unit resolution two
                   chains run the two-chain kernel, and so does a lone chain where it keeps unit tables (model 3, H = 520)
                   - elsewhere it cannot fill a pair entry and has the pair-general layout
      persistent2  unit resolution; a lone chain on general tables (models 0-2 up to 254 bins) runs the launches
      spec         a team per chain up to the CUs, per pair up to twice as many, with a forced team of k blocks
                   cpb * floor(CUs / k) chains; beyond, the launches
      packed       always
      auto         (these sizes) the speculative kernel up to 2 CUs chains, then the persistent kernel of AUTO_BEYOND"""
    cfg, kw, C = CONFIGS[case.config], case.kwargs, case.chains
    lone_general = C == 1 and (cfg.general or (cfg.model != 3 and E.launch_class(cfg.model, cfg.n_bins) is not None))
    if case.engine == "launch":
        return "launch"
    if case.engine == "packed":
        return "packed"
    if case.engine == "persistent2":
        return "launch" if lone_general else 1
    if case.engine == "persistent4":
        return 2 if (cfg.general or lone_general or C > 2) else 1
    if case.engine == "spec":
        k, cpb = kw.get("team", 0), kw.get("chains_per_team", 0)
        cap = team_cap(cus, k, cpb) if k else 2 * cus
        return 3 if C <= cap else "launch"
    assert case.engine == "auto"
    return 3 if C <= 2 * cus else AUTO_BEYOND[case.config][0 if C <= 1024 else 1]


def expected_signature(case, cus=HOST_CUS):
    """The whole class a case is meant to hit, restated from the planner's rules (csrc/lr_plan.hip, lr_plan_scan) and NOT
    asked of the planner: family, table grouping, table mode, block width, team, and the launches' partitions and
    schedule.  A threshold that moves in the planner makes the cases at it fail."""
    cfg, kw, C = CONFIGS[case.config], case.kwargs, case.chains
    fam = expected_family(case, cus)
    classed = cfg.model != 3 and E.launch_class(cfg.model, cfg.n_bins) is not None
    # the tables: pair-general (2) under a persistent kernel or the packed scan on general times and for a lone chain that
    # cannot fill a pair entry, general (0) under the launches there and where they have no table class, else unit (1)
    if cfg.general or (C == 1 and classed):
        mode = 0 if fam == "launch" else 2
    else:
        mode = 0 if (fam == "launch" and not classed) else 1
    # the grouping: four for pair-general tables; unit tables 2, 4, 8, 16 from 1, 3, 5, 9 chains; general tables 1, 2, 4, 8
    # from 1, 2, 3, 5 and sixteen (one pass of the wide scan) for 9..16 where there is a table class, eight beyond
    if mode == 2:
        cb = 4
    elif mode == 1:
        cb = 2 if C <= 2 else (4 if C <= 4 else (8 if C <= 8 else 16))
        if fam == "packed":
            cb = min(cb, 8)               # (lr_packscan_plan: eight chains per partition boundary)
    else:
        cb = C if C <= 2 else (4 if C <= 4 else (8 if C <= 8 else (16 if classed and C <= 16 else 8)))
    threads = {1: 1024 if ((C + 1) // 2 <= 256 and n_lineages(case.config) >= 20000) else 512, 2: 1024, 3: 768}.get(fam, 0)
    team, cpb = 0, 0
    if fam == 3:
        team, cpb = (kw["team"], kw["chains_per_team"]) if kw.get("team") else (1, 1 if C <= cus else 2)
    extra = ()
    if fam == "launch":
        # pipelined halves from two groups, two partitions from four: 32 / 49 chains on unit tables (cb 16), 17 / 25 on
        # general tables with a class (cb 8); the generic scan (model 3) is never pipelined, two partitions from two groups
        if mode == 1:
            parts, pipe = (2 if C >= 49 else 1), int(C >= 32)
        elif classed:
            parts, pipe = (2 if C >= 25 else 1), int(C >= 17)
        else:
            parts, pipe = (2 if C >= 9 else 1), 0
        extra = (("parts", parts), ("pipelined", pipe))
    elif fam == "packed":
        # (pair-general tables are grouped by four chains, unit tables by up to sixteen: LR_PACKED_PARTS=2 makes two
        # partitions from two groups of at least eight chains)
        two = kw.get("env", {}).get("LR_PACKED_PARTS") == "2" and C > (4 if mode == 2 else 8)
        H = E.table_class(cfg.model, cfg.n_bins)
        extra = (("parts", 2 if two else 1), ("pipelined", 0), ("PAIRS", packscan_pairs(H, C)), ("mod2", C % 2))
    elif fam == 2:
        extra = (("mod4", C % 4),)
    else:
        extra = (("mod2", C % 2),)
    return Sig(case.engine, fam if isinstance(fam, int) else 0, cb, mode, int(fam == "packed"), threads, team, cpb, extra)


def family_of(lay):
    return lay.persistent if lay.persistent else ("packed" if lay.packed_scan else "launch")


def check_class(case, lay, kernel, cus):
    """Before a case runs: the layout and the kernel name (None on the host: the layout alone) say the case hits the class
    it names (expected_signature).  Returns the signature."""
    sig, want = signature(lay, case.engine, case.chains), expected_signature(case, cus)
    assert sig == want, (case_id(case), "runs", sig, "is for", want, kernel)
    got = family_of(lay)
    if kernel is None:
        return sig
    head = {1: "lr_persist_kernel<", 2: "lr_persist4_kernel<", 3: "lr_spec_kernel<", "packed": "lr_packscan_kernel<"}.get(got)
    assert head is None or kernel.startswith(head), (case_id(case), kernel)
    if got == "launch":
        # pipelined halves run the fused kernel; sixteen chains on general tables the wide scan; else a scan per group
        name = "lr_fused_iter_kernel<" if lay.pipelined else ("lr_scan_wide_kernel<" if (sig.table_mode == 0 and sig.cb == 16) else "lr_scan")
        assert kernel.startswith(name), (case_id(case), kernel, name)
    if got == "packed":
        args = kernel[kernel.index("<") + 1:-1].split(",")
        assert int(args[0]) == dict(sig.extra)["PAIRS"], (case_id(case), kernel)
    if got == 1:
        assert kernel.endswith(", %d>" % lay.reserved1), (case_id(case), kernel)
    return sig


# ---- the oracle, by (configuration, global chain id) ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rj_stats(name):
    cfg = CONFIGS[name]
    ts, te = data(name)
    return E.rj_stats(ts, te, cfg.model, cfg.n_bins)


@functools.lru_cache(maxsize=None)
def rj_trajectory(name, chain):
    cfg = CONFIGS[name]
    ts, te = data(name)
    return E.rj_trajectory(rj_stats(name), ts, te, cfg.model, SEED, N_IT, chain)


@functools.lru_cache(maxsize=None)
def lineage_bins(name):
    from oracle import literate_oracle as lo
    ts, te = data(name)
    return lo.lineage_bins(ts, te, 0.0, CONFIGS[name].n_bins)


@functools.lru_cache(maxsize=None)
def param_data(name):
    cfg = CONFIGS[name]
    ts, te = data(name)
    bins, trend = E.param_stats(KIND[cfg.sampler], ts, te, cfg.n_bins)
    return ts, te, bins, trend


@functools.lru_cache(maxsize=None)
def param_emp(name):
    nsp, nex, dt = param_data(name)[2][2:5]
    with np.errstate(all="ignore"):
        return nsp / dt, nex / dt


@functools.lru_cache(maxsize=None)
def param_trajectory(name, chain):
    _, _, bins, trend = param_data(name)
    _, refs = E.param_reference(KIND[CONFIGS[name].sampler], bins, trend, N_IT, 1, SEED, chain, chains=(0,))
    return refs[0]


# ---- checks on what a run leaves (plain arrays: the host test feeds them fabricated output) -------------------------
def check_every_chain(snap, tr, n_it):
    """Every chain of a run: n_it iterations done, a finite log-likelihood, the sampled rows' iteration column counting
    the iterations (s_freq 1: the oracle's rows carry 0 .. n_it - 1), and no two chains ending in the same accepted state."""
    C = len(snap["likA"])
    assert np.all(snap["it"] == n_it), snap["it"]
    assert np.all(np.isfinite(snap["likA"])), snap["likA"]
    assert tr.shape[:2] == (n_it, C), tr.shape
    assert np.array_equal(tr[:, :, 0], np.broadcast_to(np.arange(n_it, dtype=float)[:, None], (n_it, C))), tr[:, :, 0]
    check_distinct_states(snap)


def check_distinct_states(snap):
    """No two chains end with bit-identical state rows (rates, shift times, log-likelihood, log-prior): a ragged slot that
    mirrors its neighbour carries a likelihood that is right for the mirrored state."""
    seen = {}
    for c in range(len(snap["likA"])):
        key = b"|".join(np.ascontiguousarray(x, dtype=np.float64).tobytes() for x in
                        (snap["L"][c], snap["M"][c], snap["tL"][c], snap["tM"][c], snap["likA"][c], snap["priorA"][c]))
        assert key not in seen, "chains %d and %d end in the same state" % (seen[key], c)
        seen[key] = c


def check_rj_case(tr, snap, name, chain_offset, cell):
    """An RJ case's leavings against the oracle: the followed chains row by row, every chain's accepted state re-scored."""
    cfg = CONFIGS[name]
    ts, te = data(name)
    C = len(snap["likA"])
    refs = {c: rj_trajectory(name, chain_offset + c) for c in followed(C)}
    E.check_rj_rows(tr, refs, N_IT, cell)
    rates = E.check_rj_states(snap, ts, te, cfg.model, cfg.n_bins, rj_stats(name), N_IT, cell, lineage_bins(name))
    check_every_chain(snap, tr, N_IT)
    return rates


def check_param_case(rows, tr, snap, name, chain_offset, cell):
    """A DDRate / trend_rate case's leavings against the oracle: rows = {chain's index: its log rows} of the followed chains
    (the engine's log_rows_from of tr, with the adequacy columns) row by row, and every chain's end state."""
    C = len(snap["likA"])
    assert sorted(rows) == followed(C), (cell, sorted(rows))
    for c in followed(C):
        E.check_param_rows(rows[c], param_trajectory(name, chain_offset + c), N_IT, cell, c)
    check_every_chain(snap, tr, N_IT)
