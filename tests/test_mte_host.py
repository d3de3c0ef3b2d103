"""The multi-trait extinction model without a GPU (literate_amd/mte.py, ops.mte_tables, tests/helpers/mte_ref.py):

  1  the grouped likelihood equals the per-lineage one (MTEmodel.py:336-354) on the example file - whole and in three slices -
     and on random data, within the bound of a reordered sum
  2  slicing, state mapping and grouping on hand-made tables
  3  the log's header and file name, 2 ln BF
  4  every refusal of the driver, by its message
  5  every case of tests/test_hip_mte.py is held to the tie condition
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import mte_ref as mr          # noqa: E402

EPS = np.finfo(float).eps


def reordered_sum_bound(n_terms, magnitude):
    """two orders of one sum of n terms differ by at most about n eps sum |terms| (tests/test_hip_score.py's bound)"""
    return n_terms * EPS * magnitude


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
def test_1_grouped_equals_per_lineage_on_the_example_whole_and_in_slices():
    from literate_amd import ops
    ts, te, traits, names = mr.read_example()
    assert len(ts) == 4752 and traits.shape[1] == 6 and names[-1] == "redundancy"
    tab = ops.mte_tables(ts, te, traits, mr.EXAMPLE_SLICES)
    assert tab["code"].shape == (392, 6) and tab["n_states"].tolist() == [5, 5, 5, 6, 6, 5]
    assert [int((x > 0).sum()) for x in tab["n"]] == [392, 281, 358, 164], "combinations held per slice"
    D = mr.Data(tab["code"], tab["n_states"], tab["n"], tab["E"], tab["B"])
    for p, (t0, t1) in enumerate(mr.EXAMPLE_SLICES):
        kept, bl, ex = ops.mte_slice(ts, te, t0, t1)
        tr = tab["code"][tab["combo"][kept]].astype(np.int64)
        assert kept.sum() == tab["n"][p].sum() > 0
        for k, I in enumerate(("ones", "zeros", "mixed")):
            m, Y, ind = mr.random_params(D, 1, 31 + k, I)
            want, mag = mr.loglik_lineages(bl, ex, tr, tab["n_states"], m[0], Y[0], ind[0])
            got = mr.loglik_grouped(D, p, m[0], Y[0], ind[0])
            # (the grouped form splits log(m w / Z): the terms E log(m / Z) and E log w bound its magnitude as well)
            assert abs(got - want) <= reordered_sum_bound(len(bl), 3 * mag), (p, I, got, want)
    assert tab["n"][0].sum() == 4752


@pytest.mark.parametrize("G,n_states", [(1, mr.T1), (65, mr.T3), (300, mr.T16), (1024, mr.T16)])
def test_1_grouped_equals_per_lineage_on_random_data(G, n_states):
    D, (combo, bl, ex, tr, keep) = mr.synthetic(2, G, n_states, 77)
    for p in range(2):
        for k, m_fixed in enumerate((None, 1e-6, 1e3)):
            m, Y, ind = mr.random_params(D, 1, 41 + k, "mixed", m_fixed)
            want, mag = mr.loglik_lineages(bl[keep[p]], ex[keep[p]], tr[keep[p]], D.n_states, m[0], Y[0], ind[0])
            got = mr.loglik_grouped(D, p, m[0], Y[0], ind[0])
            assert abs(got - want) <= reordered_sum_bound(int(keep[p].sum()), 3 * mag + abs(want)), (p, got, want)
    assert (D.n[1] == 0).any() or G == 1, "the second problem leaves combinations empty"


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_2_slicing_state_mapping_and_grouping():
    from literate_amd import ops
    #            ts    te   A   B
    rows = [(30.0, 20.0, 7, 2),        # dies in the old slice
            (25.0, 5.0, 3, 2),         # spans both: extant in the old slice, extinct in the young one
            (12.0, 0.0, 3, 9),         # extant: 2 time units in the old slice, 10 in the young one
            (9.0, 8.0, 7, 2),          # te = 8: not < t1 side of the old slice (ts > 10 fails), dies in the young one
            (40.0, 35.0, 5, 9)]        # before both slices
    ts, te = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    traits = np.array([[r[2], r[3]] for r in rows])
    slices = [(28.0, 10.0), (10.0, 0.0)]
    tab = ops.mte_tables(ts, te, traits, slices)
    # states of the WHOLE table in sorted order: A {3, 5, 7} -> 0, 1, 2; B {2, 9} -> 0, 1; combinations in lexicographic order
    assert [u.tolist() for u in tab["states"]] == [[3, 5, 7], [2, 9]] and tab["n_states"].tolist() == [3, 2]
    assert tab["code"].tolist() == [[0, 0], [0, 1], [1, 1], [2, 0]] and tab["combo"].tolist() == [3, 0, 1, 3, 2]
    # old slice (28, 10]: lineage 0 (ts clipped to 28: bl 8, extinct at 10), lineage 1 (ts 25, te 5 <= 10: extant, bl 15) and
    # lineage 2 (ts 12: extant, bl 2)
    assert tab["n"][0].tolist() == [1, 1, 0, 1] and tab["E"][0].tolist() == [0, 0, 0, 1] and tab["B"][0].tolist() == [15, 2, 0, 8]
    # young slice (10, 0]: lineage 1 (ts clipped to 10, dies at 5: bl 5), 2 (extant, bl 10), 3 (ts 9, te 8: bl 1); state 5 of A
    # (code 1) is absent from both slices but keeps its place
    assert tab["n"][1].tolist() == [1, 1, 0, 1] and tab["E"][1].tolist() == [1, 0, 0, 1] and tab["B"][1].tolist() == [5, 10, 0, 1]
    kept, bl, ex = ops.mte_slice(ts, te, np.inf, 0.0)
    assert kept.all() and bl.tolist() == [10, 20, 12, 1, 5] and ex.tolist() == [1, 1, 0, 1, 1]


def test_2_the_example_in_slices_adds_up():
    from literate_amd import ops
    ts, te, traits, _ = mr.read_example()
    edges = [(np.inf, 23.0), (23.0, 8.0), (8.0, 0.0)]
    tab = ops.mte_tables(ts, te, traits, [(np.inf, 0.0)] + edges)
    # consecutive slices cut every lifetime into pieces: lineage-time adds up, every extinction falls into one slice
    np.testing.assert_allclose(tab["B"][1:].sum(), tab["B"][0].sum(), rtol=1e-12)
    assert tab["E"][1:].sum() == tab["E"][0].sum() == (te > 0).sum()


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_3_header_file_name_and_bayes_factor():
    from literate_amd import mte
    assert mte.header(["diet", "size"], [2, 3]) == ["it", "posterior", "likelihood", "prior", "mean_r", "I_diet", "I_size", "m_diet_0", "m_diet_1",
                                                    "m_size_0", "m_size_1", "m_size_2", "sd_diet", "sd_size", "beta_hp"]
    assert mte.header(["a"], [2], ["m1_10", "m2_3"])[-3:] == ["beta_hp", "m1_10", "m2_3"]
    assert mte.log_name("/x/data.txt", 0, "", np.inf, 0) == "/x/data.log"
    assert mte.log_name("/x/data.txt", 0, "", 23.0, 8) == "/x/data23.0-8.0.log"
    assert mte.log_name("/x/data.txt", 1, "", np.inf, 8.0) == "/x/data_const_inf-8.0.log"
    assert mte.log_name("/x/data.txt", 0, "run", np.inf, 0, chain=3) == "/x/data_run__c3.log"
    assert mte.log_name("/x/data.txt", 1, "run", 23, 8, chain=0) == "/x/data_const__run_23.0-8.0_c0.log"
    assert mte.two_ln_bf(0.05, 0.05, 1000) == 0.0 and mte.two_ln_bf(0.3, 0.3, 50) == 0.0
    assert mte.two_ln_bf(1.0, 0.05, 100) == pytest.approx(2 * np.log((0.995 / 0.005) / (0.05 / 0.95)))
    assert mte.two_ln_bf(0.0, 0.05, 100) == pytest.approx(2 * np.log((0.005 / 0.995) / (0.05 / 0.95)))


def test_3_slices_from_the_flags():
    import types
    from literate_amd import mte
    A = lambda **kw: types.SimpleNamespace(**dict(dict(slices="", slice_edges="", t0=np.inf, t1=0), **kw))
    assert mte.parse_slices(A()) == [(np.inf, 0.0)]
    assert mte.parse_slices(A(t0=23.0, t1=8.0)) == [(23.0, 8.0)]
    assert mte.parse_slices(A(slices="23-8,8-0")) == [(23.0, 8.0), (8.0, 0.0)]
    assert mte.parse_slices(A(slice_edges="0,8,23,inf")) == [(np.inf, 23.0), (23.0, 8.0), (8.0, 0.0)]
    for bad in (A(slices="8-23"), A(slices="x"), A(slice_edges="5"), A(t0=3.0, t1=3.0)):
        with pytest.raises(ValueError):
            mte.parse_slices(bad)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def write_table(path, ts, te, traits, names=None):
    traits = np.asarray(traits)
    names = names or ["tr%d" % t for t in range(traits.shape[1])]
    with open(path, "w") as f:
        f.write("Species\tts\tte\t" + "\t".join(names) + "\n")
        for i in range(len(ts)):
            f.write("taxon%d\t%r\t%r\t%s\n" % (i, float(ts[i]), float(te[i]), "\t".join(repr(v) if isinstance(v, float) else str(v) for v in traits[i].tolist())))
    return str(path)


def refused(argv, match, **env):
    import MTEmodel
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with pytest.raises(SystemExit) as e:
            MTEmodel.main(argv)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert match in str(e.value), (argv, str(e.value))


def test_4_every_refusal_by_its_message(tmp_path):
    g = np.random.default_rng(3)
    n = 60
    ts, te = g.uniform(10, 30, n), np.where(g.uniform(size=n) < 0.5, g.uniform(0, 9, n), 0.0)
    ok = write_table(tmp_path / "ok.txt", ts, te, g.integers(0, 3, (n, 2)))
    run = ["-n", "10", "-s", "1"]
    refused(["-d", ok, "-A", "1"] + run, "marginal likelihoods of this model are not built")
    refused(["-d", ok] + run, "several ranks (WORLD_SIZE is 2)", WORLD_SIZE="2")
    refused(run, "-d FILE is required")
    refused(["-d", ok, "--chains", "0"] + run, "--chains and -s must be at least 1")
    refused(["-d", ok, "-pI", "1.0"] + run, "-pI takes a probability inside (0, 1)")
    refused(["-d", ok, "-bvs", "2"] + run, "-bvs, -const and -mu_species take 0 or 1")
    refused(["-d", ok, "--slices", "9-0", "--slice_edges", "9,0"] + run, "give one")
    refused(["-d", ok, "--summary", "1.0"] + run, "--summary takes a burn-in fraction in [0, 1)")
    refused(["-d", ok, "--ess", "0.5", "-n", "4", "-s", "1"], "the summary needs at least 4")
    refused(["-d", ok, "--slices", "0-9"] + run, "the older age comes first")
    refused(["-d", ok, "-traits", "3"] + run, "the table holds 2 trait columns")
    # the data
    many = np.stack([np.arange(1100) % 16, (np.arange(1100) // 16) % 16, np.arange(1100) // 256], axis=1)
    big = write_table(tmp_path / "big.txt", np.full(1100, 9.0), np.full(1100, 1.0), many)
    refused(["-d", big] + run, "1100 combinations of trait states: the sampler holds at most 1024")
    wide = write_table(tmp_path / "wide.txt", ts, te, g.integers(0, 2, (n, 17)))
    refused(["-d", wide] + run, "17 traits: the sampler holds at most 16")
    tall = write_table(tmp_path / "tall.txt", ts, te, np.stack([np.arange(n) % 17, np.arange(n) % 2], axis=1))
    refused(["-d", tall] + run, "trait tr0 has 17 states: the sampler holds at most 16 per trait")
    flat = write_table(tmp_path / "flat.txt", ts, te, np.stack([np.arange(n) % 2, np.full(n, 4)], axis=1))
    refused(["-d", flat] + run, "trait tr1 has the same state in every lineage")
    frac = write_table(tmp_path / "frac.txt", ts, te, np.stack([np.arange(n) % 2, np.where(np.arange(n) == 5, 1.5, 1.0)], axis=1))
    refused(["-d", frac] + run, "trait tr1: state 1.5 is not a non-negative integer")
    neg = write_table(tmp_path / "neg.txt", ts, te, np.stack([np.arange(n) % 2 - 1, np.arange(n) % 3], axis=1))
    refused(["-d", neg] + run, "trait tr0: state -1.0 is not a non-negative integer")
    refused(["-d", ok, "--slices", "100-50"] + run, "slice 100.0-50.0 holds no lineage")
    refused(["-d", ok, "--slices", "31-9.5"] + run, "slice 31.0-9.5 holds no extinction")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
def test_5_the_case_table_covers_what_the_device_test_needs():
    Gs = {c[1][1] for c in mr.CASES}
    assert {1, 63, 64, 65, 128, 129, 1024} <= Gs and 300 in Gs
    for G in (1, 63, 64, 65, 128, 129, 1024):
        assert {len(c[1][2]) for c in mr.CASES if c[1][1] == G} >= {1, 16}
    assert sum(mr.T16) == 128 and set(mr.T16) == {1, 2, 16}
    assert {(c[1][0], c[3]) for c in mr.CASES} == {(1, 1), (3, 5), (2, 3)}
    assert {c[2] for c in mr.CASES} == {mr.BVS, mr.NO_BVS, mr.CONSTANT} and {c[5] for c in mr.CASES} == {1, 7}
    assert all(c[4] == 300 and c[2][2] == 10 for c in mr.CASES)
    cross = {((c[1][0], c[3]), c[2], c[5]) for c in mr.CASES if c[1][1] == 65 and c[1][2] == mr.T3}
    assert len(cross) == 18
    assert len({c[0] for c in mr.CASES}) == len(mr.CASES)


@pytest.mark.parametrize("case", mr.CASES, ids=[c[0] for c in mr.CASES])
def test_5_every_gpu_case_is_held_to_the_tie_condition(case):
    D, rows, state, margin = mr.run_case(case)
    assert margin > mr.TIE, "%s: an accept decision within %g of a tie - give the case another seed" % (case[0], mr.TIE)
    st = case[2]
    prop, acc = state[:, mr.S_PROPOSED:mr.S_PROPOSED + 3], state[:, mr.S_ACCEPTED:mr.S_ACCEPTED + 3]
    assert (acc <= prop).all() and prop.sum() > 0
    if st == mr.BVS:
        assert prop[:, 2].sum() > 0 and acc[:, 2].sum() > 0, "indicator flips occur"
    if st == mr.CONSTANT:
        assert prop[:, 0].sum() == 0 and prop[:, 2].sum() == 0 and (state[:, mr.S_I:mr.S_I + D.T] == 0).all()
    if st == mr.NO_BVS:
        assert prop[:, 2].sum() == 0 and (state[:, mr.S_I:mr.S_I + D.T] == 1).all()
