"""Shared in-bin fractions other than (0, 0.5) on the host: the references tests/test_hip_shared_fractions.py compares the
kernels with agree with each other there, they tell such data from (0, 0.5) data by far more than the GPU tolerance, and
the planner does not look at the fractions."""
import ctypes as C

import numpy as np
import pytest

from helpers import edges as E
from helpers import shared_fractions as F

N, N_BINS, SEED = 3000, 24, 5
ALL = F.PAIRS + [F.CONTROL, F.OFF_GRID]


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("pair", ALL, ids=F.pair_id)
def test_gather_form_equals_the_dense_definition(pair, model):
    """The O(N) gather form the kernels are compared with (per_lineage_loglik: one birth entry, one death entry and the
    in-bin fractions per lineage) against the definition (per_lineage_loglik_dense: the overlap of every lineage with every
    bin) on random per-bin rates, 1e-12 relative: the two differ by rounding alone (~5e-16 at this size), also where a
    death sits on a window edge and for lineages with te == ts."""
    from oracle import literate_oracle as lo
    ts, te = F.lineages(N, N_BINS, pair[0], pair[1], SEED)
    stats = F.stats_of(ts, te, model)
    n_bins = len(stats["sp"])
    assert n_bins == F.window_bins(N_BINS, pair[1])
    lam, mu = F.random_rates(n_bins, 1)
    a = lo.per_lineage_loglik(ts, te, 0.0, lam, mu, model, stats["br"])
    b = lo.per_lineage_loglik_dense(ts, te, 0.0, lam, mu, model, stats["br"])
    print(pair, model, a, b, abs(a - b) / abs(b))
    assert np.isfinite(b) and abs(a - b) <= 1e-12 * abs(b), (a, b)
    # the binned form of the same likelihood (what the samplers' oracle scores) agrees as well: models 0 - 2 are sums of
    # per-bin counts and lineage-time (rounding of the br_length sums: 1e-10)
    c = lo.calc_likelihood(model, lam, mu, stats)
    assert abs(a - c) <= 1e-10 * abs(c), (a, c)


@pytest.mark.parametrize("model", [0, 1, 2])
@pytest.mark.parametrize("pair", F.PAIRS, ids=F.pair_id)
def test_the_reference_tells_the_fractions_from_the_default_ones(pair, model):
    """The same lineages at their own fractions and moved back to (0, 0.5), same rates: the reference values differ by
    more than 1e-6 relative - 1000 times the 1e-9 the GPU comparisons allow (measured: 0.9 to 78 %) - so a kernel that
    reads 0.5 for frac_death, or drops frac_birth R, cannot pass them."""
    from oracle import literate_oracle as lo
    ts, te = F.lineages(N, N_BINS, pair[0], pair[1], SEED)
    keep = te > ts                                   # (a lineage with te == ts has no (0, 0.5) counterpart)
    ts, te = ts[keep], te[keep]
    ts_c, te_c = F.control_of(ts, te)
    assert np.all(te_c > ts_c)
    assert F.fractions(ts_c, te_c)[0].max() == 0.0 and np.all(F.fractions(ts_c, te_c)[1] == 0.5)
    lam, mu = F.random_rates(N_BINS + 1, 2)
    vals = []
    for s, e in ((ts, te), (ts_c, te_c)):
        stats = F.stats_of(s, e, model)
        nb = len(stats["sp"])
        vals.append(lo.per_lineage_loglik(s, e, 0.0, lam[:nb], mu[:nb], model, stats["br"]))
    print(pair, model, vals)
    assert abs(vals[0] - vals[1]) > 1e-6 * abs(vals[1]), vals


def test_the_planner_does_not_look_at_the_fractions():
    """lr_mcmc_query_layout over the planner-map grid of models 0 and 3 at unit resolution (every chain count, both lineage
    counts, both sides of every class edge, every engine mode): the same return code and a byte-identical lr_mcmc_layout
    for every pair as for (0, 0.5).  The fractions are table contents; they must not steer the choice of kernel."""
    n = 0
    for model in (0, 3):
        for n_bins in E.class_edges(model, 0):
            for c in E.GRID_CHAINS:
                for n_lin in (4000, 1_000_000):
                    for mode in E.ENGINES.values():
                        rc0, lay0 = E.query(model, 0, True, n_bins, c, n_lin, mode, frac_birth=F.CONTROL[0], frac_death=F.CONTROL[1])
                        want = bytes(lay0)
                        assert len(want) == C.sizeof(lay0)
                        for fb, fd in F.PAIRS:
                            rc, lay = E.query(model, 0, True, n_bins, c, n_lin, mode, frac_birth=fb, frac_death=fd)
                            assert rc == rc0 and bytes(lay) == want, (model, n_bins, c, n_lin, mode, fb, fd, rc, rc0)
                            n += 1
    assert n > 1000
