"""Unit-resolution data whose shared in-bin fractions are NOT (0, 0.5).

Year-resolution births with one death_jitter added to every death give every lineage the same pair
    frac_birth = ts - floor(ts),   frac_death = te - (ceil(te) - 1),
which ChainEngine derives from the data and every kernel family folds into its lookup tables (csrc/lr_device.h: lr_put_S
writes v + frac_birth R, lr_put_E writes v - frac_death R).  The rest of the suite runs (0, 0.5) only - the default
death_jitter on integer births - where the birth-side slope vanishes and a hard-coded 0.5 cannot be told from the field.
The cases here move the same integer-year lineages by other pairs, all exactly representable, so the engine still finds
one shared pair: death_jitter 0.25 / 0.75, births off the year, and frac_death == 1.0 - death_jitter 0 or 1, integer
deaths: a death sits ON a window edge, a lineage that dies in its birth year has te == ts and its death entry is the bin
BEFORE its birth bin (entry 0 when born in the first bin), and the window's last bin is a whole one that holds the extant
lineages.  One jitter off the binary grid (0.1) makes the fractions differ by ulps between years: the engine must fall
back to general times by itself."""
import functools

import numpy as np

from helpers import edges as E

PAIRS = [(0.0, 0.25), (0.0, 0.75), (0.0, 1.0), (0.25, 0.5), (0.5, 0.75), (0.75, 1.0)]
CONTROL = (0.0, 0.5)
OFF_GRID = (0.0, 0.1)
REDUCED = [(0.0, 0.25), (0.25, 1.0)]        # the pairs of the larger shapes: a death fraction alone, both with integer deaths


def pair_id(pair):
    return "fb%g-fd%g" % pair


def window_bins(n_bins, fd):
    """Bins of the window of lineages(n, n_bins, fb, fd, seed): integer deaths (fd == 1.0) end ON the last edge, so the last
    bin is a whole one; any other fraction leaves a partial bin, which the CLI drops."""
    return n_bins + 1 if fd == 1.0 else n_bins


def fractions(ts, te):
    """The in-bin fractions as ChainEngine takes them."""
    return ts - np.floor(ts), te - (np.ceil(te) - 1.0)


@functools.lru_cache(maxsize=None)
def lineages(n, n_bins, fb, fd, seed):
    """n synthetic lineages on integer years [0, n_bins] plus the placed ones of tests/test_hip_edges.py
    (helpers/edges.py: placed_lineages - the first of them pins the window from the first possible birth to the last
    possible death), every birth moved by fb and every death by fd.  fd == 1.0 adds a lineage born in the window's last
    bin, and with fb == 0 zero-length lineages (te == ts) in the first, the second, an interior and the last bin."""
    from literate_amd import synth
    n_bins = int(n_bins)
    s, k, _ = synth.make_lineages(n, n_bins=n_bins, n_shifts=3, seed=seed, jitter=0.0)
    assert np.all(s == np.floor(s)) and np.all(k == np.floor(k)) and np.all(k >= s)
    extra = E.placed_lineages(n_bins, np.random.default_rng(seed))
    if fd == 1.0:
        extra += [(n_bins, n_bins)]                                        # born in the last bin, extant
        if fb == 0.0:
            extra += [(b, b - 1) for b in (0, 1, n_bins // 3, n_bins)]     # te == ts
    ts = np.concatenate([s, [float(a) for a, _ in extra]]) + fb
    te = np.concatenate([k, [float(b) for _, b in extra]]) + fd
    assert ts.min() == fb and te.max() == n_bins + fd and np.all(te >= ts)
    assert int(te.max()) - int(ts.min()) == window_bins(n_bins, fd)
    fs, fe = fractions(ts, te)
    if (fb, fd) == OFF_GRID:
        assert np.all(fs == fb) and np.ptp(fe) > 0.0 and np.allclose(fe, fd, rtol=0.0, atol=1e-12)
    else:
        assert np.all(fs == fb) and np.all(fe == fd)
        if (fb, fd) == (0.0, 1.0):
            assert np.count_nonzero(te == ts) == 4
    return ts, te


def control_of(ts, te):
    """The same lineages moved back to (0, 0.5): integer births, deaths half a year after their death year."""
    return np.floor(ts), np.ceil(te) - 1.0 + 0.5


def stats_of(ts, te, model):
    """The oracle's own binning of the data: dict(sp, ex, br[, ex_dead, br_dead])."""
    from oracle import literate_oracle as lo
    t0, sp, ex, br = lo.bin_events_cli(ts, te)
    assert t0 == 0
    stats = dict(sp=sp, ex=ex, br=br)
    if model == 3:
        stats["ex_dead"], stats["br_dead"] = lo.bin_events_dead(ts, te, te.max())
    return stats


def random_rates(n_bins, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 0.5, n_bins), rng.uniform(0.1, 0.5, n_bins)
