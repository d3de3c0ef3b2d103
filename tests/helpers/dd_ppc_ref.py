"""Numpy restatement of literate_amd/ppc.py's posterior_predictive_dd: steps 1 - 5 of that module's docstring on
tests/helpers/dd_sim_ref.py, the restated diversity-dependent simulator.

Steps 2 - 4 are tests/helpers/ppc_ref.check itself, not a copy.  check() hands its simulator two [n, n_bins] arrays that it
only slices (bins b0 on for the free-running set, one bin per replicate (b - b0) * R + i for the one-step set) and never
reads, so they can carry what a diversity-dependent replicate needs in the place of rates: x, the TIME_RANGE value of each
bin, where lam_bins goes, and i, the draw's number, where mu_bins goes.  The simulator below looks the draw's parameters up
by that number.  It also collects the smallest distance between a draw and a threshold over all replicates."""
import numpy as np

from helpers import dd_sim_ref, ppc_ref


def dd_simulator(params, m_birth, m_death, closest):
    """ppc_ref.check's simulator over the draws' parameters [R, 8]; appends every replicate's closest distance to `closest`"""
    def sim(x, draw, spb, n_start, seed, capacity):
        x, draw = np.asarray(x, dtype=float), np.asarray(draw)
        par = params[draw[:, 0].astype(np.int64)]
        counts, totals, d = dd_sim_ref.simulate(par, x, spb, np.asarray(n_start), seed, m_birth, m_death, capacity)
        closest.extend(d.tolist())
        return counts, totals
    return sim


def check(params, sp, ex, time_range, m_birth, m_death, steps_per_bin, seed, start_bin=None, capacity=None, start_time=0.0):
    """steps 2 - 4 under the draws' parameters [R, 8] -> ppc_ref.check's dict + closest (the smallest distance between a
    draw and a threshold over every replicate of both sets)"""
    params = np.asarray(params, dtype=float)
    R, n_bins = len(params), len(sp)
    x = np.tile(np.asarray(time_range, dtype=float), (R, 1))
    draw = np.tile(np.arange(R, dtype=float)[:, None], (1, n_bins))
    closest = []
    out = ppc_ref.check(x, draw, sp, ex, steps_per_bin, seed, dd_simulator(params, m_birth, m_death, closest), start_bin,
                        capacity, start_time)
    out["closest"] = min(closest)
    return out


def posterior_predictive_dd(rows, sp, ex, time_range, m_birth, m_death, n_draws, steps_per_bin, seed, start_bin=None,
                            capacity=None, start_time=0.0):
    """steps 1 - 4 on trace rows [S', C, W] (host): a draw's parameters are columns 4:12 of its row"""
    rows = np.asarray(rows, dtype=float)
    flat = rows.reshape(-1, rows.shape[-1])
    idx = ppc_ref.draw_indices(len(flat), n_draws)
    out = check(flat[idx][:, 4:12], sp, ex, time_range, m_birth, m_death, steps_per_bin, seed, start_bin, capacity, start_time)
    out.update(draw_rows=idx, params=flat[idx][:, 4:12])
    return out
