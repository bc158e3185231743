"""Host side of temper_samples(measure=): overlap histograms at every temperature of a tempering ladder, accumulated on the device by
the library's tn_ladder_measure (csrc/ladder.hip) between the blocks of rounds of tn_temper.

The schedule, every argument check, the link table, the moments and the time-bin jackknife are plain numpy and run without a GPU; the
only device work is ops.ladder_measure, which temper.temper_native calls after every measurement round."""
import numpy as np

from . import overlap
from .overlap import active_spins, link_pairs

MAX_NBITS = 38815                # largest row / link row tn_ladder_measure takes: 4 bytes per bin and the staging in 160 KiB of LDS (include/tnpeps.h)
MAX_CHAINS = 65536               # chains per temperature: their pairs stay below 2^32
PAIRS = ('all', 'halves')
MOMENT_KEYS = ('q', 'abs_q', 'q2', 'q4', 'binder', 'chi_sg', 'ql')


# ---------------------------------------------------------------------------------------------- schedule
def _integer(v, name, lo):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo:
        raise ValueError('%s must be an integer >= %d' % (name, lo))
    return int(v)


def schedule(rounds, measure, measure_from=0, measure_bins=16):
    """(after, bins, B): `after` (n_meas,) = the global rounds a measurement follows -- round r iff r >= measure_from and
    (r - measure_from + 1) % measure == 0 --, bins (n_meas,) = the time bin of measurement i, i B // n_meas, and B = min(measure_bins,
    n_meas).  ValueError: measure or measure_bins not a positive integer, measure_from outside [0, rounds], no measurement at all."""
    measure, measure_bins = _integer(measure, 'measure', 1), _integer(measure_bins, 'measure_bins', 1)
    measure_from = _integer(measure_from, 'measure_from', 0)
    if measure_from > rounds:
        raise ValueError('measure_from = %d lies outside [0, rounds = %d]' % (measure_from, rounds))
    n_meas = (rounds - measure_from) // measure
    if n_meas < 1:
        raise ValueError('no measurement: rounds = %d, measure_from = %d, measure = %d' % (rounds, measure_from, measure))
    B = min(measure_bins, n_meas)
    i = np.arange(n_meas, dtype=np.int64)
    return measure_from + (i + 1) * measure - 1, i * B // n_meas, B


def block_ends(rounds, per, after):
    """The ends of the blocks of rounds of temper_native: every multiple of `per` counted from the previous end, cut so that a block ends
    behind every round of `after` (None: no measurement).  rounds = 0: one empty block."""
    stops = set() if after is None else set(int(r) + 1 for r in after)
    ends, lo = [], 0
    while lo < rounds:
        hi = min(lo + per, rounds)
        inner = [s for s in stops if lo < s < hi]
        if inner:
            hi = min(inner)
        ends.append(hi)
        lo = hi
    return ends or [0]


# ---------------------------------------------------------------------------------------------- arguments
def pairs_in_halves(rounds, R):
    """Chain pairings for cluster moves that stay inside the two halves [0, R // 2) and [R // 2, R) of measure_pairs='halves': per round
    a random perfect matching of each half (one chain of an odd half stays out), from numpy's global generator.  (rounds, Pc, 2) int32."""
    rounds, R = _integer(rounds, 'rounds', 0), _integer(R, 'R', 2)
    h = R // 2
    out = []
    for _ in range(rounds):
        lo, hi = np.random.permutation(h), h + np.random.permutation(R - h)
        out.append(np.concatenate([lo[:2 * (h // 2)].reshape(-1, 2), hi[:2 * ((R - h) // 2)].reshape(-1, 2)]))
    Pc = h // 2 + (R - h) // 2
    return np.array(out, dtype=np.int32).reshape(rounds, Pc, 2)


def link_table(solver):
    """(nlinks, 2) int32: overlap.link_pairs of the model as row positions (the active spin's index, bit_tables' order); -1 for a spin no
    cell lists, which the device reads as link bit 0."""
    act = active_spins(solver)
    pairs = link_pairs(solver.J0)
    pos = np.searchsorted(act, pairs)
    ok = (pos < act.size) & (act[np.minimum(pos, max(act.size - 1, 0))] == pairs) if act.size else np.zeros(pairs.shape, dtype=bool)
    return np.where(ok, pos, -1).astype(np.int32).reshape(-1, 2)


def check_arguments(solver, a, measure, measure_from, measure_bins, measure_pairs, measure_links):
    """Everything measure= can refuse before any device work; a: what temper.check_arguments returned.  Returns a dict: after, bins, B,
    n_meas, split, links (bool)."""
    after, bins, B = schedule(a['rounds'], measure, measure_from, measure_bins)
    if solver.mode != 'Ising':
        raise ValueError("measure= is defined for mode 'Ising' only")
    if measure_pairs not in PAIRS:
        raise ValueError("measure_pairs must be 'all' or 'halves'")
    R = a['R']
    if R < 2:
        raise ValueError('measure= needs at least two chains (M >= 2 len(betas))')
    if R > MAX_CHAINS:
        raise NotImplementedError('%d chains per temperature; tn_ladder_measure takes at most %d; there is no host fallback' % (R, MAX_CHAINS))
    n = int(active_spins(solver).size)
    if n < 1:
        raise ValueError('the model has no active spin')
    if n > MAX_NBITS:
        raise NotImplementedError('the model has %d active spins; tn_ladder_measure takes at most %d (its histogram must fit the 160 KiB of '
                                  'LDS); there is no host fallback' % (n, MAX_NBITS))
    links = bool(measure_links)
    if links:
        nl = int(link_pairs(solver.J0).shape[0])
        if nl > MAX_NBITS:
            raise NotImplementedError('the model has %d couplings; tn_ladder_measure takes at most %d (its histogram must fit the 160 KiB of '
                                      'LDS); there is no host fallback (measure_links=False leaves the link overlap out)' % (nl, MAX_NBITS))
    split = 0
    if measure_pairs == 'halves':
        split = R // 2
        p = np.asarray(a['pairs'])
        if a['cluster'] and p.size and a['cluster_from'] < a['T'] and np.any((p[..., 0] < split) != (p[..., 1] < split)):
            raise ValueError("measure_pairs='halves' with cluster moves needs pairs= that stay inside the halves [0, R // 2) and [R // 2, R) "
                             '(ladder.pairs_in_halves draws such pairings)')
    return dict(after=after, bins=bins, B=B, n_meas=int(after.size), split=split, links=links)


# ---------------------------------------------------------------------------------------------- estimates
def moments_of(spin_hist, link_hist):
    """The moments of one (T, n + 1) spin histogram and (None or) one (T, n_l + 1) link histogram: a dict of (T,) arrays over MOMENT_KEYS,
    conventions of overlap.moments; chi_sg = n <q^2>, ql = the mean link overlap (NaN without links); NaN where no pair was counted."""
    spin_hist = np.asarray(spin_hist, dtype=np.float64)
    T, n = spin_hist.shape[0], spin_hist.shape[1] - 1
    out = {k: np.full(T, np.nan) for k in MOMENT_KEYS}
    values = overlap.overlap_values('spin', n)
    for t in range(T):
        tot = spin_hist[t].sum()
        if tot > 0:
            m = overlap.moments(values, spin_hist[t] / tot)
            m['chi_sg'] = n * m['q2']
            for k, v in m.items():
                out[k][t] = v
    if link_hist is not None:
        link_hist = np.asarray(link_hist, dtype=np.float64)
        lvalues = overlap.overlap_values('link', link_hist.shape[1] - 1) if link_hist.shape[1] > 1 else np.ones(1)
        for t in range(T):
            tot = link_hist[t].sum()
            if tot > 0:
                out['ql'][t] = float((link_hist[t] / tot) @ lvalues)
    return out


def energy_of(esums, R, betas, N):
    """(<E> (T,), heat capacity (T,)) of (T, 3) sums (measurements, sum E, sum E^2) over R rows per measurement:
    c = beta^2 (<E^2> - <E>^2) / N.  NaN without a measurement."""
    esums = np.asarray(esums, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        cnt = esums[:, 0] * R
        e1, e2 = esums[:, 1] / cnt, esums[:, 2] / cnt
        return e1, np.asarray(betas, dtype=np.float64) ** 2 * (e2 - e1 * e1) / N


def jackknife(parts, estimate):
    """Delete-one-bin jackknife: parts (B, ...) are additive over the bins; estimate(total) returns an array or a dict of arrays.  The
    error is sqrt((B - 1) / B sum_b (theta_(b) - mean theta_(.))^2) with theta_(b) = estimate(total - parts[b]); NaN when B < 2.  It
    assumes bins longer than the autocorrelation time."""
    parts = np.asarray(parts)
    B = parts.shape[0]
    total = parts.sum(axis=0)
    full = estimate(total)
    as_dict = isinstance(full, dict)
    keys = list(full) if as_dict else [None]
    if B < 2:
        err = {k: np.full(np.shape(full[k] if as_dict else full), np.nan) for k in keys}
    else:
        th = [estimate(total - parts[b]) for b in range(B)]
        err = {}
        for k in keys:
            x = np.array([t[k] if as_dict else t for t in th], dtype=np.float64)
            err[k] = np.sqrt((B - 1) / B * np.sum((x - x.mean(axis=0)) ** 2, axis=0))
    return err if as_dict else err[None]


def store(solver, spin_hist, link_hist, esums, n_meas, R, betas):
    """The stored results of temper_samples(measure=) (documented there) from the accumulators (B, T, n + 1) int64, (B, T, n_l + 1) int64 or
    None, (B, T, 3) float64."""
    spin_hist = np.asarray(spin_hist, dtype=np.int64)
    n = spin_hist.shape[2] - 1
    solver.temper_measurements = int(n_meas)
    solver.temper_overlap_hist = spin_hist
    solver.temper_overlap_values = overlap.overlap_values('spin', n)
    tot = spin_hist.sum(axis=0).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        solver.temper_overlap_P = tot / tot.sum(axis=1, keepdims=True)
    if link_hist is not None:
        link_hist = np.asarray(link_hist, dtype=np.int64)
        nl = link_hist.shape[2] - 1
        solver.temper_link_hist = link_hist
        solver.temper_link_values = overlap.overlap_values('link', nl) if nl > 0 else np.ones(1)
        ltot = link_hist.sum(axis=0).astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            solver.temper_link_P = ltot / ltot.sum(axis=1, keepdims=True)
    else:
        solver.temper_link_hist = solver.temper_link_values = solver.temper_link_P = None
    B, T = spin_hist.shape[:2]
    # both histograms side by side, so that one jackknife deletes a bin of both
    both = spin_hist if link_hist is None else np.concatenate([spin_hist, link_hist], axis=2)

    def est(h):
        return moments_of(h[:, :n + 1], None if link_hist is None else h[:, n + 1:])

    solver.temper_overlap_moments = est(both.sum(axis=0))
    solver.temper_overlap_errors = jackknife(both, est)
    esums = np.asarray(esums, dtype=np.float64)
    solver.temper_energy_sums = esums
    solver.temper_energy_mean, solver.temper_heat_capacity = energy_of(esums.sum(axis=0), R, betas, n)
    err = jackknife(esums, lambda s: np.stack(energy_of(s, R, betas, n)))
    solver.temper_energy_mean_error, solver.temper_heat_capacity_error = err[0], err[1]
