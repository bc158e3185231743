"""Host reference of tn_ladder_measure / tnac4o.temper_samples(measure=) (numpy and Python integers, no GPU): include/tnpeps.h, K19.

- rows by temper_ref.to_bits; link_rows: bit l = row bit links[l][0] XOR row bit links[l][1], 0 when either entry is out of range.
- counted_pairs / measure: the pair counts by a double loop over the chains with Python's popcount, the split rule, the skip rules.
- add_hist: the 64-bit accumulation (mod 2^64); add_esums: the energy sums in the order of the kernel (ascending chain, fp64).
- schedule: the measurement rounds and their time bins, restated from the rule; walk: temper_ref.run round by round with measure applied
  at the scheduled rounds.
"""
import numpy as np

import temper_ref as tr

MAX_NBITS = 38815                                                       # the limit include/tnpeps.h states


def popcount(v):
    return bin(v).count('1')


def link_rows(rows, nbits, links):
    """Link rows as Python integers."""
    out = []
    for v in rows:
        w = 0
        for l, (p, q) in enumerate(np.asarray(links).reshape(-1, 2).tolist()):
            if 0 <= p < nbits and 0 <= q < nbits:
                w |= (((v >> p) ^ (v >> q)) & 1) << l
        out.append(w)
    return out


def counted_pairs(R, split):
    """The chain pairs a measurement counts: split = 0 every ca < cb, else ca < split <= cb."""
    return [(ca, cb) for ca in range(R) for cb in range(ca + 1, R) if split == 0 or ca < split <= cb]


def pair_counts(rows, nbins, slot, M, split):
    """(T, nbins) Python integers (object array): for every temperature the histogram of popcount(row_a XOR row_b) over the counted chain
    pairs; a slot entry outside [0, M) takes its pairs out."""
    slot = np.asarray(slot)
    R, T = slot.shape
    h = np.zeros((T, nbins), dtype=object)
    for t in range(T):
        for ca, cb in counted_pairs(R, split):
            a, b = int(slot[ca, t]), int(slot[cb, t])
            if 0 <= a < M and 0 <= b < M:
                h[t, popcount(rows[a] ^ rows[b])] += 1
    return h


def measure(cells, states, slot, nbits, bitcell, links=None, split=0):
    """One measurement: (spin (T, nbits + 1), link (T, nlinks + 1) or None) increments as Python integers."""
    states = np.asarray(states)
    M = states.shape[0]
    rows = tr.to_bits(cells, states, nbits, np.asarray(bitcell).reshape(-1, 2))
    spin = pair_counts(rows, nbits + 1, slot, M, split)
    if links is None:
        return spin, None
    nlinks = np.asarray(links).reshape(-1, 2).shape[0]
    return spin, pair_counts(link_rows(rows, nbits, links), nlinks + 1, slot, M, split)


def add_hist(acc, inc):
    """acc + inc mod 2^64, as uint64 (acc: any integer array read as unsigned 64-bit; inc: Python integers)."""
    a = np.ascontiguousarray(acc).astype(np.int64, copy=False).view(np.uint64).astype(object)
    return np.array([(int(x) + int(y)) % (1 << 64) for x, y in zip(a.ravel(), np.asarray(inc, dtype=object).ravel())], dtype=np.uint64).reshape(a.shape)


def add_esums(acc, slot, energy, M):
    """esums after one measurement: per temperature s1 = sum E, s2 = sum E * E over the chains in ascending order from 0.0 (fp64, product
    rounded before the addition), then acc[t] += (1, s1, s2)."""
    slot = np.asarray(slot)
    R, T = slot.shape
    out = np.array(acc, dtype=np.float64).reshape(T, 3).copy()
    E = np.asarray(energy, dtype=np.float64)
    for t in range(T):
        s1, s2 = np.float64(0.0), np.float64(0.0)
        for c in range(R):
            s = int(slot[c, t])
            if 0 <= s < M:
                e = E[s]
                s1 = s1 + e
                s2 = s2 + e * e
        out[t, 0] = out[t, 0] + np.float64(1.0)
        out[t, 1] = out[t, 1] + s1
        out[t, 2] = out[t, 2] + s2
    return out


def schedule(rounds, measure_every, measure_from=0, measure_bins=16):
    """[(round, bin)] of every measurement, round by round from the rule: a measurement follows round r iff r >= measure_from and
    (r - measure_from + 1) % measure_every == 0; measurement i of n goes to bin i B // n, B = min(measure_bins, n)."""
    after = [r for r in range(rounds) if r >= measure_from and (r - measure_from + 1) % measure_every == 0]
    n = len(after)
    B = min(measure_bins, n)
    return [(r, i * B // n) for i, r in enumerate(after)], B


def walk(cells, Nx, Ny, states, betas, rounds, sweeps, usweep, bits, cluster_from, cpairs, ucl, uswap, nbits, bitcell, links, split, plan, B):
    """temper_ref.run one round at a time from a fresh assignment, measure applied behind the rounds of plan = [(round, bin)]: (the final
    result of run, spin (B, T, nbits + 1) uint64, link or None, esums (B, T, 3))."""
    M, T = states.shape[0], len(betas)
    tidx, slot = tr.fresh_assignment(M, T)
    s = dict(states=states, tidx=tidx, slot=slot, accepted=None, attempted=None)
    spin = np.zeros((B, T, nbits + 1), dtype=np.uint64)
    link = None if links is None else np.zeros((B, T, np.asarray(links).reshape(-1, 2).shape[0] + 1), dtype=np.uint64)
    esums = np.zeros((B, T, 3))
    due = dict(plan)
    for r in range(rounds):
        s = tr.run(cells, Nx, Ny, s['states'], betas, s['tidx'], s['slot'], r, 1, sweeps, None if usweep is None else usweep[r:r + 1], bits, cluster_from,
                   None if cpairs is None else cpairs[r:r + 1], None if ucl is None else ucl[r:r + 1], uswap[r:r + 1], s['accepted'], s['attempted'])
        if r in due:
            b = due[r]
            hs, hl = measure(cells, s['states'], s['slot'], nbits, bitcell, links, split)
            spin[b] = add_hist(spin[b], hs)
            if links is not None:
                link[b] = add_hist(link[b], hl)
            esums[b] = add_esums(esums[b], s['slot'], s['energy'], M)
    return s, spin, link, esums
