"""One measurement of tn_ladder_measure (tnac4o.temper_samples(measure=)) at the shape a user runs, next to the same histograms composed
of the entry points that existed before it, and next to one round of tn_temper.

    python tools/ladder_profile.py [OUT.json] [--reps 3]

Instance: synthetic_chimera(16, 16, seed) (256 cells of Nc = 8, 2048 spins), T = 32 temperatures, R = 64 chains (M = 2048 rows),
uniformly random states, slot with the labels of every chain permuted, link overlap on.  Every figure is the median of `reps` timed runs
after one warm-up run, device events around the whole run (host work between the launches included):
  (a) measure       one call of tn_ladder_measure: conversion of the states, link rows, both histograms, energy sums.
  (b) composition   the same two histograms from tn_pair_hist: per temperature a gather of its R packed rows (index_select through slot),
                    one call with unit weights, and an add of the low limbs into the accumulator; the same for the link rows: 2 T
                    calls.  The packed rows and link rows are made on the host beforehand and are NOT part of the time (nothing before
                    tn_ladder_measure converts states on the device outside tn_temper), and there are no energy sums: (b) does less
                    than (a).  The two results must be equal; the run fails otherwise.
  (c) round         one round of tn_temper with sweeps = 1 and cluster moves at every temperature (R / 2 pairs).
a / b and a / c are recorded; no number here is a pass / fail condition.  Writes a JSON (default profiles/ladder_profile.json)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260027
T, R = 32, 64


def timed(fn, reps):
    """[ms] of `reps` runs of fn() after one warm-up run, device events around each."""
    import torch
    out = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep:
            out.append(a.elapsed_time(b))
    return out


def stats(ms):
    import numpy as np
    return {'ms': ms, 'ms_median': float(np.median(ms)), 'spread_ms': float(np.ptp(ms))}


def main(argv):
    import numpy as np
    import torch
    import tnac4o_amd
    from tnac4o_amd import exchange, ladder, ops, overlap, relax, temper
    from tnac4o_amd.auxx import synthetic_chimera
    reps = 3
    if '--reps' in argv:
        i = argv.index('--reps')
        reps = int(argv[i + 1])
        del argv[i:i + 2]
    out_path = argv[0] if argv else os.path.join(ROOT, 'profiles', 'ladder_profile.json')
    dev = torch.device('cuda', 0)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, SEED), beta=1.0)
    Nx, Ny, ncell, M = ins.Nx, ins.Ny, ins.Nx * ins.Ny, T * R
    rng = np.random.default_rng(SEED)
    states = rng.integers(0, 256, (M, ncell)).astype(np.int16)           # lattice order of the solver's rotation
    slot = np.array([c * T + rng.permutation(T) for c in range(R)], dtype=np.int32)
    tidx = np.empty(M, dtype=np.int32)
    tidx[slot.ravel()] = np.tile(np.arange(T, dtype=np.int32), R)
    nbits, cellbits, bitcell = temper.bit_tables(ins)
    rowptr, cols = exchange.coupling_csr(ins)
    links = ladder.link_table(ins)
    nlinks = int(links.shape[0])
    table = relax.EnergyCells(ins, dev)
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x)).to(dev)      # noqa: E731
    d_st, d_slot, d_tidx, d_bc, d_links = up(states), up(slot), up(tidx), up(bitcell.astype(np.int32)), up(links)
    bits = (nbits, up(cellbits.astype(np.int32)), d_bc, up(np.asarray(rowptr, dtype=np.int32)), up(np.asarray(cols, dtype=np.int32)))
    betas = np.linspace(0.1, 1.6, T)
    res = {'what': 'tn_ladder_measure against T gathers + 2 T calls of tn_pair_hist, and against one round of tn_temper; chimera 16x16 cells, Nc = 8, '
                   'T = %d, R = %d, links on; device events around each run, median of %d after a warm-up' % (T, R, reps),
           'T': T, 'R': R, 'M': M, 'nbits': int(nbits), 'nlinks': nlinks, 'reps': reps}

    # (c) one round of tn_temper on a copy of the states; its energy_out feeds the measurement
    u = dict(usweep=up(rng.random((1, 1, ncell, M))), ucl=up(rng.random((1, T, R // 2))), uswap=up(rng.random((1, R, T - 1))),
             cpairs=up(rng.permutation(R).reshape(1, R // 2, 2).astype(np.int32)))
    acc, att = torch.zeros(T - 1, dtype=torch.int32, device=dev), torch.zeros(T - 1, dtype=torch.int32, device=dev)
    last = {}

    def round_():
        st, ti, sl = d_st.clone(), d_tidx.clone(), d_slot.clone()
        last['out'] = ops.temper(table.cells, Nx, Ny, betas, st, ti, sl, 0, 1, 1, usweep=u['usweep'], bits=bits, cluster_from=0, cpairs=u['cpairs'],
                                 ucl=u['ucl'], uswap=u['uswap'], accepted=acc, attempted=att)

    res['round'] = stats(timed(round_, reps))
    energy = ops.temper(table.cells, Nx, Ny, betas, d_st.clone(), d_tidx.clone(), d_slot.clone(), 0, 0, 0, accepted=acc, attempted=att,
                        uswap=torch.zeros((0, R, T - 1), dtype=torch.float64, device=dev))['energy']      # no round: the energies of the states

    # (a) one measurement
    d_sh = torch.zeros((T, nbits + 1), dtype=torch.int64, device=dev)
    d_lh = torch.zeros((T, nlinks + 1), dtype=torch.int64, device=dev)
    d_es = torch.zeros((T, 3), dtype=torch.float64, device=dev)

    def measure():
        ops.ladder_measure(table.cells, Nx, Ny, d_st, d_slot, nbits, d_bc, d_sh, d_links, d_lh, 0, energy, d_es)

    measure()
    torch.cuda.synchronize()
    one_s, one_l = d_sh.cpu().numpy().copy(), d_lh.cpu().numpy().copy()
    res['measure'] = stats(timed(measure, reps))

    # (b) the composition; rows and link rows packed on the host, outside the time
    sb = 1 - ((states.astype(np.int64)[:, bitcell[:, 0]] >> bitcell[:, 1]) & 1)
    lb = np.where((links >= 0).all(axis=1), sb[:, np.maximum(links[:, 0], 0)] ^ sb[:, np.maximum(links[:, 1], 0)], 0)
    d_rows, d_lrows = up(overlap.pack_bits(sb).view(np.int64)), up(overlap.pack_bits(lb).view(np.int64))
    c_sh, c_lh = torch.zeros_like(d_sh), torch.zeros_like(d_lh)
    d_slot64 = d_slot.to(torch.int64)

    def composed():
        for t in range(T):
            idx = d_slot64[:, t]
            c_sh[t] += ops.pair_hist(d_rows.index_select(0, idx), nbits)[:, 0]
            c_lh[t] += ops.pair_hist(d_lrows.index_select(0, idx), nlinks)[:, 0]

    composed()
    torch.cuda.synchronize()
    same = bool(np.array_equal(c_sh.cpu().numpy(), one_s) and np.array_equal(c_lh.cpu().numpy(), one_l))
    res['equal'] = same
    res['pairs_per_temperature'] = int(one_s[0].sum())
    if not same or res['pairs_per_temperature'] != R * (R - 1) // 2:
        raise SystemExit('tn_ladder_measure and the composition of tn_pair_hist disagree')
    res['composition'] = stats(timed(composed, reps))
    a, b, c = res['measure']['ms_median'], res['composition']['ms_median'], res['round']['ms_median']
    res['a_over_b'], res['a_over_c'] = a / b, a / c
    res['device'] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps({k: res[k] for k in ('a_over_b', 'a_over_c', 'equal')}), 'measure %.3f ms, composition %.3f ms, round %.3f ms' % (a, b, c))
    del table


if __name__ == '__main__':
    main(sys.argv[1:])
