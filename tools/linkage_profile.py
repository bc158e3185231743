"""The single-linkage tree of tnac4o.calculate_state_linkage (tn_state_linkage) at the shape a user runs, next to tn_pair_hist on the
same rows.

    python tools/linkage_profile.py run [OUT.json] [--M 65536] [--reps 3] [--beta 1.0] [--sweeps 32] [--host 4096]

Shape: synthetic_chimera(16, 16, seed) (256 cells of Nc = 8, 2048 spins, 32 words per row), at M and at M / 4 rows (the first M / 4 of
the same sets).  The states come from the library's own sweeps (tn_cell_sweep through relax_samples, numbers from seed=): 'beta
samples' -- M uniformly random states after `sweeps` heat-bath sweeps at `beta` --, and 'quenched' -- the same after
relax_samples(mode='quench'): many duplicates and ties.  Per set and M: one warm-up call of ops.state_linkage, then `reps` calls on the
same rows, each timed with device events around the call; reported are the median, the spread, the rounds, the distinct rows and the
largest merge height, with and without the fold.  'one pass': the same call on M copies of one row, which needs ONE round (every row's
nearest row is row 0) -- the work of a pair pass does not depend on the data, so this is one pair pass plus the empty launches of the
other rounds and the sort.  Yardstick, in the same process: tn_pair_hist (ops.pair_hist, no weights) on the same rows, which visits the
same M (M - 1) / 2 pairs of the triangle as a pair pass does.  Host baseline for scale: scipy's single linkage (or,
without scipy, the numpy Kruskal of tests/linkage_ref.py) on the first `host` rows of each set, the distance matrix by a float32 product
included.
No time here is a pass / fail condition.  Writes a JSON (default profiles/linkage_profile.json)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260024


def _opt(argv, name, default, cast):
    if name in argv:
        i = argv.index(name)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def timed(call, reps):
    """ms of `reps` calls by device events, after one warm-up call; the result of the last call."""
    import torch
    times, out = [], None
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = call()
        b.record()
        torch.cuda.synchronize()
        if rep:
            times.append(a.elapsed_time(b))
    return times, out


def _stats(times):
    import numpy as np
    return {'ms_per_call': times, 'ms_per_call_median': float(np.median(times)), 'spread_ms': float(np.ptp(times))}


def host_baseline(rows, nbits, n):
    """Seconds of single linkage of the first n rows on the host."""
    import numpy as np
    bits = np.unpackbits(np.ascontiguousarray(rows[:n]).view(np.uint8), axis=1, bitorder='little')[:, :nbits].astype(np.float32)
    t0 = time.perf_counter()
    ones = bits.sum(axis=1)
    D = np.rint(ones[:, None] + ones[None, :] - 2.0 * (bits @ bits.T)).astype(np.int64)
    t1 = time.perf_counter()
    try:
        from scipy.cluster.hierarchy import linkage
        from scipy.spatial.distance import squareform
        Z = linkage(squareform(D.astype(np.float64), checks=False), method='single')
        how, heights = 'scipy.cluster.hierarchy.linkage(method="single") on the condensed float64 distances', np.sort(Z[:, 2]).astype(np.int64)
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import linkage_ref
        how, heights = 'numpy Kruskal of tests/linkage_ref.py', linkage_ref.kruskal(D)[1]
    t2 = time.perf_counter()
    return {'rows': n, 'how': how, 's_distance_matrix': t1 - t0, 's_linkage': t2 - t1}, heights


def measure(kind, rows, nbits, reps, host):
    import numpy as np
    import torch
    from tnac4o_amd import ops
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    M = rows.shape[0]
    res = {'rows': kind, 'M': M, 'nbits': nbits, 'distinct_rows': int(np.unique(rows, axis=0).shape[0])}
    for fold in (False, True):
        times, out = timed(lambda: ops.state_linkage(d_rows, nbits, False, fold), reps)
        r = _stats(times)
        dist = out['edge_dist'].cpu().numpy()
        r.update({'rounds': int(out['rounds'][0]), 'largest_merge_height': int(dist.max()), 'edges_at_distance_0': int(np.count_nonzero(dist == 0)),
                  'median_nearest_distance': float(np.median(out['nn_dist'].cpu().numpy()))})
        r['ms_per_round'] = r['ms_per_call_median'] / r['rounds']
        res['fold' if fold else 'plain'] = r
    copies = d_rows[:1].expand(M, -1).contiguous()
    times, out = timed(lambda: ops.state_linkage(copies, nbits), reps)
    res['one_pass'] = _stats(times)
    res['one_pass']['rounds'] = int(out['rounds'][0])
    times, _ = timed(lambda: ops.pair_hist(d_rows, nbits), reps)
    res['pair_hist_same_rows'] = _stats(times)
    res['one_pass_over_pair_hist'] = res['one_pass']['ms_per_call_median'] / res['pair_hist_same_rows']['ms_per_call_median']
    for key, of in (('pairs_per_s_of_a_pass', 'one_pass'), ('pairs_per_s_of_pair_hist', 'pair_hist_same_rows')):     # both visit the triangle
        res[key] = M * (M - 1) / 2 / (res[of]['ms_per_call_median'] * 1e-3)
    if host and M >= host:
        res['host_baseline'], heights = host_baseline(rows, nbits, host)
        got = ops.state_linkage(d_rows[:host], nbits)['edge_dist'].cpu().numpy()
        res['host_baseline']['same_heights_as_the_device'] = bool(np.array_equal(np.sort(got), heights))
        times, _ = timed(lambda: ops.state_linkage(d_rows[:host], nbits), reps)
        res['host_baseline']['device_ms_same_rows'] = float(np.median(times))
    print(json.dumps(res), flush=True)
    return res


def run(out_json, M, reps, beta, sweeps, host):
    import numpy as np
    import torch
    import tnac4o_amd
    from tnac4o_amd import overlap
    from tnac4o_amd.auxx import synthetic_chimera
    assert torch.cuda.is_available(), 'linkage_profile needs a GPU'
    torch.cuda.set_device(0)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, SEED), beta=beta)
    nbits = int(overlap.active_spins(ins).size)
    qs = ins._cell_sizes()[ins.order]
    start = np.random.default_rng(SEED).integers(0, qs[None, :], size=(M, qs.size))
    ins.relax_samples(sweeps=sweeps, mode='heat_bath', beta=beta, states=start, seed=SEED)
    samples = overlap.pack_bits(overlap.spin_bits(ins))
    sample_energy = float(np.mean(ins.energy))
    ins.relax_samples(mode='quench', sweeps=None)
    quenched = overlap.pack_bits(overlap.spin_bits(ins))
    res = {'what': 'tn_state_linkage: ms per call by device events around the call (median of %d after a warm-up call), chimera 16x16 cells, Nc = 8; '
                   'beside it tn_pair_hist on the same rows and one pair pass (a call on M copies of one row: one round)' % reps,
           'beta': beta, 'heat_bath_sweeps_of_the_samples': sweeps, 'mean_energy_of_the_samples': sample_energy,
           'mean_energy_of_the_quenched': float(np.mean(ins.energy)), 'TN_LINKAGE_WGS': os.environ.get('TN_LINKAGE_WGS'), 'sets': []}
    for m in (M // 4, M):
        for kind, rows in (('beta samples', samples), ('quenched', quenched)):
            res['sets'].append(measure(kind, np.ascontiguousarray(rows[:m]), nbits, reps, host if m == M else 0))
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    argv = sys.argv[1:]
    M, reps = _opt(argv, '--M', 2 ** 16, int), _opt(argv, '--reps', 3, int)
    beta, sweeps, host = _opt(argv, '--beta', 1.0, float), _opt(argv, '--sweeps', 32, int), _opt(argv, '--host', 4096, int)
    run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'linkage_profile.json'), M, reps, beta, sweeps, host)
