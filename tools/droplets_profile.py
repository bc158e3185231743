"""The droplet decomposition of tnac4o.calculate_droplets (tn_droplets) at the shape a user runs, next to one round of
tn_cluster_exchange over the same rows and the same arcs.

    python tools/droplets_profile.py run [OUT.json] [--M 65536] [--reps 5] [--beta 1.0] [--sweeps 32] [--K 64]

Shape: synthetic_chimera(16, 16, seed) (256 cells of Nc = 8, 2048 spins), M rows.  The states come from the library's own sweeps
(tn_cell_sweep through relax_samples, numbers from seed=): 'beta samples' -- M uniformly random states after `sweeps` heat-bath sweeps at
`beta` --; the reference is the lowest state among their quenches; 'quenched' -- M copies of the reference after two heat-bath sweeps at
`beta`, quenched until nothing moves: local minima next to the reference, few and small droplets.  Per set: one warm-up call of
ops.droplets, then `reps` calls on the same rows, each timed with device events around the call; reported are the median, the spread,
droplets per row, differing spins, the largest droplet and the rows with more than K droplets; the same with labels=True (the call then
also writes M x 2048 int32).  Yardstick, in the same run: one round of tn_cluster_exchange over the M / 2 pairs (2k, 2k + 1) of the
same rows (fresh copies: the round moves them), which grows ONE cluster per pair along the same arcs.
No time here is a pass / fail condition.  Writes a JSON (default profiles/droplets_profile.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260023


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


def measure(kind, rows, graph, d_ref, nbits, K, reps):
    import numpy as np
    import torch
    from tnac4o_amd import ops
    d_rowptr, d_cols, d_vals, d_field = graph
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    M = rows.shape[0]
    res = {'rows': kind, 'M': M, 'nbits': nbits, 'nnz': int(d_cols.numel()), 'K': K}
    for labels in (False, True):
        times, out = timed(lambda: ops.droplets(d_rows, nbits, d_ref, d_rowptr, d_cols, d_vals, d_field, K, None, labels), reps)
        key = 'with_labels' if labels else 'droplets'
        res[key] = {'ms_per_call': times, 'ms_per_call_median': float(np.median(times)), 'spread_ms': float(np.ptp(times)),
                    'rows_per_s': M / (float(np.median(times)) * 1e-3)}
        if not labels:
            count, hist = out['count'].double(), out['size_hist'].cpu().numpy()
            res.update({'mean_droplets_per_row': float(count.mean().item()), 'most_droplets_in_a_row': int(count.max().item()),
                        'mean_differing_spins': float(out['diff'].double().mean().item()), 'largest_droplet': int(out['largest'].max().item()),
                        'rows_with_more_than_K': int((out['count'] > K).sum().item()), 'droplets_of_one_spin': int(hist[1]),
                        'droplets_in_all': int(hist.sum()), 'mean_excitation_energy': float(out['de_total'].mean().item())})
    d_pairs = torch.arange(M, dtype=torch.int32, device='cuda').reshape(-1, 2)
    d_u = torch.as_tensor(np.random.default_rng(SEED).random(M // 2)).cuda()
    times, out = timed(lambda: ops.cluster_exchange(d_rows.clone(), nbits, d_rowptr, d_cols, d_pairs, d_u), reps)
    clone_ms, _ = timed(lambda: d_rows.clone(), reps)
    res['cluster_exchange_round_same_rows'] = {'pairs': M // 2, 'ms_per_round_with_the_copy': times, 'ms_per_round_median_with_the_copy': float(np.median(times)),
                                               'ms_of_the_copy_median': float(np.median(clone_ms)), 'mean_cluster_size': float(out[0].double().mean().item()),
                                               'mean_differing_spins': float(out[1].double().mean().item())}
    print(json.dumps(res), flush=True)
    return res


def run(out_json, M, reps, beta, sweeps, K):
    import numpy as np
    import torch
    import tnac4o_amd
    from tnac4o_amd import exchange, overlap
    from tnac4o_amd.auxx import synthetic_chimera
    assert torch.cuda.is_available(), 'droplets_profile needs a GPU'
    torch.cuda.set_device(0)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, SEED), beta=beta)
    nbits = int(overlap.active_spins(ins).size)
    graph = tuple(torch.as_tensor(a).cuda() for a in exchange.weighted_coupling_csr(ins))
    qs = ins._cell_sizes()[ins.order]
    start = np.random.default_rng(SEED).integers(0, qs[None, :], size=(M, qs.size))
    ins.relax_samples(sweeps=sweeps, mode='heat_bath', beta=beta, states=start, seed=SEED)
    samples = overlap.pack_bits(overlap.spin_bits(ins))
    sample_energy = float(np.mean(ins.energy))
    ins.relax_samples(mode='quench', sweeps=None)
    lowest = int(np.argmin(ins.energy))
    e_ref = float(ins.energy[lowest])
    ref_state = np.asarray(ins.states)[lowest].astype(np.int64) & (0xff if np.asarray(ins.states).dtype.itemsize == 1 else -1)
    d_ref = torch.as_tensor(overlap.pack_bits(overlap.spin_bits(ins)[lowest:lowest + 1])[0].view(np.int64)).cuda()
    ins.relax_samples(sweeps=2, mode='heat_bath', beta=beta, states=np.repeat(ref_state[None, :], M, axis=0), seed=SEED + 1)
    ins.relax_samples(mode='quench', sweeps=None)
    quenched = overlap.pack_bits(overlap.spin_bits(ins))
    res = {'what': 'tn_droplets: ms per call by device events around the call (median of %d after a warm-up call), chimera 16x16 cells, Nc = 8, M rows, '
                   'K = %d slots; beside it one round of tn_cluster_exchange over the pairs (2k, 2k + 1) of the same rows' % (reps, K),
           'beta': beta, 'heat_bath_sweeps_of_the_samples': sweeps, 'reference_energy': e_ref, 'mean_energy_of_the_samples': sample_energy,
           'mean_energy_of_the_quenched': float(np.mean(ins.energy)), 'sets': []}
    for kind, rows in (('quenched next to the reference', quenched), ('beta samples', samples)):
        res['sets'].append(measure(kind, rows, graph, d_ref, nbits, K, reps))
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    argv = sys.argv[1:]
    M, reps = _opt(argv, '--M', 2 ** 16, int), _opt(argv, '--reps', 5, int)
    beta, sweeps, K = _opt(argv, '--beta', 1.0, float), _opt(argv, '--sweeps', 32, int), _opt(argv, '--K', 64, int)
    run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'droplets_profile.json'), M, reps, beta, sweeps, K)
