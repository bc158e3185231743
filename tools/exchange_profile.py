"""The cluster moves of tnac4o.exchange_clusters (tn_cluster_exchange) at the shape a user runs, next to one heat-bath sweep of
tn_cell_sweep at the same shape.

    python tools/exchange_profile.py run [OUT.json] [--M 65536] [--reps 3] [--cells 4] [--depth-sample 64]

Shape: synthetic_chimera(16, 16, seed) (256 cells of Nc = 8, 2048 spins), M rows paired (0, 1), (2, 3), ...  Two sets of rows:
'random' -- uniformly random rows, about half the spins of a pair differ, the clusters are large --, and 'few cells' -- the second
row of a pair is the first with `cells` random 8-spin cells redrawn: small clusters, the low-temperature shape.  Per set: one
warm-up call, then `reps` calls on fresh copies of the same rows, each timed with device events around the call; reported are ms
per round, the mean cluster size and number of differing spins, and, for the first `depth-sample` pairs, the mean number of growth
passes the kernel runs: the levels of the breadth-first search from the seed, the seed's own included, computed on the host.  A round
moves two rows of 256 bytes per pair in and out, 1 KiB per pair: at HBM rate that is microseconds, so the time of a round is pass
latency times passes.
For scale: one heat-bath sweep of tn_cell_sweep over the same M configurations of the same instance, measured in the same run.
No time here is a pass / fail condition.  Writes a JSON (default profiles/exchange_profile.json)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260020
PEAK_HBM = 8.0e12              # bytes per second (specification)


def _opt(argv, name, default, cast):
    if name in argv:
        i = argv.index(name)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def make_rows(kind, M, nbits, cells, rng):
    """(M, nwords) uint64: 'random' rows, or pairs (2k, 2k + 1) that differ in `cells` random bytes (8-spin cells) of the row."""
    import numpy as np
    nwords = nbits // 64
    rows = rng.integers(0, 2 ** 64, (M, nwords), dtype=np.uint64)
    if kind == 'few cells':
        by = rows.view(np.uint8).reshape(M, nwords * 8)
        by[1::2] = by[0::2]
        k = np.arange(M // 2)
        for _ in range(cells):
            by[2 * k + 1, rng.integers(0, nwords * 8, M // 2)] ^= rng.integers(1, 256, M // 2).astype(np.uint8)
    return rows


def passes(rows, nbits, rowptr, cols, uniforms, count):
    """Growth passes of the first `count` pairs: the levels of the breadth-first search from the seed through the differing spins, the
    seed's own included (every level is one pass that expands a frontier; the look that finds no frontier is not counted)."""
    out = []
    for p in range(count):
        a = sum(int(w) << (64 * k) for k, w in enumerate(rows[2 * p]))
        b = sum(int(w) << (64 * k) for k, w in enumerate(rows[2 * p + 1]))
        D = a ^ b
        cnt = bin(D).count('1')
        if cnt == 0:
            out.append(0)
            continue
        r = min(int(uniforms[p] * cnt), cnt - 1)
        d = D
        for _ in range(r):
            d &= d - 1
        seen, front, depth = d & -d, [(d & -d).bit_length() - 1], 0
        while front:
            nxt = []
            for i in front:
                for j in cols[rowptr[i]:rowptr[i + 1]]:
                    j = int(j)
                    if (D >> j) & 1 and not (seen >> j) & 1:
                        seen |= 1 << j
                        nxt.append(j)
            front, depth = nxt, depth + 1
        out.append(depth)
    return out


def measure(ins, kind, M, reps, cells, depth_sample):
    import numpy as np
    import torch
    from tnac4o_amd import exchange, ops
    nbits = int(ins.L)
    rowptr, cols = exchange.coupling_csr(ins)
    rng = np.random.default_rng(SEED)
    rows = make_rows(kind, M, nbits, cells, rng)
    u = rng.random(M // 2)
    d_start = torch.as_tensor(rows.view(np.int64)).cuda()
    d_rowptr, d_cols = torch.as_tensor(rowptr).cuda(), torch.as_tensor(cols).cuda()
    d_pairs, d_u = torch.arange(M, dtype=torch.int32, device='cuda').reshape(-1, 2), torch.as_tensor(u).cuda()
    times = []
    for rep in range(reps + 1):                           # the first call is the warm-up
        d_rows = d_start.clone()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        size, diff = ops.cluster_exchange(d_rows, nbits, d_rowptr, d_cols, d_pairs, d_u)
        b.record()
        torch.cuda.synchronize()
        if rep:
            times.append(a.elapsed_time(b))
    depth = passes(rows, nbits, rowptr, cols, u, min(depth_sample, M // 2))
    ms = float(np.median(times))
    res = {'rows': kind, 'M': M, 'pairs': M // 2, 'nbits': nbits, 'nnz': int(cols.size), 'ms_per_round': times, 'ms_per_round_median': ms,
           'spread_ms': float(np.ptp(times)), 'pairs_per_s': (M // 2) / (ms * 1e-3), 'mean_cluster_size': float(size.double().mean().item()),
           'largest_cluster': int(size.max().item()), 'mean_differing_spins': float(diff.double().mean().item()),
           'mean_passes_first_pairs': float(np.mean(depth)), 'most_passes_first_pairs': int(np.max(depth)), 'pairs_in_pass_sample': len(depth),
           'traffic_bytes': 4 * (nbits // 8) * (M // 2), 'traffic_least_ms': 1e3 * 4 * (nbits // 8) * (M // 2) / PEAK_HBM}
    print(json.dumps(res), flush=True)
    return res


def heat_bath_sweep(ins, M, reps):
    """ms of one heat-bath sweep of tn_cell_sweep over M uniformly drawn configurations (the measurement of tools/relax_profile.py)."""
    import numpy as np
    import torch
    from tnac4o_amd import ops, relax
    from tnac4o_amd._lib import lib
    L = lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    Nx, Ny = ins.Nx, ins.Ny
    ncell = Nx * Ny
    table = relax.EnergyCells(ins, dev)
    cells = C.cast(table.cells, C.c_void_p)
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    start = (torch.rand((M, ncell), generator=g, device=dev, dtype=torch.float64) * torch.as_tensor(ins._cell_sizes(), device=dev)[None, :]).to(torch.int16)
    u = torch.rand((1, ncell, M), generator=g, device=dev, dtype=torch.float64)
    wsb = int(L.tn_cell_sweep_ws_bytes(Nx, Ny, M))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    E = torch.empty(M, dtype=torch.float64, device=dev)
    times = []
    for rep in range(reps + 1):
        st = start.clone()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.check(L.tn_cell_sweep(Nx, Ny, cells, M, st.data_ptr(), 0, float(ins.beta), 1, u.data_ptr(), M, E.data_ptr(), None, None, ws.data_ptr(), wsb,
                                  ops._stream()))
        b.record()
        torch.cuda.synchronize()
        if rep:
            times.append(a.elapsed_time(b))
    return {'ms_per_sweep': times, 'ms_per_sweep_median': float(np.median(times))}


def run(out_json, M, reps, cells, depth_sample):
    import torch
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    assert torch.cuda.is_available(), 'exchange_profile needs a GPU'
    torch.cuda.set_device(0)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, SEED), beta=1.0)
    res = {'what': 'tn_cluster_exchange: ms per round by device events around the call (median of %d after a warm-up call), chimera 16x16 cells, '
                   'Nc = 8, pairs (2k, 2k + 1) of M rows' % reps, 'peaks': {'hbm_bytes_per_s': PEAK_HBM}, 'rounds': [], 'not_measured': []}
    for kind in ('random', 'few cells'):
        res['rounds'].append(measure(ins, kind, M, reps, cells, depth_sample))
    res['heat_bath_sweep_same_shape'] = heat_bath_sweep(ins, M, reps)
    print(json.dumps(res['heat_bath_sweep_same_shape']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    argv = sys.argv[1:]
    M, reps = _opt(argv, '--M', 2 ** 16, int), _opt(argv, '--reps', 3, int)
    cells, depth_sample = _opt(argv, '--cells', 4, int), _opt(argv, '--depth-sample', 64, int)
    run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'exchange_profile.json'), M, reps, cells, depth_sample)
