"""One call of tn_temper (tnac4o.temper_samples) at the shape a user runs, next to the same work composed of today's separate entry
points, and next to the single-beta sweep its per-row-beta sweep came from.

    python tools/temper_profile.py run [OUT.json] [--M 16384] [--reps 3] [--rounds 4]

Instance: synthetic_chimera(16, 16, seed) (256 cells of Nc = 8, 2048 spins), T = 16 betas from 0.1 to 1.6, M rows = M / 16 chains
(default M = 2^14: 1024 chains; the sweep's uniform numbers are 32 MiB per round), uniformly random start, M / 32 chain pairs per round,
cluster moves at every temperature, one sweep per round.  Every figure is the median of `reps` timed runs after one warm-up run, timed
with device events around the whole run (host work between the launches included), each from a fresh copy of the start:
  tn_temper        `rounds` rounds in one call; ms per round.
  composition      the same rounds from the parent's entry points: tn_cell_sweep per temperature group (16 calls of M / 16 rows), download,
                   binary_states + pack on the host, upload, one tn_cluster_exchange over the M / 2 row pairs, download, unpack +
                   states_from_binary on the host, upload; the swap decisions on the host from tn_cell_sweep's energies (one more
                   call without a sweep).  The groups are the static row blocks: the same volume of work, not the same trajectory.
  sweep            one heat-bath sweep of tn_cell_sweep over the M rows at one beta, and tn_temper with nbits = 0, one round of one
                   sweep (per-row beta; it adds the swap kernel and nothing else): the cost of the per-row beta against the kernel
                   it came from, with the spread (max - min) of each so that the difference can be read against it.
No time here is a pass / fail condition.  Writes a JSON (default profiles/temper_profile.json)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260021
T = 16


def _opt(argv, name, default, cast):
    if name in argv:
        i = argv.index(name)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def timed(fn, reps):
    """[ms] of `reps` runs of fn() after one warm-up run, device events around each."""
    import torch
    out = []
    for rep in range(reps + 1):
        prepared = fn(None)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(prepared)
        b.record()
        torch.cuda.synchronize()
        if rep:
            out.append(a.elapsed_time(b))
    return out


def stats(ms, per=1):
    import numpy as np
    ms = [x / per for x in ms]
    return {'ms': ms, 'ms_median': float(np.median(ms)), 'spread_ms': float(np.ptp(ms))}


def run(out_json, M, reps, rounds):
    import numpy as np
    import torch
    import tnac4o_amd
    from tnac4o_amd import exchange, ops, overlap, relax, temper
    from tnac4o_amd._lib import lib
    from tnac4o_amd.auxx import synthetic_chimera
    assert torch.cuda.is_available(), 'temper_profile needs a GPU'
    assert M % (2 * T) == 0
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    L = lib()
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, SEED), beta=1.0)
    Nx, Ny, ncell, R = ins.Nx, ins.Ny, ins.Nx * ins.Ny, M // T
    betas = np.linspace(0.1, 1.6, T)
    rng = np.random.default_rng(SEED)
    start = rng.integers(0, 256, (M, ncell)).astype(np.int16)            # lattice order of the solver's rotation
    nbits, cellbits, bitcell = temper.bit_tables(ins)
    rowptr, cols = exchange.coupling_csr(ins)
    table = relax.EnergyCells(ins, dev)
    cells = C.cast(table.cells, C.c_void_p)
    d_start = torch.as_tensor(start).to(dev)
    bits = (nbits,) + tuple(torch.as_tensor(x).to(dev) for x in (cellbits, bitcell, rowptr, cols))
    Pc = R // 2
    d_us = torch.as_tensor(rng.random((rounds, 1, ncell, M))).to(dev)
    d_cp = torch.as_tensor(np.array([rng.permutation(R).reshape(Pc, 2) for _ in range(rounds)], dtype=np.int32)).to(dev)
    d_ucl, d_uw = torch.as_tensor(rng.random((rounds, T, Pc))).to(dev), torch.as_tensor(rng.random((rounds, R, T - 1))).to(dev)
    tidx0 = torch.as_tensor((np.arange(M) % T).astype(np.int32)).to(dev)
    slot0 = torch.as_tensor(np.arange(M, dtype=np.int32).reshape(R, T)).to(dev)
    res = {'what': 'tn_temper against the composition of tn_cell_sweep + host conversion + tn_cluster_exchange, chimera 16x16 cells, Nc = 8, T = %d, '
                   'M = %d rows (%d chains), %d rounds of one sweep per run; device events around each run, median of %d after a warm-up' % (T, M, R, rounds, reps),
           'M': M, 'T': T, 'chains': R, 'rounds_per_run': rounds, 'betas': betas.tolist(), 'nbits': nbits, 'chain_pairs_per_round': Pc}
    last = {}

    def temper_run(prepared, nb=bits, nrounds=rounds):
        if prepared is None:
            return (d_start.clone(), tidx0.clone(), slot0.clone(), torch.zeros(T - 1, dtype=torch.int32, device=dev),
                    torch.zeros(T - 1, dtype=torch.int32, device=dev))
        st, tidx, slot, acc, att = prepared
        last['out'] = ops.temper(table.cells, Nx, Ny, betas, st, tidx, slot, 0, nrounds, 1, usweep=d_us[:nrounds], bits=nb, cluster_from=0,
                                 cpairs=d_cp[:nrounds] if nb is not None else None, ucl=d_ucl[:nrounds] if nb is not None else None,
                                 uswap=d_uw[:nrounds], accepted=acc, attempted=att, record=nb is not None)
        last['acc'], last['att'] = acc, att

    res['tn_temper'] = stats(timed(temper_run, reps), rounds)
    res['tn_temper'].update({'swap_accepted': last['acc'].cpu().tolist(), 'swap_attempted': last['att'].cpu().tolist(),
                             'mean_cluster_size': float(last['out']['sizes'].double().mean().item()),
                             'mean_differing_spins': float(last['out']['differing'].double().mean().item())})
    print(json.dumps(res['tn_temper']), flush=True)

    # ---- today's composition: rows of temperature t are the block [t R, (t + 1) R)
    wsb = int(L.tn_cell_sweep_ws_bytes(Nx, Ny, M))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    E = torch.empty(M, dtype=torch.float64, device=dev)
    act = overlap.active_spins(ins)
    order = np.asarray(ins.order)
    pairs = torch.arange(M, dtype=torch.int32, device=dev).reshape(-1, 2)          # neighbours inside a block: the same temperature
    d_rowptr, d_cols = bits[3], bits[4]
    host_ms = []

    def composition(prepared):
        import time
        if prepared is None:
            return d_start.clone()
        st = prepared
        host = 0.0
        for r in range(rounds):
            for t in range(T):
                ops.check(L.tn_cell_sweep(Nx, Ny, cells, R, st.data_ptr() + t * R * ncell * 2, 0, float(betas[t]), 1, d_us[r].data_ptr() + t * R * 8, M,
                                          E.data_ptr() + t * R * 8, None, None, ws.data_ptr(), wsb, ops._stream()))
            t0 = time.perf_counter()
            ins.states = st.cpu().numpy().astype(np.int64)[:, order]     # model cell order
            rows = overlap.pack_bits(overlap.spin_bits(ins))
            host += time.perf_counter() - t0
            d_rows = torch.as_tensor(rows.view(np.int64)).to(dev)
            ops.cluster_exchange(d_rows, nbits, d_rowptr, d_cols, pairs, d_ucl[r].reshape(-1)[:M // 2].contiguous())
            rows = d_rows.cpu().numpy().view(np.uint64)
            t0 = time.perf_counter()
            b = np.zeros((M, int(ins.L)), dtype=np.int8)
            b[:, act] = exchange.unpack_bits(rows, nbits)
            new = np.empty((M, ncell), dtype=np.int16)
            new[:, order] = ins.states_from_binary(b)
            host += time.perf_counter() - t0
            st.copy_(torch.as_tensor(new).to(dev))
            ops.check(L.tn_cell_sweep(Nx, Ny, cells, M, st.data_ptr(), 1, 1.0, 0, None, 0, E.data_ptr(), None, None, ws.data_ptr(), wsb, ops._stream()))
            e = E.cpu().numpy().reshape(T, R)                            # the swap decisions on the host (labels only; not applied to the blocks)
            par = r & 1
            delta = (betas[par + 1::2, None] - betas[par:T - 1:2, None]) * (e[par + 1::2] - e[par:T - 1:2])
            _ = (delta >= 0) | (d_uw[r].cpu().numpy().T[par:T - 1:2] < np.exp(np.minimum(delta, 0.0)))
        host_ms.append(1e3 * host / rounds)

    res['composition'] = stats(timed(composition, reps), rounds)
    res['composition']['host_conversion_ms_per_round'] = host_ms[1:]
    print(json.dumps(res['composition']), flush=True)

    # ---- the per-row beta against the single-beta sweep
    d_u1 = d_us[0, 0]

    def plain_sweep(prepared):
        if prepared is None:
            return d_start.clone()
        ops.check(L.tn_cell_sweep(Nx, Ny, cells, M, prepared.data_ptr(), 0, 1.0, 1, d_u1.data_ptr(), M, E.data_ptr(), None, None, ws.data_ptr(), wsb,
                                  ops._stream()))

    res['sweep_single_beta'] = stats(timed(plain_sweep, reps))
    res['sweep_per_row_beta'] = stats(timed(lambda p: temper_run(p, nb=None, nrounds=1), reps))
    a, b = res['sweep_single_beta'], res['sweep_per_row_beta']
    res['per_row_beta_minus_single_beta_ms'] = b['ms_median'] - a['ms_median']
    res['run_to_run_spread_ms'] = max(a['spread_ms'], b['spread_ms'])
    res['ratio_composition_to_tn_temper'] = res['composition']['ms_median'] / res['tn_temper']['ms_median']
    print(json.dumps({k: res[k] for k in ('sweep_single_beta', 'sweep_per_row_beta', 'per_row_beta_minus_single_beta_ms', 'run_to_run_spread_ms')}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    argv = sys.argv[1:]
    M, reps, rounds = _opt(argv, '--M', 2 ** 14, int), _opt(argv, '--reps', 3, int), _opt(argv, '--rounds', 4, int)
    run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'temper_profile.json'), M, reps, rounds)
