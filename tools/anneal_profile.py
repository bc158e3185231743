"""One call of tn_anneal (tnac4o.anneal_population) at the shape a user runs, next to the same schedule composed of the entry points that
existed before it, and its log2 Z next to the contraction's on an instance small enough for the contraction to be exact.

    python tools/anneal_profile.py run [OUT.json] [--M 16384] [--reps 3] [--runs 8]
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/anneal_profile.py once [--M 16384]
    python tools/anneal_profile.py kernels OUT/.../run_kernel_stats.csv [OUT.json]

(a) Time per step.  Instance: synthetic_chimera(16, 16, seed) (256 cells of Nc = 8, 2048 spins), K = 16 betas from 0 to 1.6, M rows
(default 2^14; the sweep's uniform numbers are 32 MiB per step), uniformly random start, one sweep per step.  Every figure is the median
of `reps` timed runs after one warm-up run, device events around the whole run (host work between the launches included), each from a
fresh copy of the start:
  tn_anneal        the 15 steps in one call; ms per step.
  split            tn_anneal with sweeps = 0 (resampling chain + energy pass per step): sweep = whole - (sweeps = 0).  K back-to-back
                   calls of tn_cell_sweep with sweeps = 0 stand beside it for scale; such a call also uploads the table of the cells
                   and is no part of tn_anneal, so the chain is NOT taken as a difference against it.  The chain and the energy
                   pass are told apart by kernel times: `once` makes a warm-up call and one call of (a) for a rocprofv3 kernel
                   trace, `kernels` folds the trace's statistics (two calls) into ms per step by kernel family and adds them to the
                   JSON.
  composition      the same schedule from tn_cell_sweep alone: per step the energies and the rows are downloaded, weights, running sums,
                   offsets and parents are computed with numpy, the resampled rows are uploaded, and tn_cell_sweep makes the sweep and
                   the energies.  The same volume of work and the same rule, numpy's order of the additions.
(b) log2 Z.  synthetic_chimera(2, 2, 29) (4 cells of Nc = 8, 32 spins) at beta = 1: calculate_free_energy with Dmax above every bond
(nothing truncated), beside anneal_log2Z[-1] of `runs` independent runs (betas 0 .. 1 in 21 steps, 2 sweeps, M rows), with their mean,
standard error, spread and rho_t.
No number here is a pass / fail condition.  Writes a JSON (default profiles/anneal_profile.json)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260022
K = 16


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


def host_resample(E, db, u):
    """The resampling rule of include/tnpeps.h (K13) in numpy: parents of the M rows."""
    import numpy as np
    M = E.size
    w = np.exp(-(db * (E - np.fmin.reduce(E))))
    w = np.where(np.isnan(w), 0.0, w)
    c = np.cumsum(w)
    if not (c[-1] > 0.0 and np.isfinite(c[-1])):
        return np.arange(M)
    O = np.clip(np.floor(c / c[-1] * M + u), 0, M).astype(np.int64)
    O = np.maximum.accumulate(O)
    O[-1] = M
    return np.searchsorted(O, np.arange(M), side='right')


def time_per_step(res, M, reps, once=False):
    import numpy as np
    import torch
    import tnac4o_amd
    from tnac4o_amd import ops, relax
    from tnac4o_amd._lib import lib
    from tnac4o_amd.auxx import synthetic_chimera
    dev = torch.device('cuda', 0)
    L = lib()
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, SEED), beta=1.0)
    Nx, Ny, ncell = ins.Nx, ins.Ny, ins.Nx * ins.Ny
    betas = np.linspace(0.0, 1.6, K)
    steps = K - 1
    rng = np.random.default_rng(SEED)
    start = rng.integers(0, 256, (M, ncell)).astype(np.int16)            # lattice order of the solver's rotation
    table = relax.EnergyCells(ins, dev)
    cells = C.cast(table.cells, C.c_void_p)
    d_start = torch.as_tensor(start).to(dev)
    d_us = torch.as_tensor(rng.random((steps, 1, ncell, M))).to(dev)
    ures = rng.random(steps)
    d_ur = torch.as_tensor(ures).to(dev)
    fam0 = torch.arange(M, dtype=torch.int32, device=dev)
    a = {'what': 'tn_anneal against the composition of tn_cell_sweep + download + numpy resampling + upload, chimera 16x16 cells, Nc = 8, K = %d betas '
                 '0 .. 1.6, M = %d rows, one sweep per step; device events around each run of %d steps, median of %d after a warm-up' % (K, M, steps, reps),
         'M': M, 'K': K, 'steps_per_run': steps, 'betas': betas.tolist()}
    last = {}

    def anneal_run(prepared, sweeps=1):
        if prepared is None:
            return d_start.clone(), fam0.clone()
        st, fam = prepared
        last['out'] = ops.anneal(table.cells, Nx, Ny, betas, st, fam, sweeps, usweep=d_us if sweeps else None, ures=d_ur)

    if once:                                                             # a warm-up call and one call, for a kernel trace
        for _ in range(2):
            anneal_run(anneal_run(None))
        torch.cuda.synchronize()
        return
    a['tn_anneal'] = stats(timed(anneal_run, reps), steps)
    out = last['out']
    a['tn_anneal'].update({'survivors': out['survivors'].cpu().tolist(),
                           'ess': (out['wsum'] ** 2 / out['w2sum']).cpu().tolist()})
    print(json.dumps(a['tn_anneal']), flush=True)
    a['tn_anneal_without_sweeps'] = stats(timed(lambda p: anneal_run(p, 0), reps), steps)

    wsb = int(L.tn_cell_sweep_ws_bytes(Nx, Ny, M))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    E = torch.empty(M, dtype=torch.float64, device=dev)

    def energy_pass(prepared):
        if prepared is None:
            return d_start.clone()
        for _ in range(K):                                               # (a run of tn_anneal makes K energy passes: one on entry, one per step)
            ops.check(L.tn_cell_sweep(Nx, Ny, cells, M, prepared.data_ptr(), 1, 1.0, 0, None, 0, E.data_ptr(), None, None, ws.data_ptr(), wsb,
                                      ops._stream()))

    a['energy_pass'] = stats(timed(energy_pass, reps), K)
    a['split_ms_per_step'] = {'sweep': a['tn_anneal']['ms_median'] - a['tn_anneal_without_sweeps']['ms_median'],
                              'resampling_chain_and_energy_pass': a['tn_anneal_without_sweeps']['ms_median'],
                              'one_tn_cell_sweep_call_without_sweeps': a['energy_pass']['ms_median']}
    print(json.dumps(a['split_ms_per_step']), flush=True)

    def composition(prepared):
        if prepared is None:
            return d_start.clone()
        st = prepared
        ops.check(L.tn_cell_sweep(Nx, Ny, cells, M, st.data_ptr(), 1, 1.0, 0, None, 0, E.data_ptr(), None, None, ws.data_ptr(), wsb, ops._stream()))
        for s in range(1, K):
            e, rows = E.cpu().numpy(), st.cpu().numpy()
            parent = host_resample(e, betas[s] - betas[s - 1], ures[s - 1])
            st.copy_(torch.as_tensor(rows[parent]).to(dev))
            ops.check(L.tn_cell_sweep(Nx, Ny, cells, M, st.data_ptr(), 0, float(betas[s]), 1, d_us[s - 1].data_ptr(), M, E.data_ptr(), None, None,
                                      ws.data_ptr(), wsb, ops._stream()))

    a['composition'] = stats(timed(composition, reps), steps)
    a['ratio_composition_to_tn_anneal'] = a['composition']['ms_median'] / a['tn_anneal']['ms_median']
    print(json.dumps({k: a[k] for k in ('composition', 'ratio_composition_to_tn_anneal')}), flush=True)
    res['time_per_step'] = a


def log2Z_agreement(res, M, runs):
    import numpy as np
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    beta = 1.0
    J = synthetic_chimera(2, 2, 29)
    ref = tnac4o_amd.tnac4o(mode='Ising', Nx=2, Ny=2, Nc=8, J=J, beta=beta)
    exact = float(ref.calculate_free_energy(Dmax=4096))
    betas = np.linspace(0.0, beta, 21)
    got, rho, ent = [], [], []
    for r in range(runs):
        np.random.seed(SEED + r)
        ins = tnac4o_amd.tnac4o(mode='Ising', Nx=2, Ny=2, Nc=8, J=J, beta=beta)
        ins.anneal_population(betas, sweeps=2, M=M)
        got.append(float(ins.anneal_log2Z[-1]))
        rho.append(float(ins.anneal_rho_t))
        ent.append(float(ins.anneal_family_entropy))
    got = np.array(got)
    res['log2Z_agreement'] = {
        'what': 'synthetic_chimera(2, 2, 29), 32 spins, beta = 1: calculate_free_energy(Dmax=4096) (no bond truncated) beside anneal_log2Z[-1] of %d '
                'independent runs, betas 0 .. 1 in 21 steps, 2 sweeps, M = %d' % (runs, M),
        'log2Z_contraction': exact, 'free_energy_row_spread': float(ref.free_energy_row_spread), 'anneal_log2Z': got.tolist(),
        'mean': float(got.mean()), 'standard_error': float(got.std(ddof=1) / np.sqrt(runs)), 'spread': float(np.ptp(got)),
        'mean_minus_contraction': float(got.mean() - exact), 'rho_t': rho, 'family_entropy': ent}
    print(json.dumps(res['log2Z_agreement']), flush=True)


def run(out_json, M, reps, runs):
    import torch
    assert torch.cuda.is_available(), 'anneal_profile needs a GPU'
    torch.cuda.set_device(0)
    res = {}
    log2Z_agreement(res, M, runs)
    time_per_step(res, M, reps)
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


def kernels(stats_csv, out_json):
    """ms per step by kernel family from the kernel statistics of a `once` run (two calls of K - 1 steps), added to the JSON."""
    import csv
    fam = {'resampling_chain': 0.0, 'sweep': 0.0, 'energy_pass': 0.0, 'other': 0.0}
    names = {}
    for row in csv.DictReader(open(stats_csv)):
        name, ms = row['Name'], float(row['TotalDurationNs']) * 1e-6
        key = ('resampling_chain' if 'anneal_' in name else 'sweep' if 'cell_sweep_kernel' in name else 'energy_pass' if 'sweep_energy_kernel' in name
               else 'other')
        if key != 'other':
            short = name.replace('(anonymous namespace)::', '').split('(')[0].replace('void ', '').replace('tn::', '')
            names[short] = names.get(short, 0.0) + ms / (2 * (K - 1))
        fam[key] += ms / (2 * (K - 1))
    res = json.load(open(out_json)) if os.path.exists(out_json) else {}
    res['kernel_trace_ms_per_step'] = {'what': 'rocprofv3 --kernel-trace --stats of `once` (a run of its own): kernel time per step, two calls of %d steps; '
                                               'the energy pass includes the one on entry; other = everything that is no kernel of the call' % (K - 1),
                                       'by_family': fam, 'by_kernel': names}
    print(json.dumps(res['kernel_trace_ms_per_step'], indent=1))
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    argv = sys.argv[1:]
    if argv and argv[0] == 'once':
        import torch
        torch.cuda.set_device(0)
        time_per_step({}, _opt(argv, '--M', 2 ** 14, int), 0, once=True)
        sys.exit(0)
    if argv and argv[0] == 'kernels':
        kernels(argv[1], argv[2] if len(argv) > 2 else os.path.join(ROOT, 'profiles', 'anneal_profile.json'))
        sys.exit(0)
    M, reps, runs = _opt(argv, '--M', 2 ** 14, int), _opt(argv, '--reps', 3, int), _opt(argv, '--runs', 8, int)
    run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'anneal_profile.json'), M, reps, runs)
