"""The cell sweeps of tnac4o.relax_samples (tn_cell_sweep) at the two shapes a user runs, next to one sample_boltzmann of the same M.

    python tools/relax_profile.py run [OUT.json] [--M 65536] [--sweeps 3] [--reps 3] [--chi 32] [--skip-sampling]
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/relax_profile.py run /dev/null --skip-sampling

Shapes: synthetic_chimera(16, 16, seed) (256 cells of Nc = 8, q = 256) and synthetic_rmf(64, 64, 8, seed) (4096 sites of d = 8), M
configurations drawn uniformly.  Per shape and mode (heat bath / quench), with the default staging rule, with every table staged in LDS
(TN_CELL_SWEEP_LDS=153600) and with every table read from global memory (TN_CELL_SWEEP_LDS=0): one warm-up call, then `reps` calls of `sweeps` sweeps on fresh copies of the same states, each
timed with device events around the call; reported are ms per sweep (the energy pass and the table launches of a call included) and
cell updates per second.  Next to them: the bytes and operations of the kernel's roofline computed from the shapes (see `roofline`),
the least time the device could take, and -- unless --skip-sampling -- the time of one sample_boltzmann(M, Dmax=chi) on the same
instance, boundary sweep apart.  No time here is a pass / fail condition: there is no earlier implementation to compare with.
Writes a JSON (default profiles/relax_profile.json) that states what was measured and what was not."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260019
PEAK_FP64 = 78.6e12            # vector fp64, operations per second (MI355X)
PEAK_HBM = 8.0e12              # bytes per second (specification; about 6.3e12 is achievable)
EXP_OPS = 20                   # fp64 operations a double-precision exp is counted as (range reduction and a polynomial of degree about 12)


def _opt(argv, name, default, cast):
    if name in argv:
        i = argv.index(name)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def roofline(M, ncell, q, neighbours, mode):
    """Operations and bytes one sweep needs, from the shapes.  Per (sample, cell): q conditional energies of `neighbours` additions
    each (4 in the bulk), a comparison per state for the minimum; heat bath: per state a subtraction, a multiplication, an exp (counted
    as EXP_OPS operations) and an addition of the running sum.  Bytes that must cross HBM: the state read and written (2 + 2), the flag (1), heat bath:
    the uniform number (8); the tables and the neighbours' states are shared and stay in cache."""
    per_state = neighbours + 1 + (3 + EXP_OPS if mode == 'heat_bath' else 0)
    ops = float(M) * ncell * q * per_state
    nbytes = float(M) * ncell * (5 + (8 if mode == 'heat_bath' else 0))
    t = max(ops / PEAK_FP64, nbytes / PEAK_HBM)
    return {'operations': ops, 'bytes': nbytes, 'least_ms': 1e3 * t, 'bound': 'operations' if ops / PEAK_FP64 >= nbytes / PEAK_HBM else 'bytes'}


def measure(ins, name, M, sweeps, reps):
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
    qs = ins._cell_sizes()
    g = torch.Generator(device=dev)
    g.manual_seed(SEED)
    start = (torch.rand((M, ncell), generator=g, device=dev, dtype=torch.float64) * torch.as_tensor(qs, device=dev)[None, :]).to(torch.int16)
    u = torch.rand((sweeps, ncell, M), generator=g, device=dev, dtype=torch.float64)
    wsb = int(L.tn_cell_sweep_ws_bytes(Nx, Ny, M))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    E = torch.empty(M, dtype=torch.float64, device=dev)
    mv = torch.empty(M, dtype=torch.int32, device=dev)
    lm = torch.empty(M, dtype=torch.int32, device=dev)
    q = int(qs.max())
    out = {'shape': name, 'cells': ncell, 'q': q, 'M': M, 'sweeps_per_call': sweeps, 'reps': reps, 'modes': {}}
    for mode_name, mode in (('heat_bath', 0), ('quench', 1)):
        res = {'roofline': roofline(M, ncell, q, 4, mode_name)}
        for label, env in (('default', None), ('lds', str(150 * 1024)), ('global', '0')):
            os.environ.pop('TN_CELL_SWEEP_LDS', None)
            if env is not None:
                os.environ['TN_CELL_SWEEP_LDS'] = env
            times, moved, Emean = [], None, None
            for rep in range(reps + 1):                   # the first call is the warm-up
                st = start.clone()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                ops.check(L.tn_cell_sweep(Nx, Ny, cells, M, st.data_ptr(), mode, float(ins.beta), sweeps, u.data_ptr() if mode == 0 else None,
                                          M if mode == 0 else 0, E.data_ptr(), mv.data_ptr(), lm.data_ptr(), ws.data_ptr(), wsb, ops._stream()))
                b.record()
                torch.cuda.synchronize()
                if rep:
                    times.append(a.elapsed_time(b) / sweeps)
                moved, Emean = float(mv.double().mean().item()), float(E.mean().item())
            ms = float(np.median(times))
            res[label] = {'ms_per_sweep': times, 'ms_per_sweep_median': ms, 'spread_ms': float(np.ptp(times)),
                          'cell_updates_per_s': M * ncell / (ms * 1e-3), 'share_of_least_time': res['roofline']['least_ms'] / ms,
                          'mean_moves_per_sample': moved, 'mean_energy_after': Emean}
            print(name, mode_name, label, json.dumps(res[label]), flush=True)
        os.environ.pop('TN_CELL_SWEEP_LDS', None)
        res['same_result_every_setting'] = bool(len({(res[k]['mean_energy_after'], res[k]['mean_moves_per_sample']) for k in ('default', 'lds', 'global')}) == 1)
        out['modes'][mode_name] = res
    return out


def sampling(ins, M, chi):
    """Seconds of the boundary sweep and of one sample_boltzmann walk of M samples on it."""
    import numpy as np
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ins._setup_rhoT(graduate_truncation=True, Dmax=chi, tolS=1e-15, tolV=1e-10, max_sweeps=20)
    torch.cuda.synchronize()
    sweep_s = time.perf_counter() - t0
    build = ins._setup_rhoT
    ins._setup_rhoT = lambda **kw: None
    u = np.random.default_rng(SEED).random((ins.Nx * ins.Ny, M))
    t0 = time.perf_counter()
    ins.sample_boltzmann(M=M, Dmax=chi, uniforms=u)
    torch.cuda.synchronize()
    walk_s = time.perf_counter() - t0
    ins._setup_rhoT = build
    return {'chi': chi, 'boundary_sweep_s': sweep_s, 'sample_boltzmann_walk_s': walk_s, 'runs': 1}


def run(out_json, M, sweeps, reps, chi, skip_sampling):
    import torch
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera, synthetic_rmf
    assert torch.cuda.is_available(), 'relax_profile needs a GPU'
    torch.cuda.set_device(0)
    res = {'what': 'tn_cell_sweep: ms per sweep by device events around calls of %d sweeps (median of %d after a warm-up call)' % (sweeps, reps),
           'peaks': {'fp64_ops_per_s': PEAK_FP64, 'hbm_bytes_per_s': PEAK_HBM}, 'shapes': [], 'not_measured': []}
    shapes = (('chimera 16x16 cells, Nc = 8', lambda: tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, SEED), beta=1.0)),
              ('RMF 64x64, d = 8', lambda: tnac4o_amd.tnac4o(mode='RMF', Nx=64, Ny=64, J=synthetic_rmf(64, 64, 8, SEED), beta=1.0)))
    for name, make in shapes:
        ins = make()
        shape = measure(ins, name, M, sweeps, reps)
        if skip_sampling:
            shape['sample_boltzmann'] = None
            res['not_measured'].append('sample_boltzmann(M=%d, Dmax=%d) on %s (skipped on request)' % (M, chi, name))
        else:
            try:
                shape['sample_boltzmann'] = sampling(ins, M, chi)
            except (NotImplementedError, MemoryError) as e:
                shape['sample_boltzmann'] = None
                res['not_measured'].append('sample_boltzmann(M=%d, Dmax=%d) on %s: %s' % (M, chi, name, e))
        print(name, 'sample_boltzmann', json.dumps(shape['sample_boltzmann']), flush=True)
        res['shapes'].append(shape)
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, 'w') as f:                   # (after every shape: a later one that fails loses nothing)
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    argv = sys.argv[1:]
    M, sweeps, reps = _opt(argv, '--M', 2 ** 16, int), _opt(argv, '--sweeps', 3, int), _opt(argv, '--reps', 3, int)
    chi = _opt(argv, '--chi', 32, int)
    skip = '--skip-sampling' in argv
    if skip:
        argv.remove('--skip-sampling')
    run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'relax_profile.json'), M, sweeps, reps, chi, skip)
