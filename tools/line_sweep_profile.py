"""The line sweeps of tnac4o.relax_lines (tn_line_sweep) next to the cell sweeps of relax_samples (tn_cell_sweep) on the same states.

    python tools/line_sweep_profile.py run [OUT.json] [--M 16384,65536] [--sweeps 2] [--reps 3] [--beta 3.0] [--n 10]

Shape: synthetic_chimera(16, 16, seed) (256 cells of Nc = 8, q = 256, 16 columns in E1 / E4), M configurations drawn uniformly.
Speed, per M: for lines = rows / columns / both and mode = heat bath / quench one warm-up call, then `reps` calls of `sweeps` sweeps on
fresh copies of the same states, each timed with device events around the call; reported are the ms per sweep of every call, their
median and spread; beside them the same for tn_cell_sweep, the ratio, and the counted work of a line sweep (`counted_work`) with the
least time the device could take for it.  The heat-bath call includes its table build and the read-back of the range guard.
What the move buys, at the smallest M and inverse temperature `beta`, from one random start: the mean energy after n line sweeps
('both') and after n cell sweeps, and the mean energy and the sweeps of a quench to convergence with each move.
No number here is a pass / fail condition.  Writes a JSON (default profiles/line_sweep_profile.json)."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260025
PEAK_FP64 = 78.6e12            # vector fp64, operations per second (MI355X)
PEAK_HBM = 8.0e12              # bytes per second (specification)
EXP_OPS = 20                   # fp64 operations a double-precision exp is counted as (as tools/relax_profile.py)
LINES = {'rows': 0, 'columns': 1, 'both': 2}


def _opt(argv, name, default, cast):
    if name in argv:
        i = argv.index(name)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def counted_work(M, ncell, q, cols, passes, mode):
    """Operations and bytes of one sweep of `passes` passes, from the shapes.  Per (sample, cell, pass), forward and again backward:
    q side energies of 2 additions, q x cols multiply-adds (2 operations each) of the message product -- (min, +): an addition and a
    comparison --, a comparison per state; heat bath: 2 exponentials per state (the weight, forward and backward) and the running
    sum; the gather of the messages reads each state once.  Bytes that must cross HBM: the state read and written (2 + 2), the flag
    (1), heat bath: the uniform number (8); tables and messages stay in cache / LDS."""
    per_state = 2 * (2 + 2 * cols + 1) + 1 + ((2 * EXP_OPS + 4) if mode == 'heat_bath' else 0)
    ops = float(M) * ncell * passes * q * per_state
    nbytes = float(M) * ncell * passes * (5 + (8 if mode == 'heat_bath' else 0))
    return {'operations': ops, 'multiply_adds': float(M) * ncell * passes * q * 2 * cols,
            'exponentials': float(M) * ncell * passes * q * 2 if mode == 'heat_bath' else 0.0, 'bytes': nbytes,
            'least_ms': 1e3 * max(ops / PEAK_FP64, nbytes / PEAK_HBM), 'bound': 'operations' if ops / PEAK_FP64 >= nbytes / PEAK_HBM else 'bytes'}


class Bench:
    def __init__(self, ins, M):
        import torch
        from tnac4o_amd import relax
        from tnac4o_amd._lib import lib
        self.torch, self.L, self.ins, self.M = torch, lib(), ins, M
        self.dev = torch.device('cuda', torch.cuda.current_device())
        self.Nx, self.Ny = ins.Nx, ins.Ny
        self.ncell = self.Nx * self.Ny
        self.table = relax.EnergyCells(ins, self.dev)
        self.cells = C.cast(self.table.cells, C.c_void_p)
        self.qs = ins._cell_sizes()
        self.g = torch.Generator(device=self.dev)
        self.g.manual_seed(SEED)
        self.start = (torch.rand((M, self.ncell), generator=self.g, device=self.dev, dtype=torch.float64)
                      * torch.as_tensor(self.qs, device=self.dev)[None, :]).to(torch.int16)
        self.wsb = max(int(self.L.tn_line_sweep_ws_bytes(self.Nx, self.Ny, M)), int(self.L.tn_cell_sweep_ws_bytes(self.Nx, self.Ny, M)))
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)
        self.E = torch.empty(M, dtype=torch.float64, device=self.dev)
        self.mv = torch.empty(M, dtype=torch.int32, device=self.dev)
        self.lm = torch.empty(M, dtype=torch.int32, device=self.dev)

    def uniforms(self, rows):
        return self.torch.rand((rows, self.M), generator=self.g, device=self.dev, dtype=self.torch.float64)

    def call(self, st, move, mode, sweeps, beta, u):
        """move: 'cell' or a lines value.  Returns the device milliseconds of the call."""
        from tnac4o_amd import ops
        t = self.torch
        a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        up, ldu = (u.data_ptr(), self.M) if mode == 0 else (None, 0)
        a.record()
        if move == 'cell':
            ops.check(self.L.tn_cell_sweep(self.Nx, self.Ny, self.cells, self.M, st.data_ptr(), mode, beta, sweeps, up, ldu, self.E.data_ptr(),
                                           self.mv.data_ptr(), self.lm.data_ptr(), self.ws.data_ptr(), self.wsb, ops._stream()))
        else:
            ops.check(self.L.tn_line_sweep(self.Nx, self.Ny, self.cells, self.M, st.data_ptr(), mode, LINES[move], beta, sweeps, up, ldu,
                                           self.E.data_ptr(), self.mv.data_ptr(), self.lm.data_ptr(), self.ws.data_ptr(), self.wsb, ops._stream()))
        b.record()
        t.cuda.synchronize()
        return a.elapsed_time(b)

    def timed(self, move, mode, sweeps, reps, beta):
        import numpy as np
        P = 2 if move == 'both' else 1
        u = self.uniforms(sweeps * P * self.ncell) if mode == 0 else None
        times = []
        for rep in range(reps + 1):                       # the first call is the warm-up
            ms = self.call(self.start.clone(), move, mode, sweeps, beta, u)
            if rep:
                times.append(ms / sweeps)
        return {'ms_per_sweep': times, 'ms_per_sweep_median': float(np.median(times)), 'spread_ms': float(np.ptp(times)),
                'mean_energy_after': float(self.E.mean().item()), 'mean_moves_per_sample': float(self.mv.double().mean().item())}

    def quench_to_convergence(self, st, move, max_sweeps=64, block=4):
        done, ms = 0, 0.0
        while done < max_sweeps:
            ms += self.call(st, move, 1, block, 1.0, None)
            done += block
            if not bool(self.lm.any().item()):
                break
        return {'sweeps_run': done, 'converged': not bool(self.lm.any().item()), 'ms': ms, 'mean_energy': float(self.E.mean().item()),
                'lowest_energy': float(self.E.min().item())}


def speed(ins, M, sweeps, reps, beta):
    b = Bench(ins, M)
    q, cols = int(b.qs.max()), 16
    out = {'M': M, 'sweeps_per_call': sweeps, 'reps': reps, 'beta': beta, 'modes': {}}
    for mode_name, mode in (('heat_bath', 0), ('quench', 1)):
        res = {'cell_sweep': b.timed('cell', mode, sweeps, reps, beta)}
        for lines in ('rows', 'columns', 'both'):
            r = b.timed(lines, mode, sweeps, reps, beta)
            r['counted_work'] = counted_work(M, b.ncell, q, cols, 2 if lines == 'both' else 1, mode_name)
            r['ratio_to_cell_sweep'] = r['ms_per_sweep_median'] / res['cell_sweep']['ms_per_sweep_median']
            r['share_of_least_time'] = r['counted_work']['least_ms'] / r['ms_per_sweep_median']
            res[lines] = r
            print(M, mode_name, lines, json.dumps(r), flush=True)
        print(M, mode_name, 'cell_sweep', json.dumps(res['cell_sweep']), flush=True)
        out['modes'][mode_name] = res
    return out


def quality(ins, M, beta, n):
    """From one random start at `beta`: mean energy after n heat-bath sweeps and after a quench to convergence, with each move."""
    b = Bench(ins, M)
    out = {'M': M, 'beta': beta, 'n': n, 'mean_energy_of_the_start': None, 'heat_bath': {}, 'quench': {}}
    b.call(b.start.clone(), 'cell', 1, 0, 1.0, None)
    out['mean_energy_of_the_start'] = float(b.E.mean().item())
    for move, P in (('both', 2), ('cell', 1)):
        st = b.start.clone()
        ms = b.call(st, move, 0, n, beta, b.uniforms(n * P * b.ncell))
        out['heat_bath'][move] = {'sweeps': n, 'ms': ms, 'mean_energy': float(b.E.mean().item()), 'lowest_energy': float(b.E.min().item())}
        out['quench'][move] = b.quench_to_convergence(b.start.clone(), move)
        print('quality', move, json.dumps(out['heat_bath'][move]), json.dumps(out['quench'][move]), flush=True)
    return out


def run(out_json, Ms, sweeps, reps, beta, n):
    import torch
    import tnac4o_amd
    from tnac4o_amd import lines
    from tnac4o_amd.auxx import synthetic_chimera
    assert torch.cuda.is_available(), 'line_sweep_profile needs a GPU'
    torch.cuda.set_device(0)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, SEED), beta=beta)
    res = {'what': 'tn_line_sweep next to tn_cell_sweep on chimera 16x16 cells, Nc = 8 (q = 256): ms per sweep by device events around calls of '
                   '%d sweeps (median of %d after a warm-up call)' % (sweeps, reps),
           'peaks': {'fp64_ops_per_s': PEAK_FP64, 'hbm_bytes_per_s': PEAK_HBM, 'exp_counted_as_ops': EXP_OPS},
           'beta_times_largest_chain_range': beta * lines.chain_range(ins, 'both'), 'speed': [], 'what_the_move_buys': None}
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    for M in Ms:
        res['speed'].append(speed(ins, M, sweeps, reps, beta))
        with open(out_json, 'w') as f:                   # (after every part: a later one that fails loses nothing)
            json.dump(res, f, indent=1)
    res['what_the_move_buys'] = quality(ins, min(Ms), beta, n)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    argv = sys.argv[1:]
    Ms = _opt(argv, '--M', [2 ** 14, 2 ** 16], lambda s: [int(x) for x in s.split(',')])
    sweeps, reps = _opt(argv, '--sweeps', 2, int), _opt(argv, '--reps', 3, int)
    beta, n = _opt(argv, '--beta', 3.0, float), _opt(argv, '--n', 10, int)
    run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'line_sweep_profile.json'), Ms, sweeps, reps, beta, n)
