"""The line pass of tnac4o.calculate_correlation_function on the bench instance (synthetic chimera, L = 2048, beta = 3, chi = 64).

    python tools/correlation_function_profile.py run          # boundaries once, then the passes and the step comparison
    python tools/correlation_function_profile.py step         # boundaries, a 1 s pause, then ONE stack step of 64 slots at a bulk cell
    python tools/correlation_function_profile.py once [R]     # boundaries, a warm-up pass, a 1 s pause, then ONE line pass (reach R; default all)
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/correlation_function_profile.py step
    python tools/correlation_function_profile.py analyse OUT/.../run_kernel_trace.csv [GFLOP]

`run` prints and writes to a JSON file (default correlation_function_profile.json):
  the two boundary sweeps; the wall time of _line_pass (lines='rows') at max_distance 1, 2, 4 and the whole row, best of 3, with
  _correlation_pass on the same boundaries beside it; the flop count of each pass (the model of DESIGN section 12 on the actual bond
  dimensions) and the rate over wall time; and the batching comparison at a bulk cell: t1, one left step of tn_env3, against t64,
  one step of tn_env3_stack with 64 slots and no insertion (device time between two events, mean of 20 after 3 warm-up calls).
`analyse` is that of marginal_profile.py: the kernels after the pause, by total time."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from marginal_profile import analyse  # noqa: E402


def line_pass_flops(ins, reach):
    """Flops of the GEMMs of one _line_pass over the rows of the frame: the right sweep, and per cell k of the left sweep the
    1 + sum of nop over the start cells within `reach` slots that are stepped and closed (plus the nop insertions of the cell)."""
    tot = 0.0
    for ny in range(ins.Ny):
        top, bot = ins.rhoT[ny + 1].A, ins.rhoB[ny].A
        nops = [int(ins.sN[ny][nx]) for nx in range(ins.Nx)]
        for nx in range(ins.Nx):
            Dt, pd, Dt2 = top[nx].shape
            Db, pu, Db2 = bot[nx].shape
            bl = ins.lr[ny, nx - 1] if nx > 0 else 1
            br = ins.lr[ny, nx] if nx < ins.Nx - 1 else 1
            first, second, third = bl * pd * Dt2 * Db * Dt, Dt2 * Db * pu * bl * pd * br, br * Dt2 * Db2 * Db * pu
            right = br * Dt2 * Db * Db2 * pu + bl * pd * pu * br * Dt2 * Db + Dt * Db * pd * Dt2 * bl
            cell = bl * pd * pu * br * Dt2 * Db
            carried = 1 + sum(nops[max(0, nx - reach):nx])
            opened = nops[nx] if nx < ins.Nx - 1 else 0
            tot += 2.0 * (right + carried * (first + second + third + cell) + opened * (second + third))
    return tot


def _setup(beta=3.0, chi=64):
    import torch
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    torch.cuda.set_device(0)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, 20260004), beta=beta)
    kw = dict(graduate_truncation=True, Dmax=chi, tolS=1e-16, tolV=1e-10, max_sweeps=20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ins._setup_rhoT(**kw)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ins._setup_rhoB(**kw)
    torch.cuda.synchronize()
    return ins, t1 - t0, time.perf_counter() - t1


def _bulk_cell(ins, ny=8, nx=8):
    """(EL, At, W, Ab) of a bulk cell: the plain left environment carried there, and the cell's three sites."""
    import torch
    from tnac4o_amd import ops
    fac = ins._peps_factors_dev([(ny, x) for x in range(nx + 1)])
    At = [a.contiguous() for a in ins.rhoT[ny + 1].A]
    Ab = [a.contiguous() for a in ins.rhoB[ny].A]
    EL = torch.ones((1, 1, 1), dtype=torch.float64, device=At[0].device)
    for x in range(nx):
        F, dm, rm, pd, br = fac[x]
        EL, _ = ops.env3(0, EL, At[x], ops.mpo_from_factor(F, dm, rm, pd, br), Ab[x])
    F, dm, rm, pd, br = fac[nx]
    return EL, At[nx], ops.mpo_from_factor(F, dm, rm, pd, br), Ab[nx]


def _device_ms(fn, reps=20, warm=3):
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def step_comparison(ins, nE=64):
    import torch
    from tnac4o_amd import ops
    EL, At, W, Ab = _bulk_cell(ins)
    rng = torch.Generator(device='cpu').manual_seed(1)
    stack = torch.cat([EL[None], torch.randn((nE - 1,) + tuple(EL.shape), dtype=torch.float64, generator=rng).to(EL.device)]).contiguous()
    Wops = W[None].contiguous()
    t1 = _device_ms(lambda: ops.env3(0, EL, At, W, Ab))
    tn = _device_ms(lambda: ops.env3_stack(stack, At, Wops, Ab))
    th = _device_ms(lambda: ops.env3_stack(stack, At, Wops, Ab, keep_half=True))
    Dt, pd, Dt2 = At.shape
    bl, _, br, pu = W.shape
    Db, _, Db2 = Ab.shape
    gflop = 2e-9 * (bl * pd * Dt2 * Db * Dt + Dt2 * Db * pu * bl * pd * br + br * Dt2 * Db2 * Db * pu)
    return {'cell': [int(v) for v in (Dt, pd, Dt2, bl, br, pu, Db, Db2)], 'step_gflop': gflop, 't1_ms': t1, 'slots': nE, 't%d_ms' % nE: tn,
            't%d_keep_half_ms' % nE: th, 'ratio_t%d_over_%d_t1' % (nE, nE): tn / (nE * t1), 't1_tflops': gflop / t1,
            't%d_tflops' % nE: nE * gflop / tn}


def run(out_json='correlation_function_profile.json'):
    import torch
    ins, t_top, t_bot = _setup()
    res = {'rhoT_s': t_top, 'rhoB_s': t_bot, 'passes': {}}
    tc = []
    for _ in range(3):
        t0 = time.perf_counter()
        ins._correlation_pass()
        torch.cuda.synchronize()
        tc.append(1e3 * (time.perf_counter() - t0))
    res['correlation_pass_ms'] = min(tc)
    for reach in (1, 2, 4, None):
        ts = []
        for _ in range(4):                       # the first grows the workspace
            t0 = time.perf_counter()
            ins._line_pass(max_distance=reach)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        gflop = line_pass_flops(ins, ins.Nx - 1 if reach is None else reach) / 1e9
        res['passes']['full' if reach is None else str(reach)] = {'line_pass_ms': min(ts[1:]), 'runs_ms': ts, 'gflop': gflop,
                                                                  'tflops_wall': gflop / min(ts[1:])}
    res['step'] = step_comparison(ins)
    print(json.dumps(res))
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


def step():
    import torch
    from tnac4o_amd import ops
    ins, _, _ = _setup()
    EL, At, W, Ab = _bulk_cell(ins)
    stack = torch.cat([EL[None]] * 64).contiguous()
    Wops = W[None].contiguous()
    ops.env3_stack(stack, At, Wops, Ab)           # sizes the workspace
    torch.cuda.synchronize()
    time.sleep(1.0)                               # the gap `analyse` cuts the trace at
    ops.env3_stack(stack, At, Wops, Ab)
    torch.cuda.synchronize()


def once(reach=None):
    import torch
    ins, _, _ = _setup()
    ins._line_pass(max_distance=reach)            # sizes the workspace
    torch.cuda.synchronize()
    time.sleep(1.0)                               # the gap `analyse` cuts the trace at
    t0 = time.perf_counter()
    ins._line_pass(max_distance=reach)
    torch.cuda.synchronize()
    print(json.dumps({'line_pass_ms': 1e3 * (time.perf_counter() - t0),
                      'gflop': line_pass_flops(ins, ins.Nx - 1 if reach is None else reach) / 1e9}))


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(*(sys.argv[2:3]))
    elif sys.argv[1] == 'step':
        step()
    elif sys.argv[1] == 'once':
        once(int(sys.argv[2]) if len(sys.argv) > 2 else None)
    else:
        analyse(sys.argv[2], float(sys.argv[3]) if len(sys.argv) > 3 else None)
