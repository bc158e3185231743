"""The marginal pass of tnac4o.calculate_marginals on the bench instance (synthetic chimera, L = 2048, beta = 3, chi = 64).

    python tools/marginal_profile.py run                      # boundaries, a 1 s pause, then the marginal pass once
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/marginal_profile.py run
    python tools/marginal_profile.py analyse OUT/.../run_kernel_trace.csv

`run` prints the pass's wall time and its flop count (the model of DESIGN §9, evaluated on the actual bond dimensions) and writes
it to a JSON file (default marginal_profile.json).  `analyse` keeps the kernels launched after the pause (the longest gap in the
trace) and prints their summed duration, launches, the kernels by total time and the achieved fp64 rate."""
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pass_flops(ins):
    """Flops of the GEMMs of one marginal pass (both environment sweeps and the cell products) on the boundaries as they are."""
    tot = 0.0
    for ny in range(ins.Ny):
        top, bot = ins.rhoT[ny + 1].A, ins.rhoB[ny].A
        for nx in range(ins.Nx):
            Dt, pd, Dt2 = top[nx].shape
            Db, pu, Db2 = bot[nx].shape
            bl = ins.lr[ny, nx - 1] if nx > 0 else 1
            br = ins.lr[ny, nx] if nx < ins.Nx - 1 else 1
            left = bl * pd * Dt2 * Db * Dt + Dt2 * Db * pu * bl * pd * br + br * Dt2 * Db2 * Db * pu
            right = br * Dt2 * Db * Db2 * pu + bl * pd * pu * br * Dt2 * Db + Dt * Db * pd * Dt2 * bl
            cell = bl * pd * pu * br * Dt2 * Db
            tot += 2.0 * (left + right + cell)
    return tot


def run(out_json='marginal_profile.json'):
    import torch
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    torch.cuda.set_device(0)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, 20260004), beta=3.0)
    kw = dict(graduate_truncation=True, Dmax=64, tolS=1e-16, tolV=1e-10, max_sweeps=20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ins._setup_rhoT(**kw)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ins._setup_rhoB(**kw)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    time.sleep(1.0)                       # the gap `analyse` cuts the trace at
    t3 = time.perf_counter()
    ins._marginal_pass()
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    res = {'rhoT_s': t1 - t0, 'rhoB_s': t2 - t1, 'pass_ms': 1e3 * (t4 - t3), 'pass_gflop': pass_flops(ins) / 1e9}
    res['pass_tflops_wall'] = res['pass_gflop'] / res['pass_ms']
    print(json.dumps(res))
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


def analyse(trace_csv, gflop=None):
    rows = []
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    rows.sort()
    gaps = [(rows[i + 1][0] - rows[i][1], i + 1) for i in range(len(rows) - 1)]
    _, cut = max(gaps)
    tail = rows[cut:]
    busy = sum(e - s for s, e, _ in tail) / 1e6
    span = (tail[-1][1] - tail[0][0]) / 1e6
    by = {}
    for s, e, n in tail:
        k = n.split('(')[0][:80]
        c, t = by.get(k, (0, 0.0))
        by[k] = (c + 1, t + (e - s) / 1e6)
    print('marginal pass: %d launches, kernel time %.2f ms, first-to-last %.2f ms' % (len(tail), busy, span))
    for k, (c, t) in sorted(by.items(), key=lambda kv: -kv[1][1])[:12]:
        print('  %8.3f ms  %6d  %s' % (t, c, k))
    if gflop:
        print('achieved %.2f TFLOP/s over kernel time (%.1f GFLOP)' % (gflop / busy, gflop))


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        run(*(sys.argv[2:3]))
    else:
        analyse(sys.argv[2], float(sys.argv[3]) if len(sys.argv) > 3 else None)
