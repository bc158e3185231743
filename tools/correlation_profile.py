"""The correlation pass of tnac4o.calculate_correlations on the bench instance (synthetic chimera, L = 2048, beta = 3, chi = 64).

    python tools/correlation_profile.py run                    # boundaries, a 1 s pause, then the correlation pass once
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/correlation_profile.py run
    python tools/correlation_profile.py analyse OUT/.../run_kernel_trace.csv [GFLOP]

`run` prints the pass's wall time, best of 3 after the first, with the marginal pass on the same boundaries beside it, and its flop
count (the GEMMs are those of the marginal pass: tools/marginal_profile.py), and writes them to a JSON file (default
correlation_profile.json).  `analyse` (that of marginal_profile.py) keeps the kernels after the pause; for a trace of exactly one
correlation pass, give `run --once` (no repeats, no marginal pass)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from marginal_profile import analyse, pass_flops  # noqa: E402


def run(out_json='correlation_profile.json', once=False):
    import torch
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    torch.cuda.set_device(0)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, 20260004), beta=3.0)
    kw = dict(graduate_truncation=True, Dmax=64, tolS=1e-16, tolV=1e-10, max_sweeps=20)
    ins._setup_rhoT(**kw)
    ins._setup_rhoB(**kw)
    torch.cuda.synchronize()
    time.sleep(1.0)                       # the gap `analyse` cuts the trace at
    t0 = time.perf_counter()
    ins._correlation_pass()
    torch.cuda.synchronize()
    res = {'first_pass_ms': 1e3 * (time.perf_counter() - t0), 'pass_gflop': pass_flops(ins) / 1e9}
    if not once:
        tc, tm = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            ins._correlation_pass()
            torch.cuda.synchronize()
            tc.append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            ins._marginal_pass()
            torch.cuda.synchronize()
            tm.append(1e3 * (time.perf_counter() - t0))
        res.update(correlation_pass_ms=min(tc), marginal_pass_ms=min(tm), correlation_runs_ms=tc, marginal_runs_ms=tm)
    print(json.dumps(res))
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    if sys.argv[1] == 'run':
        args = [a for a in sys.argv[2:] if a != '--once']
        run(*(args[:1]), once='--once' in sys.argv[2:])
    else:
        analyse(sys.argv[2], float(sys.argv[3]) if len(sys.argv) > 3 else None)
