"""The sampling phase of tnac4o.gibbs_sampling (host walk) and tnac4o.sample_boltzmann (tn_gibbs_sample) on one instance and one set
of boundaries, the boundary sweep excluded.

    python tools/sampling_profile.py run [OUT.json] [--n 8] [--chi 32] [--M 16384] [--betas 1,3] [--reps 3]
    python tools/sampling_profile.py once BETA [--n 8] [--chi 32] [--M 16384]      # sweep, a 1 s pause, one sample_boltzmann walk
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/sampling_profile.py once 3
    python tools/marginal_profile.py analyse OUT/.../run_kernel_trace.csv        # the kernels after the pause

`run`: synthetic_chimera(n, n, seed) at every beta: the boundaries rhoT are built once (timed apart); then, with the sweep switched
off, one warm-up run of each method and `reps` alternating repetitions, each on a fresh copy of the same uniform numbers, timed with
the host clock around a device synchronise.  Writes a JSON (default profiles/sampling_profile.json) with every repetition, the
spread, whether both methods drew the same configurations, and the largest number of distinct boundary rows the walk met."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260004
SWEEP = dict(graduate_truncation=True, tolS=1e-15, tolV=1e-10, max_sweeps=20)


def _opt(argv, name, default, cast):
    if name in argv:
        i = argv.index(name)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def _solver(n, beta, chi):
    """(solver with rhoT built and the sweep switched off for the calls that follow, seconds of the sweep)"""
    import torch
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=n, Ny=n, Nc=8, J=synthetic_chimera(n, n, SEED), beta=beta)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ins._setup_rhoT(Dmax=chi, **SWEEP)
    torch.cuda.synchronize()
    sweep_s = time.perf_counter() - t0
    ins._setup_rhoT = lambda **kw: None                  # both methods find the boundaries as they are
    return ins, sweep_s


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(out_json, n, chi, M, betas, reps):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    res = {'instance': 'synthetic_chimera(%d, %d, %d)' % (n, n, SEED), 'chi': chi, 'M': M, 'reps': reps, 'cases': []}
    for beta in betas:
        ins, sweep_s = _solver(n, beta, chi)
        np.random.seed(5)
        u = np.random.rand(n * n, M)                      # the numbers the host walk takes from numpy's global generator after seed(5)

        def host():
            np.random.seed(5)
            ins.gibbs_sampling(M=M, Dmax=chi)

        def walk():
            ins.sample_boltzmann(M=M, Dmax=chi, uniforms=u)

        _timed(host), _timed(walk)                       # warm-up
        th, tw = [], []
        for _ in range(reps):
            th.append(_timed(host))
            tw.append(_timed(walk))
        host()                                           # same numbers -> same configurations
        st_host, E_host = np.copy(ins.states), np.copy(ins.energy)
        walk()
        case = {'beta': beta, 'sweep_s': sweep_s, 'gibbs_sampling_s': th, 'sample_boltzmann_s': tw,
                'gibbs_sampling_median_s': float(np.median(th)), 'sample_boltzmann_median_s': float(np.median(tw)),
                'spread_s': float(max(np.ptp(th), np.ptp(tw))), 'speedup_median': float(np.median(th) / np.median(tw)),
                'faster_by_more_than_spread': bool(min(th) - max(tw) > max(np.ptp(th), np.ptp(tw))),
                'same_configurations': float(np.mean(np.all(st_host == ins.states, axis=1))),
                'max_energy_difference_of_equal_configurations': float(np.max(np.abs(E_host - ins.energy)[np.all(st_host == ins.states, axis=1)], initial=0.0)),
                'max_distinct_rows': int(ins.sample_max_groups), 'log2Z_lower': float(ins.log2Z_lower),
                'log2Z_estimate': float(ins.log2Z_estimate), 'sample_log2Z_spread': float(np.ptp(ins.sample_log2Z)),
                'negative_probability': float(ins.negative_probability)}
        print(json.dumps(case), flush=True)
        res['cases'].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


def once(beta, n, chi, M):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    ins, _ = _solver(n, beta, chi)
    u = np.random.default_rng(11).random((n * n, M))
    time.sleep(1.0)                                      # the gap `analyse` cuts the trace at
    print('sample_boltzmann: %.3f s' % _timed(lambda: ins.sample_boltzmann(M=M, Dmax=chi, uniforms=u)))


if __name__ == '__main__':
    argv = sys.argv[1:]
    n, chi, M = _opt(argv, '--n', 8, int), _opt(argv, '--chi', 32, int), _opt(argv, '--M', 2 ** 14, int)
    betas = _opt(argv, '--betas', [1.0, 3.0], lambda s: [float(x) for x in s.split(',')])
    reps = _opt(argv, '--reps', 3, int)
    if argv and argv[0] == 'once':
        once(float(argv[1]), n, chi, M)
    else:
        run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'sampling_profile.json'), n, chi, M, betas, reps)
