"""tn_pair_moments at M = 2^16, G = 16, wpg = 2: wall time on random rows and on the samples of a droplet L = 2048 sample_boltzmann
run (16 lattice columns of 128 spins: the same G and wpg), against the cost model of DESIGN §16.

    python tools/overlap_corr_profile.py run [OUT.json] [--M 65536] [--G 16] [--wpg 2] [--chi 32] [--beta 3] [--no-droplet]
    python tools/overlap_corr_profile.py once [--M 65536] [--G 16] [--wpg 2]                   # a 1 s pause, then one call
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/overlap_corr_profile.py once

`run`: every case is timed with the host clock around a device synchronise, best of 3 after a warm-up call, on the rows as given
(no condensing); the droplet case also reports the time of calculate_overlap_correlations('x', 'spin'), which condenses first, and
the number of distinct rows.  The model: per pair (G+1)(G+2)/2 elements at 8 VALU operations each (per two pairs and element the
loop issues 16: two 16-bit products, four 32 x 32 -> 64-bit multiply-adds, two 64-bit adds, addresses) plus G wpg 64-bit XOR +
popcount at 4 operations each, against 256 compute units x 4 SIMDs x 32 lanes x the clock (2.4 GHz).  The JSON (default
profiles/overlap_corr_profile.json) is rewritten after every case."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CLOCK_HZ = 2.4e9
VALU_LANES = 256 * 4 * 32          # compute units x SIMDs x lanes per clock
OPS_PER_ELEMENT = 8.0              # VALU operations per pair and element of the phase-2 loop
OPS_PER_WORD = 4.0                 # 2 XOR + 2 popcount-accumulate on 32-bit halves


def _opt(argv, name, default, cast):
    if name in argv:
        i = argv.index(name)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def _flag(argv, name):
    if name in argv:
        argv.remove(name)
        return True
    return False


def model_seconds(M, G, wpg):
    """(moments part, popcount part) in seconds at the VALU rate"""
    pairs = M * (M - 1) / 2.0
    rate = VALU_LANES * CLOCK_HZ
    return pairs * (G + 1) * (G + 2) / 2.0 * OPS_PER_ELEMENT / rate, pairs * G * wpg * OPS_PER_WORD / rate


def _rows(M, G, wpg):
    import numpy as np
    import torch
    return torch.as_tensor(np.random.default_rng(1).integers(0, 2 ** 63, (M, G * wpg), dtype=np.int64)).cuda()


def _best_of(fn, reps=3):
    import torch
    fn()                                                   # warm-up: sizes the workspace
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return min(out), out


def _case(name, d_rows, G, wpg):
    from tnac4o_amd import ops, overlap
    M = int(d_rows.shape[0])
    best, times = _best_of(lambda: ops.pair_moments(d_rows, G, wpg))
    out = ops.pair_moments(d_rows, G, wpg).cpu().numpy()
    assert overlap.limbs_to_int(out[G, G].reshape(1, 2))[0] == M * (M - 1) // 2
    mom, pop = model_seconds(M, G, wpg)
    case = {'case': name, 'M': M, 'G': G, 'wpg': wpg, 'best_s': best, 'times_s': times, 'model_moments_s': mom, 'model_popcount_s': pop,
            'fraction_of_model': (mom + pop) / best, 'pairs_per_s': M * (M - 1) / 2.0 / best,
            'multiply_adds_per_s': M * (M - 1) / 2.0 * (G + 1) * (G + 2) / 2.0 / best}
    print(json.dumps(case), flush=True)
    return case


def _write(out_json, res):
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


def run(out_json, M, G, wpg, chi, beta, droplet):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    res = {'cases': [_case('random', _rows(M, G, wpg), G, wpg)]}
    _write(out_json, res)
    if droplet:
        import golden_inputs as gi
        import tnac4o_amd
        from tnac4o_amd import overlap
        ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=gi.droplet_J(2048, 1), beta=beta)
        np.random.seed(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ins.sample_boltzmann(M=M, Dmax=chi)
        torch.cuda.synchronize()
        sample_s = time.perf_counter() - t0
        group, sizes = overlap.line_groups(ins, 'x', 'spin')
        rows, w = overlap.pack_groups(overlap.spin_bits(ins), group, sizes.size, False)
        case = _case('droplet2048', torch.as_tensor(rows.view(np.int64)).cuda(), int(sizes.size), w)
        t0 = time.perf_counter()
        ins.calculate_overlap_correlations('x', 'spin')
        torch.cuda.synchronize()
        case.update(sample_boltzmann_s=sample_s, calculate_overlap_correlations_s=time.perf_counter() - t0,
                    distinct_rows=int(np.unique(rows, axis=0).shape[0]), chi=chi, beta=beta, chi_k=[float(x) for x in ins.overlap_chi['x']],
                    xi_over_L=float(ins.overlap_xi_over_L['x']))
        print(json.dumps(case), flush=True)
        res['cases'].append(case)
        _write(out_json, res)


def once(M, G, wpg):
    import torch
    from tnac4o_amd import ops
    torch.cuda.set_device(0)
    d_rows = _rows(M, G, wpg)
    ops.pair_moments(d_rows[:256], G, wpg)                 # loads the code object
    torch.cuda.synchronize()
    time.sleep(1.0)
    t0 = time.perf_counter()
    ops.pair_moments(d_rows, G, wpg)
    torch.cuda.synchronize()
    print('tn_pair_moments (M = %d, G = %d, wpg = %d): %.3f ms' % (M, G, wpg, 1e3 * (time.perf_counter() - t0)))


if __name__ == '__main__':
    argv = sys.argv[1:]
    M, G, wpg = _opt(argv, '--M', 2 ** 16, int), _opt(argv, '--G', 16, int), _opt(argv, '--wpg', 2, int)
    chi, beta = _opt(argv, '--chi', 32, int), _opt(argv, '--beta', 3.0, float)
    no_droplet = _flag(argv, '--no-droplet')
    if argv and argv[0] == 'once':
        once(M, G, wpg)
    else:
        run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'overlap_corr_profile.json'), M, G, wpg, chi, beta, not no_droplet)
