"""tn_pair_hist at M = 2^16: wall time on random rows, on identical rows (every pair in one bin) and on the samples of a droplet
L = 2048 sample_boltzmann run, against the popcount model of DESIGN §13.

    python tools/overlap_profile.py run [OUT.json] [--M 65536] [--nbits 2048] [--chi 32] [--beta 3] [--no-droplet]
    python tools/overlap_profile.py once [random|identical] [--M 65536] [--nbits 2048]       # a 1 s pause, then one call
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/overlap_profile.py once random

`run`: every case is timed with the host clock around a device synchronise, best of 3 after a warm-up call, on the rows as given
(no condensing); the droplet case also reports the time of calculate_overlap_distribution('spin'), which condenses first, and the
number of distinct rows.  The model: pairs x nwords 64-bit XOR + popcount, four 32-bit VALU operations each, against 256 compute
units x 4 SIMDs x 32 lanes x the clock (2.4 GHz).  Writes a JSON (default profiles/overlap_profile.json)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CLOCK_HZ = 2.4e9
VALU_LANES = 256 * 4 * 32          # compute units x SIMDs x lanes per clock


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


def model_seconds(M, nwords):
    """pairs x nwords x (2 XOR + 2 popcount-accumulate on 32-bit halves) at the VALU rate"""
    return M * (M - 1) / 2.0 * nwords * 4.0 / (VALU_LANES * CLOCK_HZ)


def _rows(kind, M, nbits):
    import numpy as np
    import torch
    nwords = -(-nbits // 64)
    rng = np.random.default_rng(1)
    rows = rng.integers(0, 2 ** 63, (M, nwords), dtype=np.int64)
    if kind == 'identical':
        rows[:] = rows[0]
    return torch.as_tensor(rows).cuda()


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


def _case(name, d_rows, nbits):
    from tnac4o_amd import ops, overlap
    M, nwords = int(d_rows.shape[0]), -(-nbits // 64)
    best, times = _best_of(lambda: ops.pair_hist(d_rows, nbits))
    hist = overlap.limbs_to_int(ops.pair_hist(d_rows, nbits).cpu().numpy())
    assert sum(hist) == M * (M - 1) // 2
    mod = model_seconds(M, nwords)
    case = {'case': name, 'M': M, 'nbits': nbits, 'nwords': nwords, 'best_s': best, 'times_s': times, 'model_s': mod,
            'fraction_of_model': mod / best, 'pairs_per_s': M * (M - 1) / 2.0 / best, 'bins_hit': sum(1 for h in hist if h)}
    print(json.dumps(case), flush=True)
    return case


def run(out_json, M, nbits, chi, beta, droplet):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    res = {'cases': []}
    for kind in ('random', 'identical'):
        res['cases'].append(_case(kind, _rows(kind, M, nbits), nbits))
    res['contention_cost'] = res['cases'][1]['best_s'] / res['cases'][0]['best_s']
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
        rows = overlap.pack_bits(overlap.spin_bits(ins))
        case = _case('droplet2048', torch.as_tensor(rows.view(np.int64)).cuda(), ins.active)
        t0 = time.perf_counter()
        ins.calculate_overlap_distribution('spin')
        torch.cuda.synchronize()
        case.update(sample_boltzmann_s=sample_s, calculate_overlap_distribution_s=time.perf_counter() - t0,
                    distinct_rows=int(np.unique(rows, axis=0).shape[0]), chi=chi, beta=beta, q2=ins.overlap_moments['q2'],
                    binder=ins.overlap_moments['binder'])
        print(json.dumps(case), flush=True)
        res['cases'].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


def once(kind, M, nbits):
    import torch
    from tnac4o_amd import ops
    torch.cuda.set_device(0)
    d_rows = _rows(kind, M, nbits)
    ops.pair_hist(d_rows[:256], nbits)                     # loads the code object
    torch.cuda.synchronize()
    time.sleep(1.0)
    t0 = time.perf_counter()
    ops.pair_hist(d_rows, nbits)
    torch.cuda.synchronize()
    print('tn_pair_hist (%s, M = %d, nbits = %d): %.3f ms' % (kind, M, nbits, 1e3 * (time.perf_counter() - t0)))


if __name__ == '__main__':
    argv = sys.argv[1:]
    M, nbits = _opt(argv, '--M', 2 ** 16, int), _opt(argv, '--nbits', 2048, int)
    chi, beta = _opt(argv, '--chi', 32, int), _opt(argv, '--beta', 3.0, float)
    no_droplet = _flag(argv, '--no-droplet')
    if argv and argv[0] == 'once':
        once(argv[1] if len(argv) > 1 else 'random', M, nbits)
    else:
        run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'overlap_profile.json'), M, nbits, chi, beta, not no_droplet)
