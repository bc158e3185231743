"""tn_spin_moments at N = 2048 bits and K = 2^16 rows: wall time on random rows with one weight plane (no weights) and with 32
(random 32-bit weights), and on the samples of a droplet L = 2048 sample_boltzmann run, against the cost model of DESIGN §17; for
scale, the float64 product S^T diag(w) S of the same shape through numpy.

    python tools/spin_moments_profile.py run [OUT.json] [--M 65536] [--N 2048] [--chi 32] [--beta 3] [--no-droplet] [--no-numpy]
    python tools/spin_moments_profile.py once [--M 65536] [--N 2048] [--planes 1|32]            # a 1 s pause, then one call
    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- python tools/spin_moments_profile.py once

`run`: every case is timed with the host clock around a device synchronise, best of 3 after a warm-up call, on the rows as given
(no condensing); the droplet case also reports the time of calculate_sample_correlations, which condenses first, and the number of
distinct rows.  The model: N^2 / 2 pairs of bits x ceil(K / 64) words x (5 P + 2) 32-bit lane operations (per plane two ANDs, two
popcount-accumulates and the doubling of Horner's rule; two XORs per word) against 256 compute units x 4 SIMDs x 32 lanes x the
clock (2.4 GHz); the transposition is not in it.  The JSON (default profiles/spin_moments_profile.json) is rewritten after every
case."""
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


def model_seconds(M, N, P):
    return N * N / 2.0 * -(-M // 64) * (5.0 * P + 2.0) / (VALU_LANES * CLOCK_HZ)


def _rows(M, N):
    import numpy as np
    import torch
    return torch.as_tensor(np.random.default_rng(1).integers(-2 ** 63, 2 ** 63, (M, -(-N // 64)), dtype=np.int64)).cuda()


def _weights(M, P):
    import numpy as np
    import torch
    if P == 1:
        return None, 1
    w = np.random.default_rng(2).integers(0, 2 ** P, M, dtype=np.uint64).astype(np.uint32)
    return torch.as_tensor(w.view(np.int32)).cuda(), 2 ** P - 1


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


def _case(name, d_rows, N, P):
    from tnac4o_amd import ops
    M = int(d_rows.shape[0])
    d_w, wmax = _weights(M, P)
    best, times = _best_of(lambda: ops.spin_moments(d_rows, N, d_w, wmax))
    out = ops.spin_moments(d_rows, N, d_w, wmax).cpu().numpy()
    total = M if d_w is None else int(d_w.cpu().numpy().view('uint32').astype('uint64').sum())
    assert int(out[N, N + 1]) == total and not out.diagonal().any()
    model = model_seconds(M, N, P)
    case = {'case': name, 'M': M, 'N': N, 'planes': P, 'best_s': best, 'times_s': times, 'model_s': model, 'fraction_of_model': model / best,
            'word_pairs_per_s': N * N / 2.0 * -(-M // 64) / best}
    print(json.dumps(case), flush=True)
    return case


def _write(out_json, res):
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


def run(out_json, M, N, chi, beta, droplet, with_numpy):
    import numpy as np
    import torch
    torch.cuda.set_device(0)
    res = {'cases': []}
    for P in (1, 32):
        res['cases'].append(_case('random, %d plane%s' % (P, '' if P == 1 else 's'), _rows(M, N), N, P))
        _write(out_json, res)
    if with_numpy:                                         # for scale only: the +-1 product on the host, float64, the BLAS threads of the process
        rng = np.random.default_rng(3)
        S = 2.0 * rng.integers(0, 2, (M, N)).astype(np.float64) - 1.0
        w = rng.random(M)
        t0 = time.perf_counter()
        C = (S.T * w) @ S
        host_s = time.perf_counter() - t0
        res['numpy_float64'] = {'M': M, 'N': N, 'seconds': host_s, 'threads': int(os.environ.get('OMP_NUM_THREADS', '0')) or None, 'trace': float(np.trace(C))}
        print(json.dumps(res['numpy_float64']), flush=True)
        del S, C
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
        rows = overlap.pack_bits(overlap.spin_bits(ins))
        case = _case('droplet2048', torch.as_tensor(rows.view(np.int64)).cuda(), int(ins.active), 1)
        t0 = time.perf_counter()
        ins.calculate_sample_correlations()
        torch.cuda.synchronize()
        case.update(sample_boltzmann_s=sample_s, calculate_sample_correlations_s=time.perf_counter() - t0,
                    distinct_rows=int(np.unique(rows, axis=0).shape[0]), chi=chi, beta=beta, chi_sg_00=float(ins.sample_chi_sg[0, 0]),
                    chi_sg_10=float(ins.sample_chi_sg[1, 0]), chi_sg_01=float(ins.sample_chi_sg[0, 1]))
        print(json.dumps(case), flush=True)
        res['cases'].append(case)
        _write(out_json, res)


def once(M, N, P):
    import torch
    from tnac4o_amd import ops
    torch.cuda.set_device(0)
    d_rows = _rows(M, N)
    d_w, wmax = _weights(M, P)
    ops.spin_moments(d_rows[:256], N, None if d_w is None else d_w[:256].contiguous(), wmax)       # loads the code object
    torch.cuda.synchronize()
    time.sleep(1.0)
    t0 = time.perf_counter()
    ops.spin_moments(d_rows, N, d_w, wmax)
    torch.cuda.synchronize()
    print('tn_spin_moments (M = %d, N = %d, %d planes): %.3f ms' % (M, N, P, 1e3 * (time.perf_counter() - t0)))


if __name__ == '__main__':
    argv = sys.argv[1:]
    M, N, P = _opt(argv, '--M', 2 ** 16, int), _opt(argv, '--N', 2048, int), _opt(argv, '--planes', 1, int)
    chi, beta = _opt(argv, '--chi', 32, int), _opt(argv, '--beta', 3.0, float)
    no_droplet, no_numpy = _flag(argv, '--no-droplet'), _flag(argv, '--no-numpy')
    if argv and argv[0] == 'once':
        once(M, N, P)
    else:
        run(argv[1] if len(argv) > 1 else os.path.join(ROOT, 'profiles', 'spin_moments_profile.json'), M, N, chi, beta, not no_droplet, not no_numpy)
