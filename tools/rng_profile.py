"""What the device generator (tn_uniforms, seed= of the Monte Carlo calls) saves against uniform numbers drawn by numpy on
the host and uploaded, which is what the calls do with seed=None.

    python tools/rng_profile.py [OUT.json] [--M 16384] [--reps 3] [--rounds 4]

Every figure is the median of `reps` timed runs after one warm-up run on one MI355X.
(a) fill       tn_uniforms into a (256, M) float64 tensor (the numbers of one sweep of 256 cells over M rows; M = 2^14: 32 MiB),
               device events around the call; beside it np.random.rand(256, M) and its upload as the calls make it
               (torch.as_tensor(...).to(device)), device events and the host clock around both (the stream is idle while numpy draws);
               and tn_uniforms of the (15 * 256, M) numbers of one whole call of (b), 480 MiB, past the caches.
(b) anneal     the host clock around tnac4o.anneal_population at the timing shape of DESIGN §21 -- synthetic_chimera(16, 16, seed),
               256 cells of Nc = 8, K = 16 betas from 0 to 1.6, a fresh population of M rows, one sweep per step -- ending in a device
               synchronise, with seed= and with seed=None (numpy's global generator, the call as it was before seed= existed).
(c) temper     the same pair for tnac4o.temper_samples at the shape of DESIGN §20: the same instance, T = 16 betas from 0.1 to 1.6,
               M rows = M / 16 chains, `rounds` rounds of one sweep, cluster moves at every temperature.
No number here is a pass / fail condition.  Writes a JSON (default profiles/rng_profile.json)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20260023
NCELL = 256


def _opt(argv, name, default, cast):
    if name in argv:
        i = argv.index(name)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def timed(fn, reps):
    """([ms by device events], [ms by the host clock]) of `reps` runs of fn() after one warm-up run; every run ends synchronised."""
    import torch
    ev, wall = [], []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if rep:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return ev, wall


def stats(ms):
    import numpy as np
    return {'ms': ms, 'ms_median': float(np.median(ms)), 'spread_ms': float(np.ptp(ms))}


def fill(res, M, reps):
    import numpy as np
    import torch
    from tnac4o_amd import ops
    dev = torch.device('cuda', 0)
    out = torch.empty((NCELL, M), dtype=torch.float64, device=dev)
    keep = {}

    def host():
        keep['u'] = torch.as_tensor(np.ascontiguousarray(np.random.rand(NCELL, M))).to(dev)

    np.random.seed(SEED)
    ev_d, wall_d = timed(lambda: ops.uniforms(SEED, 5 << 56, 0, NCELL, M, out=out), reps)
    ev_h, wall_h = timed(host, reps)
    nbytes = NCELL * M * 8
    res['fill'] = {'what': 'tn_uniforms of (%d, %d) float64 (%d bytes) against np.random.rand of that shape and its upload; median of %d after a warm-up'
                           % (NCELL, M, nbytes, reps),
                   'tn_uniforms_device_events': stats(ev_d), 'tn_uniforms_host_clock': stats(wall_d),
                   'numpy_and_upload_device_events': stats(ev_h), 'numpy_and_upload_host_clock': stats(wall_h)}
    res['fill']['tn_uniforms_GB_per_s'] = nbytes / (res['fill']['tn_uniforms_device_events']['ms_median'] * 1e-3) / 1e9
    res['fill']['ratio_host_to_device'] = res['fill']['numpy_and_upload_host_clock']['ms_median'] / res['fill']['tn_uniforms_device_events']['ms_median']
    # the numbers of one whole call of (b): 15 steps of 256 cells, past the caches
    steps = 15
    big = torch.empty((steps * NCELL, M), dtype=torch.float64, device=dev)
    ev_b, _ = timed(lambda: ops.uniforms(SEED, 11 << 56, 0, steps * NCELL, M, out=big), reps)
    res['fill']['tn_uniforms_%dx%d' % (steps * NCELL, M)] = dict(stats(ev_b), bytes=steps * nbytes,
                                                                  GB_per_s=steps * nbytes / (float(np.median(ev_b)) * 1e-3) / 1e9)
    del big
    print(json.dumps(res['fill']), flush=True)


def _instance():
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    return tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, SEED), beta=1.0)


def anneal(res, M, reps):
    import numpy as np
    K = 16
    betas = np.linspace(0.0, 1.6, K)
    ins = _instance()
    np.random.seed(SEED)
    _, seeded = timed(lambda: ins.anneal_population(betas, sweeps=1, M=M, seed=SEED), reps)
    _, host = timed(lambda: ins.anneal_population(betas, sweeps=1, M=M), reps)
    res['anneal_population'] = {'what': 'host clock around anneal_population (synchronised), chimera 16x16 cells, Nc = 8, K = %d betas 0 .. 1.6, a fresh '
                                        'population of M = %d, one sweep per step: %d steps, %d uniform numbers; median of %d after a warm-up'
                                        % (K, M, K - 1, (K - 1) * (NCELL * M + 1) + M * NCELL, reps),
                                'seed': stats(seeded), 'seed_none': stats(host)}
    a = res['anneal_population']
    a['ms_per_step'] = {'seed': a['seed']['ms_median'] / (K - 1), 'seed_none': a['seed_none']['ms_median'] / (K - 1)}
    a['ratio_seed_none_to_seed'] = a['seed_none']['ms_median'] / a['seed']['ms_median']
    print(json.dumps(a), flush=True)


def temper(res, M, reps, rounds):
    import numpy as np
    T = 16
    betas = np.linspace(0.1, 1.6, T)
    ins = _instance()
    start = np.random.default_rng(SEED).integers(0, 256, (M, NCELL))

    def run(**kw):
        ins.states = start
        ins.temper_samples(betas, rounds=rounds, sweeps=1, **kw)

    np.random.seed(SEED)
    _, seeded = timed(lambda: run(seed=SEED), reps)
    _, host = timed(run, reps)
    res['temper_samples'] = {'what': 'host clock around temper_samples (synchronised), chimera 16x16 cells, Nc = 8, T = %d betas 0.1 .. 1.6, M = %d rows = %d '
                                     'chains, %d rounds of one sweep, cluster moves at every temperature; median of %d after a warm-up'
                                     % (T, M, M // T, rounds, reps),
                             'seed': stats(seeded), 'seed_none': stats(host)}
    a = res['temper_samples']
    a['ms_per_round'] = {'seed': a['seed']['ms_median'] / rounds, 'seed_none': a['seed_none']['ms_median'] / rounds}
    a['ratio_seed_none_to_seed'] = a['seed_none']['ms_median'] / a['seed']['ms_median']
    print(json.dumps(a), flush=True)


def run(out_json, M, reps, rounds):
    import torch
    assert torch.cuda.is_available(), 'rng_profile needs a GPU'
    torch.cuda.set_device(0)
    res = {}
    fill(res, M, reps)
    anneal(res, M, reps)
    temper(res, M, reps, rounds)
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    argv = sys.argv[1:]
    M, reps, rounds = _opt(argv, '--M', 2 ** 14, int), _opt(argv, '--reps', 3, int), _opt(argv, '--rounds', 4, int)
    run(argv[0] if argv else os.path.join(ROOT, 'profiles', 'rng_profile.json'), M, reps, rounds)
