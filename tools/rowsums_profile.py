"""tn_pair_rowsums next to tn_pair_hist, in one process: wall time of each call on M = 2^14 and 2^16 rows of 2048 random bits, unit
weights, rows as given (no condensing).

    python tools/rowsums_profile.py [OUT.json] [--M 16384,65536] [--nbits 2048]

Every call is timed by device events around it on the current stream, median of 3 after a warm-up call (which sizes the workspace).
tn_pair_rowsums walks the full square of the pair matrix, tn_pair_hist its upper triangle: the expectation of DESIGN §26 is twice the
popcount work without the histogram's LDS atomics.  A record, no pass / fail number.  Writes a JSON (default
profiles/rowsums_profile.json) and prints the table of DESIGN §26."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _opt(argv, name, default, cast):
    if name in argv:
        i = argv.index(name)
        v = cast(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def _median_of(fn, reps=3):
    """(median, all) milliseconds of fn() by device events, after one warm-up call."""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(float(t0.elapsed_time(t1)))
    return sorted(out)[len(out) // 2], out


def run(out_json, Ms, nbits):
    import numpy as np
    import torch
    from tnac4o_amd import ops, overlap
    torch.cuda.set_device(0)
    nwords = -(-nbits // 64)
    res = {'nbits': nbits, 'nwords': nwords, 'weights': None, 'TN_PAIR_ROWSUMS_WGS': os.environ.get('TN_PAIR_ROWSUMS_WGS'),
           'TN_PAIR_HIST_WGS': os.environ.get('TN_PAIR_HIST_WGS'), 'device': torch.cuda.get_device_name(0), 'cases': []}
    for M in Ms:
        rows = torch.as_tensor(np.random.default_rng(1).integers(0, 2 ** 63, (M, nwords), dtype=np.int64)).cuda()
        hist_ms, hist_all = _median_of(lambda: ops.pair_hist(rows, nbits))
        sums_ms, sums_all = _median_of(lambda: ops.pair_rowsums(rows, nbits))
        hist = overlap.limbs_to_int(ops.pair_hist(rows, nbits).cpu().numpy())
        R = overlap.rowsums_to_int(ops.pair_rowsums(rows, nbits).cpu().numpy())
        for k in range(5):                                             # the two kernels hold the same integers
            assert sum(r[k] for r in R) == 2 * sum(h * d ** k for d, h in enumerate(hist)), k
        case = {'M': M, 'pair_hist_ms': hist_ms, 'pair_hist_all_ms': hist_all, 'pair_rowsums_ms': sums_ms, 'pair_rowsums_all_ms': sums_all,
                'ratio': sums_ms / hist_ms, 'ordered_pairs_per_s': M * (M - 1) / (sums_ms * 1e-3),
                'pair_hist_pairs_per_s': M * (M - 1) / 2.0 / (hist_ms * 1e-3)}
        print(json.dumps(case), flush=True)
        res['cases'].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, 'w') as f:
        json.dump(res, f, indent=1)
    print('| M | `tn_pair_hist` | `tn_pair_rowsums` | ratio |\n|---|---|---|---|')
    for c in res['cases']:
        print('| %d | %.2f ms | %.2f ms | %.2f |' % (c['M'], c['pair_hist_ms'], c['pair_rowsums_ms'], c['ratio']))


if __name__ == '__main__':
    argv = sys.argv[1:]
    Ms = _opt(argv, '--M', [2 ** 14, 2 ** 16], lambda s: [int(x) for x in s.split(',')])
    nbits = _opt(argv, '--nbits', 2048, int)
    run(argv[0] if argv else os.path.join(ROOT, 'profiles', 'rowsums_profile.json'), Ms, nbits)
