"""One call of the factorisation per path of the tn_qr host driver (qr_factor_impl in csrc/qr.hip) at the smallest shape that reaches
the path, with fixed seeds: tiny, one-launch, the same through the blocked path, folded last panel, merged reflectors, panel by panel,
two-level, 64-wide, rank-revealing exit, pivoted site factorisation with device and with host selection -- row-major and column-major
where the entry point allows, TN_QR_RANK_UPDATE at 1 and 0 where the driver reads it.  Every output (Q, R, keff, permutation, dropped2)
goes into one .npz, so that two builds can be compared bit for bit; under `rocprofv3 --kernel-trace` the run gives the launches of
every path in order.
Usage: qr_paths.py run OUT.npz                      one run (fresh process per build)
       qr_paths.py compare A.npz B.npz              numpy.array_equal of every array
       qr_paths.py launches A.csv B.csv             kernel name, grid, workgroup and LDS size of two kernel traces, line by line
                                                    (without the runtime's own copy kernels)"""
import csv
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# name, m, n, nb, rank (None: full), rank_tol, switches, layouts, does the path read TN_QR_RANK_UPDATE
QR_PATHS = [
    ('tiny', 31, 1, 32, None, 0.0, {}, 'rc', False),
    ('one_launch', 300, 64, 32, None, 0.0, {}, 'rc', False),
    ('one_launch_shape_blocked', 300, 64, 32, None, 0.0, {'TN_QR_SMALL': '0'}, 'rc', True),
    ('folded_last_panel', 300, 96, 32, None, 0.0, {}, 'rc', True),
    ('merged_reflectors', 1400, 96, 32, None, 0.0, {}, 'rc', True),
    ('panel_by_panel', 1400, 96, 32, None, 0.0, {'TN_QR_MERGED_Q': '0'}, 'rc', True),
    ('two_level', 512, 256, 32, None, 0.0, {'TN_QR_NBO': '128'}, 'rc', True),
    ('wide_64', 300, 257, 64, None, 0.0, {}, 'rc', False),
    ('rank_revealing_exit', 200, 100, 32, 20, 1e-10, {}, 'rc', True),
]
SITE_PATHS = [('pivoted_device', '1'), ('pivoted_host', '0')]      # ops.site_qr on 96 x 80 of rank 40, TN_PIVOT_DEVICE


def with_env(env, fn):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                      # (the library reads these switches per call)
    try:
        return fn()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(out_path):
    import torch
    from tnac4o_amd import ops
    out = {}
    for i, (name, m, n, nb, rank, tol, env, layouts, reads_ru) in enumerate(QR_PATHS):
        rng = np.random.default_rng(1000 + i)
        A = rng.standard_normal((m, n)) if rank is None else rng.standard_normal((m, rank)) @ rng.standard_normal((rank, n))
        for layout in layouts:
            T = torch.from_numpy(A).cuda() if layout == 'r' else torch.from_numpy(np.ascontiguousarray(A.T)).cuda().t()
            for ru in (('1', '0') if reads_ru else ('1',)):
                k = min(m, n)
                Q = torch.empty((m, k), dtype=torch.float64, device='cuda')
                R = torch.empty((k, n), dtype=torch.float64, device='cuda')
                _, _, keff = with_env(dict(env, TN_QR_RANK_UPDATE=ru), lambda: ops.qr_into(T, Q, R, nb=nb, rank_tol=tol))
                torch.cuda.synchronize()
                key = '%s/%s/ru%s/' % (name, 'rowmajor' if layout == 'r' else 'colmajor', ru)
                out[key + 'Q'], out[key + 'R'] = Q[:, :keff].cpu().numpy(), R[:keff].cpu().numpy()      # (nothing is written behind keff)
                out[key + 'keff'] = np.int64(keff)
                print('%-60s keff %d' % (key, keff), flush=True)
    rng = np.random.default_rng(2000)
    B = rng.standard_normal((96, 40)) @ rng.standard_normal((40, 80))
    for name, mode in SITE_PATHS:
        for ru in ('1', '0'):
            info = {}
            A3 = torch.from_numpy(B).cuda().view(48, 2, 80).clone()      # side 0: the (Dl p) x Dr matrix, consumed by the call
            Q, R, k, _ = with_env({'TN_PIVOT_DEVICE': mode, 'TN_QR_RANK_UPDATE': ru},
                                  lambda: ops.site_qr(0, A3, None, rank_tol=1e-10, normalise=False, info=info, pivot=True))
            torch.cuda.synchronize()
            key = '%s/ru%s/' % (name, ru)
            out[key + 'Q'], out[key + 'R'], out[key + 'keff'] = Q.cpu().numpy(), R.cpu().numpy(), np.int64(k)
            out[key + 'perm'], out[key + 'dropped2'] = info['perm'].cpu().numpy(), np.float64(info['dropped2'])
            print('%-60s keff %d dropped2 %.3e' % (key, k, info['dropped2']), flush=True)
    np.savez(out_path, **out)
    print('%d arrays -> %s' % (len(out), out_path))


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    bad = sorted(set(a.files) ^ set(b.files))
    for key in sorted(set(a.files) & set(b.files)):
        same = np.array_equal(a[key], b[key])
        print('%-70s %-14s %s' % (key, a[key].shape, 'equal' if same else 'DIFFERENT'))
        if not same:
            bad.append(key)
    print('%d arrays compared, %d different or missing: %s' % (len(a.files), len(bad), bad))
    return 1 if bad else 0


def launches(path):
    """The launches of a kernel trace in order of their start.  The HIP runtime's own copy kernels (__amd_rocclr_*) are left out: whether a
    read-back goes through one of them or through a DMA engine is the runtime's choice and differs between two runs of the same build."""
    rows = [r for r in csv.DictReader(open(path)) if not r['Kernel_Name'].startswith('__amd_rocclr')]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    cols = ('Kernel_Name', 'Grid_Size_X', 'Grid_Size_Y', 'Grid_Size_Z', 'Workgroup_Size_X', 'Workgroup_Size_Y', 'Workgroup_Size_Z', 'LDS_Block_Size')
    return [' '.join(r.get(c, '?') for c in cols) for r in rows]


def compare_launches(a_path, b_path):
    a, b = launches(a_path), launches(b_path)
    diff = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
    print('%d and %d launches, %d lines differ' % (len(a), len(b), len(diff) + abs(len(a) - len(b))))
    for i in diff[:10]:
        print('  line %d:\n    %s\n    %s' % (i, a[i], b[i]))
    names = {}
    for line in a:
        nm = line.replace('(anonymous namespace)', '{anonymous}').split('(')[0].replace('void ', '')
        names[nm] = names.get(nm, 0) + 1
    for nm in sorted(names):
        print('  %6d  %s' % (names[nm], nm))
    return 1 if diff or len(a) != len(b) else 0


if __name__ == '__main__':
    if len(sys.argv) == 3 and sys.argv[1] == 'run':
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] in ('compare', 'launches'):
        sys.exit((compare if sys.argv[1] == 'compare' else compare_launches)(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
