"""Reference and inputs for the direct tests of the values-only SVD of small centre matrices (svd_vals_small_body in csrc/svd.hip,
behind tn_svdvals for sides <= 64, tn_svdvals_async and tn_svdvals_small_batched).

- ref_svdvals(A): the singular values from mpmath.svd_r at 40 digits, sorted descending, rounded to float64.  A 64 x 64 matrix costs
  seconds, so the values of the inputs below are kept in tests/golden/svdvals_ref.npz, keyed by a hash of the input's shape and
  bytes: a hit returns the stored values, anything else is computed (and kept for the process).  `python tests/svdvals_ref.py`
  rewrites the file; tests/test_svdvals_host.py recomputes its entries.
- cases(): the seeded inputs, name -> matrix (both dimensions <= 64; 'view' is a strided view of a larger array).
- exact_cases(): name -> (matrix, values) for inputs whose rows are exactly orthogonal with exactly representable squared norms:
  the values are the sorted row norms bit for bit and one sweep without a rotation suffices.
- boundary_cases(): 64 x n inputs and their 65-row extensions (the first size of the block path).
- root_and_view(A): the owning array of a view with its element offset and strides, to rebuild the same view on the device.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'svdvals_ref.npz')
DPS = 40
GAUSS_SHAPES = ((1, 1), (1, 64), (64, 1), (2, 2), (3, 5), (7, 8), (8, 9), (9, 8), (17, 17), (31, 33), (33, 64), (63, 63), (63, 64),
                (64, 63), (64, 64))
RANGE_SHAPE = (24, 40)
RANGE_EXPONENTS = (-500, -300, -260, -100, 100, 250, 300, 480)
NONFINITE_SHAPES = ((5, 7), (64, 64))

_store = None
_memo = {}


def _rng(*key):
    return np.random.default_rng([20240, *key])


def _key(A):
    A = np.ascontiguousarray(A, dtype=np.float64)
    return 'k' + hashlib.sha256(repr(A.shape).encode() + A.tobytes()).hexdigest()[:24]


def mp_svdvals(A):
    """Singular values of A by mpmath.svd_r at DPS digits: descending, rounded to float64 (always computed)."""
    import mpmath
    A = np.asarray(A, dtype=np.float64)
    with mpmath.workdps(DPS):
        S = mpmath.svd_r(mpmath.matrix(A.tolist()), compute_uv=False)
        vals = sorted((abs(S[i]) for i in range(len(S))), reverse=True)
        return np.array([float(v) for v in vals], dtype=np.float64)


def stored(A):
    """The values kept for A in tests/golden/svdvals_ref.npz, or None."""
    global _store
    if _store is None:
        _store = {}
        if os.path.exists(GOLDEN):
            with np.load(GOLDEN) as z:
                _store = {k: z[k] for k in z.files}
    v = _store.get(_key(A))
    return None if v is None else v.copy()


def ref_svdvals(A):
    """Singular values of A (min(k, n) of them, descending, float64) at 40 digits: stored, else computed once per process."""
    k = _key(A)
    if k not in _memo:
        v = stored(A)
        _memo[k] = mp_svdvals(A) if v is None else v
    return _memo[k].copy()


# ------------------------------------------------------------------------------------------------------------------ inputs
def _orth(rng, m, n=None):
    """m x n with orthonormal columns (n <= m)."""
    return np.linalg.qr(rng.standard_normal((m, n or m)))[0]


def gauss(shape):
    return _rng(1, *shape).standard_normal(shape)


def cases():
    """name -> matrix.  Every call returns the same bits."""
    out = {}
    for sh in GAUSS_SHAPES:
        out['gauss_%dx%d' % sh] = gauss(sh)
    r = _rng(2)
    out['col_graded'] = (r.standard_normal((60, 60)) * np.logspace(0, -18, 60)[None, :]) @ _orth(r, 60)
    r = _rng(3)
    out['row_graded'] = np.logspace(0, -15, 64)[:, None] * r.standard_normal((64, 64))
    r = _rng(4)
    out['usv'] = (_orth(r, 64, 48) * np.logspace(0, -14, 48)[None, :]) @ _orth(r, 48).T
    r = _rng(5)
    out['rank7'] = r.standard_normal((40, 7)) @ r.standard_normal((7, 33))
    r = _rng(6)
    d = r.standard_normal((20, 30))
    d[5] = d[2]
    d[17] = d[2]
    d[11] = d[9]
    out['dup_rows'] = d
    out['orth3'] = 3.0 * _orth(_rng(7), 64)
    r = _rng(8)
    s = np.concatenate([np.ones(16), np.full(16, 1.0 - 1e-10)])
    out['clusters'] = (_orth(r, 32) * s[None, :]) @ _orth(r, 32).T
    t = _rng(9).standard_normal((10, 12))
    t[9] *= 2.0 ** -60                                       # deflated by the kernel: reported as 0
    out['tiny_row'] = t
    out['view'] = _rng(10).standard_normal((50, 90))[:40, 10:70:2]
    out['zero'] = np.zeros((4, 9))
    return out


def exact_cases():
    """name -> (matrix, values): rows exactly orthogonal, squared norms exact, all norms within 2^40 of each other (nothing is
    deflated), so the values are the row norms sorted descending (zero padded to min(k, n))."""
    out = {}
    d = np.array([3.0, -5.0 * 2.0 ** -7, 7.0 * 2.0 ** 9, 1.5, 0.0, -2.0 ** -12, 2.0 ** 14, 11.0 * 2.0 ** -3, 2.0 ** 14])
    D = np.zeros((9, 13))
    D[np.arange(9), np.arange(9)] = d
    out['diagonal'] = (D, np.sort(np.abs(d))[::-1].copy())
    r = _rng(11)
    n = 33
    e = r.integers(-20, 21, n)
    P = np.zeros((n, n))
    P[np.arange(n), r.permutation(n)] = np.where(r.random(n) < 0.5, -1.0, 1.0) * 2.0 ** e
    out['signed_perm'] = (P, np.sort(2.0 ** e)[::-1].copy())
    from scipy.linalg import hadamard
    e = _rng(12).integers(-20, 21, 64)
    H = hadamard(64).astype(np.float64) * (2.0 ** e)[:, None]
    out['hadamard'] = (H, np.sort(8.0 * 2.0 ** e)[::-1].copy())
    return out


def boundary_cases():
    """name -> matrix: two 64-row inputs (single launch) and the same with one more Gaussian row (65 rows: the block path)."""
    c = cases()
    out = {}
    for i, name in enumerate(('gauss_64x64', 'usv')):
        A = c[name]
        out[name + '_64'] = A
        out[name + '_65'] = np.vstack([A, _rng(13, i).standard_normal((1, A.shape[1]))])
    return out


def range_base():
    return gauss(RANGE_SHAPE)


def nonfinite_base(shape):
    return _rng(14, *shape).standard_normal(shape)


def all_reference_inputs():
    """Every matrix whose reference values the tests look up (what tests/golden/svdvals_ref.npz holds)."""
    out = dict(cases())
    out.update({k: v[0] for k, v in exact_cases().items()})
    out.update(boundary_cases())
    out['range_base'] = range_base()
    return out


def root_and_view(A):
    """(root, offset, strides): the array that owns A's memory, and A's offset and strides in it in elements."""
    root = A
    while root.base is not None:
        root = root.base
    off = (A.__array_interface__['data'][0] - root.__array_interface__['data'][0]) // A.itemsize
    return root, off, tuple(s // A.itemsize for s in A.strides)


def write_golden():
    vals = {}
    for name, A in all_reference_inputs().items():
        vals[_key(A)] = mp_svdvals(A)
        print(name, A.shape, flush=True)
    np.savez_compressed(GOLDEN, **vals)


if __name__ == '__main__':
    write_golden()
