"""Reference, inputs and settings for the direct tests of the truncating SVD tn_svd_trunc (csrc/svd.hip) on its three paths:
svd_trunc_small_kernel (both sides <= 64), the block path with all rounds in one launch (svdl_kernel) and with separate launches.

- ref_svdvals(A): singular values at 40 digits (svdvals_ref.mp_svdvals), rounded to float64, kept in tests/golden/svd_trunc_ref.npz
  under a hash of shape and bytes: a hit returns the stored values, a miss is computed once per process.  `python
  tests/svd_trunc_ref.py` rewrites the file (a few minutes); tests/test_svd_trunc_host.py checks that it is complete.
- trunc_rule(sigma, Dmax, tol): the documented rule in Python floats, keep = min(#(s_i > s_0 max(eps, tol)), Dmax) and
  discarded = sqrt(sum_{i >= keep} s_i^2) / s_0 added from the smallest value up (0.0 when s_0 == 0).
- cases(): name -> matrix, the smallest shapes that reach each piece of code; settings(name): the (Dmax, tol) pairs of a case.
- margin_violations(): the (case, Dmax, tol) whose kept rank is pinned although a reference value lies within a relative 1e-9 of
  the threshold s_0 max(eps, tol).  It must return nothing.
- RELAXED: the cases whose spectrum truly crosses eps s_0 (the noise values of a rank-deficient product, 0.1-1 eps s_0, which no
  double precision SVD determines): their kept rank is pinned only where Dmax or tol decides (pinned()), and is otherwise held
  between the number of values above 1e-13 s_0 and the number of values above 0.  At most two cases, a condition of the suite.
  (That cap is why 'rank7', 'dup_rows', 'col_graded' and 'row_graded' of svdvals_ref.cases() are not reused here: their spectra
  cross eps s_0 as well -- row_graded has values at 1.3 and 0.7 eps s_0 -- and the values-only tests keep them.  'graded' here is
  row-graded over twelve decades, its smallest value 50 eps s_0.)
"""
import math
import os

import numpy as np

import svdvals_ref as sv
from svdvals_ref import _key, mp_svdvals, root_and_view  # noqa: F401  (root_and_view: re-exported for the GPU tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'svd_trunc_ref.npz')
EPS = 2.220446049250313e-16
MARGIN = 1e-9
SMALL_GAUSS = ((1, 1), (1, 9), (9, 1), (3, 5), (17, 17), (33, 64), (64, 33), (64, 64))
REUSED = ('usv', 'clusters', 'tiny_row', 'view', 'zero')
BLOCK_GAUSS = ((1, 65), (65, 1), (3, 65), (65, 3), (65, 65), (65, 70), (70, 66), (66, 70))
RELAXED = ('rank7_65', 'usv_65')
GRADED = ('graded', 'usv', 'usv_65')
CLUSTERED = ('clusters', 'clusters_65')
TOL_ONE = ('gauss_17x17', 'gauss_65x70')
TOL_MID = ('gauss_33x64', 'gauss_70x66')
TINY_ROW = {'tiny_row': 9, 'tiny_row_65': 9}                   # case -> the input row that is deflated up front
ZERO = ('zero', 'zero_65')
RANGE_BLOCK_SHAPE = (65, 66)
NONFINITE_SHAPES = ((5, 7), (64, 64), (65, 66))
BATCH_SHAPES = ((17, 17), (65, 66))
STRIDE_CASES = ('gauss_33x64', 'gauss_64x33', 'gauss_65x70', 'gauss_70x66')

_store = None
_memo = {}


def stored(A):
    """The values kept for A in tests/golden/svd_trunc_ref.npz, or None."""
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


# ------------------------------------------------------------------------------------------------------------------ the rule
def discarded_at(sigma, keep, fsum=False):
    """sqrt(sum_{i >= keep} s_i^2) / s_0, added from the smallest value up (fsum: correctly rounded sum); 0.0 when s_0 == 0."""
    s = [float(v) for v in sigma]
    if s[0] == 0.0:
        return 0.0
    if fsum:
        d2 = math.fsum(v * v for v in s[keep:])
    else:
        d2 = 0.0
        for v in reversed(s[keep:]):
            d2 += v * v
    return math.sqrt(d2) / s[0]


def trunc_rule(sigma, Dmax, tol, fsum=False):
    """(keep, discarded) of the documented rule on the descending values `sigma`."""
    s = [float(v) for v in sigma]
    thr = s[0] * max(EPS, float(tol))
    keep = min(sum(1 for v in s if v > thr), int(Dmax))
    return keep, discarded_at(s, keep, fsum)


# ------------------------------------------------------------------------------------------------------------------ inputs
def cases():
    """name -> matrix.  Every call returns the same bits."""
    c = sv.cases()
    out = {}
    for sh in SMALL_GAUSS:
        out['gauss_%dx%d' % sh] = sv.gauss(sh)
    for name in REUSED:
        out[name] = c[name]
    out['graded'] = np.logspace(0, -12, 64)[:, None] * sv._rng(37).standard_normal((64, 64))   # rows graded, every value >> eps s_0
    for sh in BLOCK_GAUSS:
        out['gauss_%dx%d' % sh] = sv.gauss(sh)
    r = sv._rng(30)
    s = np.concatenate([np.logspace(0, -14, 48), np.zeros(17)])
    out['usv_65'] = (sv._orth(r, 65) * s[None, :]) @ sv._orth(r, 70, 65).T
    r = sv._rng(31)
    out['rank7_65'] = r.standard_normal((66, 7)) @ r.standard_normal((7, 70))
    r = sv._rng(32)
    s = np.concatenate([np.ones(16), np.full(16, 1.0 - 1e-10), np.logspace(-1, -6, 34)])
    out['clusters_65'] = (sv._orth(r, 66) * s[None, :]) @ sv._orth(r, 66).T
    t = sv._rng(33).standard_normal((66, 70))
    t[TINY_ROW['tiny_row_65']] *= 2.0 ** -60                    # deflated up front
    out['tiny_row_65'] = t
    out['view_65'] = sv._rng(34).standard_normal((80, 150))[5:71, 7:143:2]
    out['zero_65'] = np.zeros((66, 70))
    return out


def is_block(name, A=None):
    A = cases()[name] if A is None else A
    return max(A.shape) >= 65


def paths(A):
    """The paths a matrix can take: a side >= 65 leaves only the block path."""
    return ('block', 'block_separate') if max(A.shape) >= 65 else ('small', 'block', 'block_separate')


def settings(name, A=None):
    """The (Dmax, tol) pairs of a case."""
    A = cases()[name] if A is None else A
    m = min(A.shape)
    out = [(m, 0.0), (10 ** 6, 1e-16)]                          # the second: far above the size (the buffers hold min(k, n))
    if m >= 2:
        out.append((m // 2, 0.0))                               # cuts the spectrum in the middle
    if name in CLUSTERED:
        out += [(8, 0.0), (24, 0.0)]                            # inside the first and inside the second 16-fold cluster
    if name in GRADED:
        out.append((10 ** 6, 1e-6))
    if name == 'rank7_65':
        out += [(5, 0.0), (10 ** 6, 1e-6)]                      # Dmax below the rank, tol far above the noise: the kept rank is pinned
    if name in TOL_ONE:
        out.append((10 ** 6, 1.0))                              # nothing exceeds s_0 itself: keep = 0
    if name in TOL_MID:
        out.append((10 ** 6, 0.3))                              # tol > eps decides, in the middle of the spectrum
    return out


def range_base(path):
    return sv.range_base() if path == 'small' else sv.gauss(RANGE_BLOCK_SHAPE)


def nonfinite_base(shape):
    return sv._rng(35, *shape).standard_normal(shape)


def batch_items(shape, batch=3):
    return [sv._rng(36, i, *shape).standard_normal(shape) for i in range(batch)]


def all_reference_inputs():
    """Every matrix whose reference values the tests look up (what tests/golden/svd_trunc_ref.npz holds)."""
    out = dict(cases())
    out['range_small'] = range_base('small')
    out['range_block'] = range_base('block')
    return out


# ------------------------------------------------------------------------------------------------------------------ what is pinned
def count_above(sigma, rel):
    return int(np.sum(np.asarray(sigma) > rel * sigma[0])) if sigma[0] > 0 else 0


def pinned(name, sigma, Dmax, tol):
    """Whether the tests hold the kept rank of (name, Dmax, tol) to trunc_rule exactly.  A RELAXED case: only where Dmax decides (it
    is at most the number of values above 1e-13 s_0) or tol does (tol >= 1e-9, far above the noise)."""
    if name not in RELAXED:
        return True
    return Dmax <= count_above(sigma, 1e-13) or tol >= 1e-9


def keep_bounds(name, sigma, Dmax, tol):
    """(lowest, highest) kept rank the tests accept."""
    keep = trunc_rule(sigma, Dmax, tol)[0]
    if pinned(name, sigma, Dmax, tol):
        return keep, keep
    return min(count_above(sigma, 1e-13), Dmax), min(int(np.sum(np.asarray(sigma) > 0.0)), Dmax)


def margin_violations():
    """The (case, Dmax, tol) with a pinned kept rank and a reference value within a relative MARGIN of s_0 max(eps, tol)."""
    bad = []
    for name, A in cases().items():
        sigma = ref_svdvals(A)
        if sigma[0] == 0.0:
            continue
        for Dmax, tol in settings(name, A):
            if tol >= 1.0:                                      # no value of a descending list exceeds s_0 tol, whatever its error: keep = 0
                continue
            thr = sigma[0] * max(EPS, tol)
            if pinned(name, sigma, Dmax, tol) and np.any(np.abs(sigma - thr) <= MARGIN * thr):
                bad.append((name, Dmax, tol))
    return bad


def write_golden():
    vals = {}
    for name, A in all_reference_inputs().items():
        vals[_key(A)] = mp_svdvals(A)
        print(name, A.shape, flush=True)
    np.savez_compressed(GOLDEN, **vals)


if __name__ == '__main__':
    write_golden()
    print('margin violations:', margin_violations())
