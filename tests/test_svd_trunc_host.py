"""CPU checks of what the GPU tests of tn_svd_trunc stand on (tests/svd_trunc_ref.py): the golden file holds exactly the referenced
inputs, small entries are recomputed at 40 digits, the margin condition holds, trunc_rule agrees with a plain numpy evaluation on
LAPACK's values wherever those decide -- and the argument errors tn_svd_trunc / tn_svd_trunc_batched raise before any device work
(a host address stands in for device memory and is never dereferenced)."""
import ctypes
import math

import numpy as np
import pytest

import svd_trunc_ref as tr

CASES = tr.cases()
LAPACK_ERR = 1e-13                                               # |LAPACK value - true value| <= 1e-13 s_0, the bound the suite holds LAPACK to


def _lib():
    from tnac4o_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _msg(L):
    buf = ctypes.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    return buf.value.decode()


def _expect_neg(L, rc, text):
    assert rc < 0, rc
    assert text in _msg(L), _msg(L)


# ------------------------------------------------------------------------------------------------------------------ the golden file
def test_golden_file_holds_exactly_the_referenced_inputs():
    inputs = tr.all_reference_inputs()
    keys = {tr._key(A) for A in inputs.values()}
    with np.load(tr.GOLDEN) as z:
        assert set(z.files) == keys
        for name, A in inputs.items():
            v = z[tr._key(A)]
            assert v.dtype == np.float64 and v.shape == (min(A.shape),), name
            assert np.all(np.diff(v) <= 0) and np.all(v >= 0), name
    for name, A in inputs.items():
        assert tr.stored(A) is not None, name
        assert max(min(A.shape), 0) <= 70, name                  # a full rewrite stays at a few minutes
    again = tr.cases()
    assert list(again) == list(CASES)
    for name in CASES:
        assert tr._key(again[name]) == tr._key(CASES[name]), name


@pytest.mark.parametrize('name', ['gauss_1x1', 'gauss_1x9', 'gauss_9x1', 'gauss_3x5', 'gauss_17x17', 'tiny_row', 'zero'])
def test_small_entries_recomputed(name):
    pytest.importorskip('mpmath')
    A = CASES[name]
    assert max(A.shape) <= 17
    assert np.array_equal(tr.mp_svdvals(A), tr.stored(A))


def test_margin_condition_and_relaxed_list():
    assert tr.margin_violations() == []
    assert len(tr.RELAXED) <= 2 and set(tr.RELAXED) <= set(CASES)
    # every case has the two settings the suite always runs, one that cuts the spectrum, and the special ones are present
    for name, A in CASES.items():
        st = tr.settings(name, A)
        assert (min(A.shape), 0.0) in st and (10 ** 6, 1e-16) in st, name
        assert min(A.shape) < 2 or any(D < min(A.shape) for D, _ in st), name
    for name in tr.CLUSTERED:
        sigma = tr.ref_svdvals(CASES[name])
        for D in (8, 24):                                       # inside a cluster: the neighbours on both sides of the cut agree to 1e-9
            assert (D, 0.0) in tr.settings(name) and abs(sigma[D - 1] - sigma[D]) <= 1e-9 * sigma[0]
    assert sum((10 ** 6, 1.0) in tr.settings(n) for n in CASES if not tr.is_block(n)) >= 1
    assert sum((10 ** 6, 1.0) in tr.settings(n) for n in CASES if tr.is_block(n)) >= 1
    # a relaxed case is pinned wherever Dmax or tol decides, and only there
    for name in tr.RELAXED:
        sigma = tr.ref_svdvals(CASES[name])
        flags = [tr.pinned(name, sigma, D, t) for D, t in tr.settings(name)]
        assert any(flags) and not all(flags), name
        for D, t in tr.settings(name):
            lo, hi = tr.keep_bounds(name, sigma, D, t)
            assert 0 <= lo <= hi <= min(D, sigma.size)


# ------------------------------------------------------------------------------------------------------------------ the rule
def test_trunc_rule_on_written_out_values():
    s = [4.0, 2.0, 1.0, 0.5, 1e-20]
    assert tr.trunc_rule(s, 10, 0.0) == (4, 1e-20 / 4.0)
    assert tr.trunc_rule(s, 2, 0.0) == (2, math.sqrt(1e-40 + 0.25 + 1.0) / 4.0)
    assert tr.trunc_rule(s, 10, 0.25) == (2, math.sqrt(1e-40 + 0.25 + 1.0) / 4.0)        # 1.0 > 4 * 0.25 is false: strict
    assert tr.trunc_rule(s, 10, 1.0) == (0, math.sqrt(1e-40 + 0.25 + 1.0 + 4.0 + 16.0) / 4.0)
    assert tr.trunc_rule(s, 10, 7.0)[0] == 0
    assert tr.trunc_rule([0.0, 0.0, 0.0], 3, 0.0) == (0, 0.0)
    assert tr.trunc_rule([3.0], 10 ** 6, 1e-16) == (1, 0.0)
    # from the smallest value up: the small ones are not lost against the large one
    t = [1.0] + [2.0 ** -27] * 4
    assert tr.trunc_rule(t, 0, 0.0)[1] == math.sqrt(1.0 + 2.0 ** -52)
    assert tr.trunc_rule(t, 0, 0.0, fsum=True)[1] == math.sqrt(1.0 + 2.0 ** -52)


@pytest.mark.parametrize('name', list(CASES))
def test_trunc_rule_against_numpy_on_lapack_values(name):
    """Wherever LAPACK's values decide the kept rank (none of them within its error of the threshold, or Dmax decides), the rule
    on the 40-digit values gives the same rank and, to LAPACK's error, the same discarded weight; the fsum variant agrees with
    the plain sum to rounding."""
    A = CASES[name]
    sigma = tr.ref_svdvals(A)
    lap = np.linalg.svd(np.ascontiguousarray(A), compute_uv=False)
    assert np.abs(lap - sigma).max() <= LAPACK_ERR * max(sigma[0], 1e-300)
    decided = 0
    for Dmax, tol in tr.settings(name, A):
        keep, disc = tr.trunc_rule(sigma, Dmax, tol)
        keep_f, disc_f = tr.trunc_rule(sigma, Dmax, tol, fsum=True)
        # n squares added one by one: (n - 1) eps / 2 on the sum, half of that on its root, plus the root and the quotient
        assert keep_f == keep and abs(disc_f - disc) <= (sigma.size / 4 + 2) * tr.EPS * disc
        if name in tr.ZERO:
            assert (keep, disc) == (0, 0.0)
            decided += 1
            continue
        if tol >= 1.0:
            assert keep == 0 and disc == pytest.approx(np.linalg.norm(sigma) / sigma[0], rel=1e-14)
        t = max(tr.EPS, tol)
        thr = lap[0] * t
        lo = min(int(np.sum(lap > thr + LAPACK_ERR * lap[0])), Dmax)
        hi = min(int(np.sum(lap > thr - LAPACK_ERR * lap[0])), Dmax)
        if tol >= 1.0:
            lo = hi = 0
        if lo != hi:
            continue
        decided += 1
        assert keep == lo, (name, Dmax, tol)
        want = np.sqrt(np.sum(lap[keep:][::-1] ** 2)) / lap[0]
        # each value off by <= 1e-13 s_0: the norm of min(k, n) of them by <= sqrt(min(k, n)) 1e-13, and s_0 itself by 1e-13 relative
        assert abs(disc - want) <= math.sqrt(lap.size) * LAPACK_ERR + 2 * LAPACK_ERR * want, (name, Dmax, tol)
    assert decided >= 1, name


# ------------------------------------------------------------------------------------------------------------------ argument errors
def _host_ptr(n=64):
    host = (ctypes.c_double * n)()
    return host, ctypes.cast(host, ctypes.c_void_p)


def test_svd_trunc_argument_errors():
    L = _lib()
    _h, P = _host_ptr()
    keep = ctypes.c_int64(-5)
    need = int(L.tn_svd_ws_bytes(70, 66, 1))

    def call(C=P, k=70, n=66, Dmax=8, U=P, S=P, Vt=P, kout=True, ws=P, wsb=need):
        return L.tn_svd_trunc(C, n, 1, k, n, Dmax, 0.0, U, Dmax, 1, S, Vt, n, 1, ctypes.byref(keep) if kout else None, None, None, None,
                              ws, wsb, None)
    for kw in ('C', 'U', 'S', 'Vt', 'ws'):
        _expect_neg(L, call(**{kw: None}), 'null operand')
    _expect_neg(L, call(kout=False), 'null operand')
    for kw in ('k', 'n', 'Dmax'):
        for bad in (0, -3):
            _expect_neg(L, call(wsb=1 << 40, **{kw: bad}), 'bad dimensions')
    _expect_neg(L, call(wsb=need - 1), 'workspace too small')
    small = int(L.tn_svd_ws_bytes(17, 17, 1))                    # the one-launch path asks for the same workspace
    _expect_neg(L, call(k=17, n=17, wsb=small - 1), 'workspace too small')
    assert keep.value == -5


def test_svd_trunc_batched_argument_errors():
    L = _lib()
    _h, P = _host_ptr()
    keep = (ctypes.c_int64 * 3)(-5, -5, -5)
    need = -(-int(L.tn_svd_ws_bytes(65, 66, 1)) // 256) * 256

    def call(C=P, k=65, n=66, Dmax=8, U=P, S=P, Vt=P, kout=True, batch=3, ws=P, wsb=need):
        return L.tn_svd_trunc_batched(C, n, 1, k, n, Dmax, 0.0, U, Dmax, 1, S, Vt, n, 1, keep if kout else None, None, None, None, batch,
                                      k * n + 7, k * Dmax + 5, Dmax + 3, Dmax * n + 9, ws, wsb, None)
    _expect_neg(L, call(batch=-1), 'negative batch')
    for kw in ('C', 'U', 'S', 'Vt', 'ws'):
        _expect_neg(L, call(**{kw: None}), 'null operand')
    _expect_neg(L, call(kout=False), 'null operand')
    for kw in ('k', 'n', 'Dmax'):
        for bad in (0, -3):
            _expect_neg(L, call(wsb=1 << 40, **{kw: bad}), 'bad dimensions')
    _expect_neg(L, call(wsb=need - 1), 'workspace too small')
    assert L.tn_svd_trunc_batched(None, 1, 1, 4, 4, 4, 0.0, None, 4, 1, None, None, 4, 1, None, None, None, None, 0, 16, 16, 4, 16, None, 0,
                                  None) == 0                     # batch = 0: a no-op, nothing dereferenced
    assert list(keep) == [-5, -5, -5]
