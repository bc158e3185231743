"""CPU checks of the helper kernels' surface: the host references of tests/helpers_ref.py on hand-built cases with the expected
values written out, and the argument errors of the helper entry points (checked before any launch, so a host address stands
in for device memory and is never dereferenced)."""
import ctypes
from fractions import Fraction

import numpy as np

import helpers_ref as hr


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


# ------------------------------------------------------------------------------------------------------------ the references
def test_argsort_ref_order():
    nan, inf = float('nan'), float('inf')
    w = [1.0, nan, 3.0, -0.0, 3.0, 0.0, -inf, inf, nan, -2.0, 0.0]
    # NaN first (by index), then +inf, the two 3.0 by index, 1.0, the three zeros by index (+0.0 == -0.0), -2.0, -inf
    assert hr.argsort_desc_ref(w).tolist() == [1, 8, 7, 2, 4, 0, 3, 5, 10, 9, 6]
    assert hr.argsort_desc_ref([5.0] * 6).tolist() == [0, 1, 2, 3, 4, 5]
    assert hr.argsort_desc_ref([1.0, 2.0, nan]).tolist() == [2, 1, 0]
    assert hr.argsort_desc_ref([7.0]).tolist() == [0]


def test_exact_sums_and_bounds():
    big = Fraction(*1e100.as_integer_ratio())
    assert hr.exact_dot([1e100, 1.0, -1e100], [1.0, 1.0, 1.0]) == (Fraction(1), 2 * big + 1)
    assert hr.exact_dot([0.5, 0.25], [0.5, -4.0]) == (Fraction(-3, 4), Fraction(5, 4))
    assert hr.exact_sum([0.1, 0.2]) == Fraction(*0.1.as_integer_ratio()) + Fraction(*0.2.as_integer_ratio())
    assert hr.gamma(1) == Fraction(1, 2 ** 53 - 1)
    # depths of the documented orders
    assert hr.weighted_sum_bound(256, Fraction(1)) == hr.gamma(1 + 8 + 1)
    assert hr.weighted_sum_bound(257, Fraction(1)) == hr.gamma(2 + 8 + 1)
    assert hr.rows_norm2_depth(1) == 11 and hr.rows_norm2_depth(256) == 11 and hr.rows_norm2_depth(257) == 12
    assert hr.within(1.0 + 2.0 ** -52, Fraction(1), Fraction(1, 2 ** 52))
    assert not hr.within(1.0 + 2.0 ** -51, Fraction(1), Fraction(1, 2 ** 52))


def test_gram_ref_floor_and_kfro():
    G = np.array([[4.0, 1.0, 0.0], [1.0, 1e-30, 0.0], [0.0, 0.0, 2.0]])
    d2, gmax = hr.gram_weights_ref(G, 0.25)
    assert gmax == 4.0
    assert d2.tolist() == [4.0, 1.0, 2.0]                  # G_11 below the floor 0.25 * 4 -> 1.0
    # 16/16 + 2 * 1/(4*1) + 1e-60/1 + 4/4
    assert abs(hr.gram_kfro_ref(G, d2) - 2.5) <= 2.5 * 2.0 ** -52
    d2z, gz = hr.gram_weights_ref(np.zeros((3, 3)), 1e-12)
    assert gz == 0.0 and d2z.tolist() == [0.0, 0.0, 0.0]


def test_gather_ref_round_trip():
    A = np.arange(12.0).reshape(4, 3)
    perm = np.array([2, 0, 3, 1])
    w2 = np.array([4.0, 9.0, 16.0, 1.0])
    F = hr.gather_scale_rows_ref(A, perm, w2)
    assert F.tolist() == [[24.0, 28.0, 32.0], [0.0, 2.0, 4.0], [9.0, 10.0, 11.0], [9.0, 12.0, 15.0]]
    B = hr.gather_scale_rows_ref(F, perm, w2, inverse=True)
    assert np.array_equal(B, A)


def test_bond_deflate_ref_rule():
    nmax = 2.0 ** 10
    budget = hr.EPS ** 2 * nmax                            # 2^-94
    # exactly on the budget: dropped (<=); indices 1 and 3 tie, the lower index goes first
    assert hr.bond_deflate_ref([nmax, budget / 2, 4.0, budget / 2, 1.0]) == (0, [0, 2, 4], budget / nmax)
    # the second of the pair two ulps larger (one ulp would be lost in the rounded sum): it no longer fits and is kept
    assert hr.bond_deflate_ref([nmax, budget / 2, 4.0, budget / 2 * (1 + 2.0 ** -51), 1.0]) == (0, [0, 2, 3, 4], budget / 2 / nmax)
    # equal norms: ties broken by index (four of the five fit)
    assert hr.bond_deflate_ref([nmax] + [budget / 4] * 5 + [nmax]) == (0, [0, 5, 6], budget / nmax)
    # every index negligible but one: at most k - 1 dropped
    assert hr.bond_deflate_ref([0.0, 0.0, 5.0, 0.0]) == (0, [2], 0.0)
    # all zero, k == 1: nothing dropped
    assert hr.bond_deflate_ref([0.0, 0.0, 0.0]) == (0, [0, 1, 2], 0.0)
    assert hr.bond_deflate_ref([0.0]) == (0, [0], 0.0)
    assert hr.bond_deflate_ref([3.0]) == (0, [0], 0.0)
    # non-finite
    assert hr.bond_deflate_ref([1.0, float('nan')])[0] == -2
    assert hr.bond_deflate_ref([float('inf'), 1.0])[0] == -2
    # exact squared norms of both sides
    C = np.array([[3.0, 4.0], [0.0, 2.0 ** -60], [1.0, 0.0]])
    assert hr.bond_norms2(0, C).tolist() == [25.0, 2.0 ** -120, 1.0]
    assert hr.bond_norms2(1, C).tolist() == [10.0, 16.0 + 2.0 ** -120]
    Q = np.arange(6.0).reshape(2, 3)
    Co, Qo = hr.bond_deflate_apply(0, C, Q, [0, 2])
    assert Co.tolist() == [[3.0, 4.0], [1.0, 0.0]] and Qo.tolist() == [[0.0, 2.0], [3.0, 5.0]]


def test_scale_phys_ref_and_ulps():
    A = np.ones((2, 3, 2))
    d = np.array([2.0, 4.0, 8.0, 99.0])
    assert hr.scale_phys_ref(A, d)[1, :, 0].tolist() == [2.0, 4.0, 8.0]
    assert hr.scale_phys_ref(A, d, inv=True)[0, :, 1].tolist() == [0.5, 0.25, 0.125]
    assert hr.ulps(np.array([1.0, -1.0, 0.0]), np.array([np.nextafter(1.0, 2.0), -1.0, -0.0])).tolist() == [1, 0, 0]


# ------------------------------------------------------------------------------------------------------------ argument errors
def _host_ptr(n=64):
    host = (ctypes.c_double * n)()
    return host, ctypes.cast(host, ctypes.c_void_p)


def test_argsort_and_weighted_sum_argument_errors():
    L = _lib()
    _h, P = _host_ptr()
    _expect_neg(L, L.tn_argsort_desc(None, 4, P, None), 'null operand')
    _expect_neg(L, L.tn_argsort_desc(P, 4, None, None), 'null operand')
    _expect_neg(L, L.tn_argsort_desc(P, 0, P, None), 'length out of range')
    _expect_neg(L, L.tn_argsort_desc(P, -3, P, None), 'length out of range')
    _expect_neg(L, L.tn_argsort_desc(P, (1 << 20) + 1, P, None), 'length out of range')
    _expect_neg(L, L.tn_weighted_sum(None, P, 4, P, P, None), 'null operand')
    _expect_neg(L, L.tn_weighted_sum(P, P, 4, P, None, None), 'null operand')
    _expect_neg(L, L.tn_weighted_sum(P, P, 0, P, P, None), 'empty input')


def test_gram_rows_gather_argument_errors():
    L = _lib()
    _h, P = _host_ptr()
    _expect_neg(L, L.tn_gram_weights(None, 4, 0.0, P, P, None), 'null operand')
    _expect_neg(L, L.tn_gram_weights(P, 4, 0.0, None, P, None), 'null operand')
    _expect_neg(L, L.tn_gram_weights(P, 4, 0.0, P, None, None), 'null operand')
    _expect_neg(L, L.tn_gram_weights(P, 0, 0.0, P, P, None), 'bad arguments')
    _expect_neg(L, L.tn_gram_weights(P, 65537, 0.0, P, P, None), 'bad arguments')
    _expect_neg(L, L.tn_gram_weights(P, 4, -1e-12, P, P, None), 'bad arguments')
    assert L.tn_rows_norm2(None, 0, 5, None, None) == 0                      # rows = 0: a no-op, nothing dereferenced
    _expect_neg(L, L.tn_rows_norm2(None, 3, 5, P, None), 'null operand')
    _expect_neg(L, L.tn_rows_norm2(P, 3, 5, None, None), 'null operand')
    _expect_neg(L, L.tn_rows_norm2(P, 3, 0, P, None), 'bad dimensions')
    assert L.tn_gather_scale_rows(None, 0, 5, None, None, None, 0, None) == 0
    for inv in (0, 1):
        _expect_neg(L, L.tn_gather_scale_rows(None, 3, 5, P, P, P, inv, None), 'null operand')
        _expect_neg(L, L.tn_gather_scale_rows(P, 3, 5, None, P, P, inv, None), 'null operand')
        _expect_neg(L, L.tn_gather_scale_rows(P, 3, 5, P, None, P, inv, None), 'null operand')
        _expect_neg(L, L.tn_gather_scale_rows(P, 3, 5, P, P, None, inv, None), 'null operand')
    _expect_neg(L, L.tn_scale_phys(None, 2, 2, 2, P, 0, None), 'null operand')
    _expect_neg(L, L.tn_scale_phys(P, 2, 2, 2, None, 1, None), 'null operand')
    assert L.tn_scale_phys(P, 0, 2, 2, P, 0, None) == 0                     # empty tensor: a no-op


def test_bond_deflate_argument_errors():
    L = _lib()
    _h, P = _host_ptr()
    kk, d2 = ctypes.c_int64(0), ctypes.c_double(0.0)

    def bd(side=0, C=P, k=4, n=3, Q=P, m=5, Co=P, Qo=P, kout=True, ws=P, wsb=1 << 20):
        return L.tn_bond_deflate(side, C, k, n, Q, m, Co, Qo, ctypes.byref(kk) if kout else None, ctypes.byref(d2), ws, wsb, None)
    _expect_neg(L, bd(side=2), 'side must be 0')
    _expect_neg(L, bd(side=-1), 'side must be 0')
    for kw in ('C', 'Q', 'Co', 'Qo', 'ws'):
        _expect_neg(L, bd(**{kw: None}), 'null operand')
    _expect_neg(L, bd(kout=False), 'null operand')
    _expect_neg(L, bd(k=0), 'bad dimensions')
    _expect_neg(L, bd(k=257), 'bad dimensions')
    _expect_neg(L, bd(side=1, n=0), 'bad dimensions')
    _expect_neg(L, bd(m=0), 'bad dimensions')
    _expect_neg(L, bd(k=256, wsb=256 * 8 - 8), 'workspace too small')
    _expect_neg(L, bd(side=1, k=3, wsb=23), 'workspace too small')
