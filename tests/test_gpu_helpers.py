"""GPU tests of the helper kernels of the weighted first pass and of bond deflation (tn_argsort_desc, tn_weighted_sum,
tn_rows_norm2, tn_gram_weights, tn_gather_scale_rows, tn_bond_deflate, tn_scale_phys) against the exact references of
tests/helpers_ref.py.  Every export is called through the C-ABI with each output framed by guard bytes (tests/guarded.py) and
pre-filled with NaN, so a write past an output or an element left unwritten shows."""
import ctypes as ct

import numpy as np
import pytest

import helpers_ref as hr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
from guarded import Guarded, same_bits  # noqa: E402

F64 = torch.float64
SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 513, 8192)
SENT = 0x5A                        # sentinel byte of outputs that must stay untouched


@pytest.fixture(scope='module')
def L():
    from tnac4o_amd import _lib
    return _lib.lib()


def _st(stream=None):
    return ct.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def dev(x, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def _msg(L):
    buf = ct.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    return buf.value.decode()


# ---------------------------------------------------------------------------------------------------------- tn_argsort_desc
def _argsort_inputs(n, rng):
    cases = {'spread': hr.spread(rng, n), 'equal': np.full(n, 0.75)}
    t = np.round(rng.standard_normal(n) * 2.0)                  # exact ties, +0.0 and -0.0 among them
    z = t == 0
    t[z] = np.where(rng.random(int(z.sum())) < 0.5, 0.0, -0.0)
    cases['ties'] = t
    s = hr.spread(rng, n)
    s[-1] = np.nan
    cases['nan_last'] = s
    if n >= 4:
        x = hr.spread(rng, n)
        x[rng.choice(n, 4, replace=False)] = [np.inf, -np.inf, np.nan, np.nan]
        cases['inf_nan'] = x
    return cases


@pytest.mark.parametrize('n', SIZES)
def test_argsort_desc_exact(L, n):
    """The permutation equals the rule exactly: descending, NaN first, equal values (+0.0 == -0.0) by increasing index."""
    rng = np.random.default_rng(n)
    for name, x in _argsort_inputs(n, rng).items():
        w = dev(x)
        out = Guarded.of(torch.int64, (n,))
        assert L.tn_argsort_desc(w.data_ptr(), n, out.ptr, _st()) == 0, _msg(L)
        torch.cuda.synchronize()
        assert out.intact(), name
        assert np.array_equal(out.host(), hr.argsort_desc_ref(x)), name


# ---------------------------------------------------------------------------------------------------------- tn_weighted_sum
@pytest.mark.parametrize('n', SIZES)
def test_weighted_sum_bound_and_reproducible(L, n):
    """w = a * b bit for bit; the sum within the bound of the documented order (256 strided partial sums, then a binary tree) of
    the EXACT sum of the exact products; bit-identical over 10 calls and on a second stream.  (No bit comparison with a numpy
    emulation of the order: the device may fuse the multiply into the addition.)"""
    rng = np.random.default_rng(1000 + n)
    h = rng.standard_normal(n // 2)
    inputs = {'spread': (hr.spread(rng, n), hr.spread(rng, n)),
              'normal': (rng.standard_normal(n), rng.standard_normal(n)),
              'cancel': (np.concatenate([h, -h[::-1], np.ones(n % 2)]), np.ones(n))}
    side = torch.cuda.Stream()
    for name, (a, b) in inputs.items():
        ad, bd = dev(a), dev(b)
        w_ref, S, T = hr.weighted_sum_ref(a, b)
        sums = []
        for rep in range(12):
            stream = side if rep >= 10 else torch.cuda.current_stream()
            w, s = Guarded.of(F64, (n,)), Guarded.of(F64, (1,))
            torch.cuda.synchronize()
            assert L.tn_weighted_sum(ad.data_ptr(), bd.data_ptr(), n, w.ptr, s.ptr, _st(stream)) == 0, _msg(L)
            torch.cuda.synchronize()
            assert w.intact() and s.intact(), name
            assert same_bits(w.host(), w_ref), name
            sums.append(s.host()[0])
        assert len({x.tobytes() for x in sums}) == 1, (name, sums)
        assert hr.within(sums[0], S, hr.weighted_sum_bound(n, T)), (name, sums[0], float(S))


def test_weighted_sum_special_values(L):
    a = np.array([1.0, -0.0, np.inf, 2.0, 0.0] * 60)
    b = np.array([-0.0, 3.0, 1.0, np.nan, -5.0] * 60)
    for aa, bb, expect in ((a, b, 'nan'), (np.array([1.0, np.inf, -2.0]), np.ones(3), 'inf'), (np.array([-0.0] * 3), np.ones(3), 'zero')):
        n = aa.size
        w, s = Guarded.of(F64, (n,)), Guarded.of(F64, (1,))
        ad, bd = dev(aa), dev(bb)
        assert L.tn_weighted_sum(ad.data_ptr(), bd.data_ptr(), n, w.ptr, s.ptr, _st()) == 0, _msg(L)
        torch.cuda.synchronize()
        assert w.intact() and s.intact()
        got, ref = w.host(), aa * bb
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        assert same_bits(got[ok], ref[ok])                      # signed zeros and infinities included
        sv = s.host()[0]
        assert {'nan': np.isnan(sv), 'inf': sv == np.inf, 'zero': sv == 0.0}[expect], sv


# ---------------------------------------------------------------------------------------------------------- tn_rows_norm2
@pytest.mark.parametrize('cols', (1, 255, 256, 257, 511, 512, 513, 100000))
def test_rows_norm2_bound(L, cols):
    """Within gamma_D of the exact sum of squares, D = ceil(cols/256) + 10 roundings per term (the thread's accumulator, s0 + s1,
    6 shuffle levels, 2 levels over the waves, the square itself); a row of small integers is exact."""
    rng = np.random.default_rng(cols)
    A = np.stack([hr.spread(rng, cols), rng.standard_normal(cols), rng.integers(-3, 4, cols).astype(np.float64)])
    rows = A.shape[0]
    Ad = dev(A)
    out = Guarded.of(F64, (rows,))
    assert L.tn_rows_norm2(Ad.data_ptr(), rows, cols, out.ptr, _st()) == 0, _msg(L)
    torch.cuda.synchronize()
    assert out.intact()
    got = out.host()
    ex = hr.rows_norm2_ref(A)
    for r in range(rows):
        assert hr.within(got[r], ex[r], hr.rows_norm2_bound(cols, ex[r])), (r, got[r], float(ex[r]))
    assert got[2] == float(ex[2])
    z = Guarded.of(F64, (4,), SENT)                              # rows = 0: a no-op
    assert L.tn_rows_norm2(Ad.data_ptr(), 0, cols, z.ptr, _st()) == 0
    torch.cuda.synchronize()
    assert z.intact() and z.untouched(SENT)


# ---------------------------------------------------------------------------------------------------------- tn_gram_weights
def _gram_call(L, G, floor_rel):
    n = G.shape[0]
    Gd = dev(G)
    d2, st = Guarded.of(F64, (n,)), Guarded.of(F64, (65,))
    assert L.tn_gram_weights(Gd.data_ptr(), n, floor_rel, d2.ptr, st.ptr, _st()) == 0, _msg(L)
    torch.cuda.synchronize()
    assert d2.intact() and st.intact()
    return d2.host(), st.host()


@pytest.mark.parametrize('n', (1, 63, 64, 65, 1000, 4096))
@pytest.mark.parametrize('floor_rel', (0.0, 1e-12))
def test_gram_weights(L, n, floor_rel):
    """d2 = max(G_cc, floor_rel max G_cc) and stats[64] = max G_cc bit for bit; the 64 partial sums added in order within the bound
    of gram_kfro_bound of ||G / (d d^T)||_F^2; the parts beyond the last row block are exactly zero; bit-identical on a repeat."""
    rng = np.random.default_rng(n + 7)
    B = rng.standard_normal((n, 24)) * 10.0 ** rng.uniform(-50, 50, n)[:, None]      # diagonal over 1e-100 .. 1e100
    G = B @ B.T
    d2, st = _gram_call(L, G, floor_rel)
    d2b, stb = _gram_call(L, G, floor_rel)
    assert same_bits(d2, d2b) and same_bits(st, stb)
    d2_ref, gmax = hr.gram_weights_ref(G, floor_rel)
    assert same_bits(d2, d2_ref)
    assert same_bits(st[64:], np.array([gmax]))
    if floor_rel > 0 and n > 1:
        assert (np.diagonal(G) < gmax * floor_rel).any()        # the floor is exercised
    rows_per = -(-n // hr.GW_PARTS)
    used = -(-n // rows_per)
    assert np.all(st[used:64] == 0.0)
    tot = 0.0
    for x in st[:64]:
        tot += float(x)
    kf = hr.gram_kfro_ref(G, d2_ref)
    assert abs(tot - kf) <= hr.gram_kfro_bound(n, kf), (tot, kf)


def test_gram_weights_all_zero(L):
    """The documented precondition: an all-zero G yields d2 = 0, stats[64] = 0 (how a caller recognises it) and NaN partial sums
    for the row blocks that hold rows."""
    n = 5
    d2, st = _gram_call(L, np.zeros((n, n)), 1e-12)
    assert np.all(d2 == 0.0) and st[64] == 0.0
    assert np.all(np.isnan(st[:n])) and np.all(st[n:64] == 0.0)


# ---------------------------------------------------------------------------------------------------------- tn_gather_scale_rows
@pytest.mark.parametrize('cols', (1, 255, 256, 257, 4096))
def test_gather_scale_rows(L, cols):
    """Forward bit-exact to sqrt(w2[perm]) A[perm] and inverse to A / sqrt(w2[perm]) scattered by perm (the device's sqrt and
    division are correctly rounded); forward then inverse returns A within 3 ulps (three roundings: the product, 1/sqrt, the
    second product)."""
    rng = np.random.default_rng(cols + 3)
    rows = 37
    A = hr.spread(rng, rows * cols).reshape(rows, cols)
    perm = rng.permutation(rows)
    w2 = 10.0 ** rng.uniform(-100, 100, rows)
    Ad, pdv, wd = dev(A), dev(perm, torch.int64), dev(w2)
    F = Guarded.of(F64, (rows, cols))
    assert L.tn_gather_scale_rows(Ad.data_ptr(), rows, cols, pdv.data_ptr(), wd.data_ptr(), F.ptr, 0, _st()) == 0, _msg(L)
    B = Guarded.of(F64, (rows, cols))
    assert L.tn_gather_scale_rows(F.ptr, rows, cols, pdv.data_ptr(), wd.data_ptr(), B.ptr, 1, _st()) == 0, _msg(L)
    torch.cuda.synchronize()
    assert F.intact() and B.intact()
    Fh, Bh = F.host(), B.host()
    assert same_bits(Fh, hr.gather_scale_rows_ref(A, perm, w2))
    assert same_bits(Bh, hr.gather_scale_rows_ref(Fh, perm, w2, inverse=True))
    assert hr.ulps(Bh, A).max() <= 3
    z = Guarded.of(F64, (4,), SENT)                              # rows = 0: a no-op
    for inv in (0, 1):
        assert L.tn_gather_scale_rows(Ad.data_ptr(), 0, cols, pdv.data_ptr(), wd.data_ptr(), z.ptr, inv, _st()) == 0
    torch.cuda.synchronize()
    assert z.intact() and z.untouched(SENT)


# ---------------------------------------------------------------------------------------------------------- tn_bond_deflate
def _deflate(L, side, C, Q):
    k = C.shape[0] if side == 0 else C.shape[1]
    n = C.shape[1] if side == 0 else C.shape[0]
    m = Q.shape[0] if side == 0 else Q.shape[1]
    Cd, Qd = dev(C), dev(Q)
    Co, Qo, ws = Guarded.of(F64, C.shape, SENT), Guarded.of(F64, Q.shape, SENT), Guarded(k * 8)
    kk, d2 = ct.c_int64(-1), ct.c_double(-1.0)
    rc = L.tn_bond_deflate(side, Cd.data_ptr(), k, n, Qd.data_ptr(), m, Co.ptr, Qo.ptr, ct.byref(kk), ct.byref(d2), ws.ptr, k * 8, _st())
    torch.cuda.synchronize()
    assert Co.intact() and Qo.intact() and ws.intact()
    return rc, kk.value, d2.value, Co, Qo


def _check_deflate(L, side, C, Q, expect_kept=None, expect_rel=None):
    """Run tn_bond_deflate and compare with the rule of helpers_ref on the exact squared norms (the inputs are small integers times
    powers of two, so the device's norms are exact too and the decision is not left to rounding)."""
    h = hr.bond_norms2(side, C)
    rc_ref, kept, rel = hr.bond_deflate_ref(h)
    if expect_kept is not None:
        assert (kept, rel) == (expect_kept, expect_rel)          # the case is built as intended
    rc, kk, d2, Co, Qo = _deflate(L, side, C, Q)
    if rc_ref == -2:
        assert rc == -2 and 'non-finite' in _msg(L), (rc, _msg(L))
        assert Co.untouched(SENT) and Qo.untouched(SENT)
        return None
    assert rc == 0, _msg(L)
    k = len(h)
    assert kk == len(kept)
    if kk == k:                                                  # nothing written
        assert Co.untouched(SENT) and Qo.untouched(SENT) and d2 == 0.0
        return kept
    Cref, Qref = hr.bond_deflate_apply(side, C, Q, kept)
    assert same_bits(Co.host(F64, (-1,))[:Cref.size].reshape(Cref.shape), Cref)
    assert same_bits(Qo.host(F64, (-1,))[:Qref.size].reshape(Qref.shape), Qref)
    assert Co.untouched(SENT, Cref.size * 8) and Qo.untouched(SENT, Qref.size * 8)
    assert d2 == rel
    dropped = [i for i in range(k) if i not in kept]            # the state moves by at most eps^2 max_i ||C_i||^2
    assert hr.exact_sum(h[dropped]) <= hr.exact_sum([hr.EPS ** 2 * h.max()])
    return kept


def _bond(side, slices):
    """C from its bond slices: rows (side 0) or columns (side 1)."""
    S = np.array(slices, dtype=np.float64)
    return S if side == 0 else np.ascontiguousarray(S.T)


def _site(side, k, m, rng):
    return hr.spread(rng, m * k, 30).reshape((m, k) if side == 0 else (k, m))


@pytest.mark.parametrize('side', (0, 1))
def test_bond_deflate_budget_edge(L, side):
    rng = np.random.default_rng(11 + side)
    t = 2.0 ** -47                                               # t^2 = 2^-94;  nmax = 2^11 -> budget eps^2 nmax = 2^-93
    on = [[32, 32, 0], [t, 0, 0], [2, 0, 0], [0, t, 0], [1, 0, 0], [0, 0, 3]]
    _check_deflate(L, side, _bond(side, on), _site(side, 6, 300, rng), [0, 2, 4, 5], 2.0 ** -104)          # exactly on the budget
    over = [[32, 32, 0], [t, 0, 0], [2, 0, 0], [2.0 ** -72, t, 0], [1, 0, 0], [0, 0, 3]]
    _check_deflate(L, side, _bond(side, over), _site(side, 6, 300, rng), [0, 2, 3, 4, 5], 2.0 ** -105)     # 2^-144 past it
    tie = [[32, 0, 0], [t, 0, 0], [2, 0, 0], [0, t, 0], [1, 0, 0], [0, 0, 3]]
    _check_deflate(L, side, _bond(side, tie), _site(side, 6, 300, rng), [0, 2, 3, 4, 5], 2.0 ** -104)      # room for one of the tie


@pytest.mark.parametrize('side', (0, 1))
def test_bond_deflate_ties_by_index(L, side):
    rng = np.random.default_rng(21 + side)
    s = 2.0 ** -48                                               # 2^-96 each: eight of the ten fit into 2^-93
    sl = [[0] * 5 for _ in range(12)]
    for j, i in enumerate([0, 1, 2, 3, 4, 6, 7, 8, 9, 10]):
        sl[i][j % 5] = s
    sl[5] = [32, 32, 0, 0, 0]
    sl[11] = [0, 0, 0, 0, 1]
    _check_deflate(L, side, _bond(side, sl), _site(side, 12, 77, rng), [5, 9, 10, 11], 2.0 ** -104)


@pytest.mark.parametrize('side', (0, 1))
def test_bond_deflate_degenerate(L, side):
    rng = np.random.default_rng(31 + side)
    one = [[0, 0], [0, 0], [0, 0], [1, 2], [0, 0], [0, 0], [0, 0]]   # all negligible but one: k - 1 dropped
    _check_deflate(L, side, _bond(side, one), _site(side, 7, 65, rng), [3], 0.0)
    _check_deflate(L, side, _bond(side, [[3, 4, 5]]), _site(side, 1, 65, rng), [0], 0.0)                    # k = 1
    _check_deflate(L, side, _bond(side, [[0, 0, 0]] * 5), _site(side, 5, 65, rng), [0, 1, 2, 3, 4], 0.0)    # all zero
    for bad in (np.nan, np.inf):
        sl = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
        sl[1][2] = bad
        assert _check_deflate(L, side, _bond(side, sl), _site(side, 3, 65, rng)) is None


def _int_slices(rng, k, n, tiny):
    """k bond slices of n small integers; the slices listed in `tiny` scaled by 2^-60 (negligible, exact squares)."""
    S = rng.integers(-3, 4, (k, n)).astype(np.float64)
    S[:, 0] = np.where(S[:, 0] == 0, 1.0, S[:, 0])              # no all-zero slice
    S[list(tiny)] *= 2.0 ** -60
    return S


@pytest.mark.parametrize('side', (0, 1))
def test_bond_deflate_k256(L, side):
    rng = np.random.default_rng(41 + side)
    k, n, m = 256, 300, 513
    tiny = [i for i in range(1, 255) if i % 3 == 0]
    S = _int_slices(rng, k, n, tiny)
    kept = _check_deflate(L, side, _bond(side, S), _site(side, k, m, rng))
    assert kept == [i for i in range(k) if i not in tiny]


@pytest.mark.parametrize('side', (0, 1))
def test_bond_deflate_grid_stride(L, side):
    """m k' > 2048 x 256 gathered elements: the grid-stride branch of gather_cols_idx_kernel runs (side 0: Q m x k by columns,
    side 1: C n x k by columns)."""
    rng = np.random.default_rng(51 + side)
    k = 64
    n, m = (40, 16384) if side == 0 else (16384, 40)
    S = _int_slices(rng, k, n, (3, 17, 40))
    kept = _check_deflate(L, side, _bond(side, S), _site(side, k, m, rng))
    assert len(kept) == 61 and (m if side == 0 else n) * len(kept) > 2048 * 256


# ---------------------------------------------------------------------------------------------------------- tn_scale_phys
@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 4, 65), (7, 2, 257), (5, 3, 1), (300, 4, 2000)])
@pytest.mark.parametrize('inv', (0, 1))
def test_scale_phys_exact(L, shape, inv):
    """A * diag[s] / A / diag[s] bit for bit over (Dl, p, Dr); 300 x 4 x 2000 > 2048 x 1024 runs the grid-stride loop more than once."""
    rng = np.random.default_rng(sum(shape) + inv)
    Dl, p, Dr = shape
    A = hr.spread(rng, Dl * p * Dr, 50).reshape(shape)
    diag = hr.spread(rng, p + 1, 50)
    g = Guarded.of(F64, shape)
    g.tensor().copy_(dev(A))
    dd = dev(diag)
    assert L.tn_scale_phys(g.ptr, Dl, p, Dr, dd.data_ptr(), inv, _st()) == 0, _msg(L)
    torch.cuda.synchronize()
    assert g.intact()
    assert same_bits(g.host(), hr.scale_phys_ref(A, diag, inv))
