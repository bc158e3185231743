"""The pairs of products through the MPS (x) MPO factors in one launch (csrc/factor_products.hip, tn_factor_products) against the
two tn_gemm launches they replace: every element of the result the same BIT FOR BIT (numpy.array_equal), on random inputs with exact
zeros and negative values.  The shapes are the smallest at which the kernel can go wrong: depths K1 that are no multiple of 4 or of
16 and one full K tile, widths around the 16-column tiles and the 64-column chunk, S tiles of 1, 15, 255 and 256 rows, result rows
around the 32 rows of a wave and the 256 of a slab, more than one workgroup.  Shapes outside the kernel's limits, and first products
whose launch plan splits K, must be reported ineligible and come out of the entry's own two launches with the same bits."""
import ctypes as ct

import numpy as np
import pytest

from test_gpu_kernels import _with_env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

F64 = torch.float64


@pytest.fixture(scope='module')
def L():
    from tnac4o_amd import _lib
    return _lib.lib()


def _st():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(seed, *shape):
    """Normal values, one in eight replaced by an exact zero."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.randn(*shape, dtype=F64, generator=g)
    x[torch.rand(*shape, generator=g) < 0.125] = 0.0
    return x.cuda()


def nans(*shape):
    return torch.full(shape, float('nan'), dtype=F64, device='cuda')


def gemm(L, M, N, K, A, sa, B, sb, C, sc, batch=1, bs=(0, 0, 0), split=False):
    """C = A B through tn_gemm (alpha = 1, beta = 0); split: with the workspace the launch plan asks for, as Chain::mm does."""
    wsb = int(L.tn_gemm_ws_bytes(M, N, K, batch)) if split else 0
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda') if wsb > 0 else None
    rc = L.tn_gemm(M, N, K, 1.0, A.data_ptr(), sa[0], sa[1], B.data_ptr(), sb[0], sb[1], 0.0, C.data_ptr(), sc[0], sc[1], batch, bs[0], bs[1],
                   bs[2], ws.data_ptr() if ws is not None else None, wsb, _st())
    assert rc == 0, rc
    return wsb


def launches(L, fn):
    """fn() with the four GEMM tile families profiled: (launches per family, result)."""
    L.tn_profile_reset()
    L.tn_profile_sample(1)
    L.tn_profile_enable(0xF)
    try:
        out = fn()
        torch.cuda.synchronize()
        calls = []
        for f in range(4):
            c, ms, fl, by = ct.c_uint64(0), ct.c_double(0), ct.c_double(0), ct.c_double(0)
            assert L.tn_profile_get(f, ct.byref(c), ct.byref(ms), ct.byref(fl), ct.byref(by)) == 0
            calls.append(int(c.value))
    finally:
        L.tn_profile_enable(0)
    return calls, out


def fused(L, dims, P, sp, X, sx, W, sw, Out, so, Mhi=1, first_batched=0):
    Z, I, J, K1, N, M = dims
    wsb = int(L.tn_factor_products_ws_bytes(Z, I, J, K1, N, first_batched))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device='cuda')
    rc = L.tn_factor_products(Z, I, J, K1, N, Mhi, M // Mhi, P.data_ptr(), sp[0], sp[1], sp[2], X.data_ptr(), sx[0], sx[1], sx[2], W.data_ptr(),
                              sw[0], sw[1], Out.data_ptr(), so[0], so[1], so[2], so[3], first_batched, ws.data_ptr(), wsb, _st())
    assert rc == 0, rc


def canonical(L, dims, seed, first_batched=0):
    """Contiguous P (Z, I, K1), X (K1, J, N), W (M, I J), Out (Z, M, N): (result of tn_factor_products, result of the two tn_gemm launches,
    GEMM launches the entry made, whether the first tn_gemm split K)."""
    Z, I, J, K1, N, M = dims
    Q = I * J
    P, X, W = rnd(seed, Z, I, K1), rnd(seed + 1, K1, J, N), rnd(seed + 2, M, Q)
    T, ref = nans(Z * I, J * N), nans(Z, M, N)
    if first_batched:
        wsb = gemm(L, Z * I, N, K1, P, (K1, 1), X, (J * N, 1), T, (J * N, 1), batch=J, bs=(0, N, N))
    else:
        wsb = gemm(L, Z * I, J * N, K1, P, (K1, 1), X, (J * N, 1), T, (J * N, 1), split=True)
    gemm(L, M, N, Q, W, (Q, 1), T, (N, 1), ref, (N, 1), batch=Z, bs=(0, Q * N, M * N))
    out = nans(Z, M, N)
    calls, _ = launches(L, lambda: fused(L, dims, P, (I * K1, K1, 1), X, (J * N, N, 1), W, (Q, 1), out, (M * N, 0, N, 1), first_batched=first_batched))
    return out.cpu().numpy(), ref.cpu().numpy(), calls, wsb > 0


#        Z   I   J  K1    N    M
INSIDE = [
    (1, 1, 1, 1, 1, 1),                                                                    # all extents 1
    (3, 5, 3, 1, 33, 17), (3, 5, 3, 3, 33, 17), (3, 5, 3, 17, 33, 17),                     # K1: no multiple of 4, of 16
    (64, 16, 16, 64, 64, 17),                                                              # K1 = 64, one full K tile (256 tiles: the plan does not split)
    (3, 4, 4, 17, 1, 17), (3, 4, 4, 17, 31, 17), (3, 4, 4, 17, 32, 17), (3, 4, 4, 17, 33, 17), (3, 4, 4, 17, 64, 17), (3, 4, 4, 17, 65, 17),
    (3, 1, 1, 17, 33, 17), (3, 3, 5, 17, 33, 17), (3, 15, 17, 17, 33, 17), (3, 16, 16, 17, 33, 17),      # I J = 1, 15, 255, 256
    (3, 4, 4, 17, 33, 1), (3, 4, 4, 17, 33, 255), (3, 4, 4, 17, 33, 256), (3, 4, 4, 17, 33, 272),       # rows of the second product
    (1, 4, 4, 17, 33, 17), (70, 4, 4, 17, 33, 17),                                         # batch
]


@pytest.mark.parametrize('dims', INSIDE, ids=lambda d: 'x'.join(map(str, d)))
def test_one_launch_same_bits(L, dims):
    Z, I, J, K1, N, M = dims
    assert L.tn_factor_products_eligible(Z, I, J, K1, N, M, 0) == 1
    out, ref, calls, split = canonical(L, dims, 1000 + sum(dims))
    assert not split and np.isfinite(ref).all()
    assert calls == [0, 0, 0, 1]                      # one launch, booked with the 64 x 64 family
    assert np.array_equal(out, ref)


@pytest.mark.parametrize('dims', [(3, 1, 257, 17, 33, 17), (3, 17, 2, 17, 33, 17), (3, 4, 4, 65, 33, 17)], ids=lambda d: 'x'.join(map(str, d)))
def test_outside_the_limits_falls_back(L, dims):
    """More than 256 rows of S, more than 16 rows i, K1 beyond 64: not eligible; the entry's own two launches give the same bits."""
    assert L.tn_factor_products_eligible(*dims, 0) == 0
    out, ref, calls, _ = canonical(L, dims, 2000 + sum(dims))
    assert sum(calls) == 2 and np.isfinite(ref).all()
    assert np.array_equal(out, ref)


def test_split_first_product_is_not_eligible(L):
    """15 x 99 x 64: two tiles, so the launch plan cuts K = 64 in two -- another summation order than the kernel's.  The same
    operation with the first product batched over j (no workspace, never split) is eligible."""
    dims = (3, 5, 3, 64, 33, 17)
    assert L.tn_gemm_ws_bytes(15, 99, 64, 1) > 0
    assert L.tn_factor_products_eligible(*dims, 0) == 0 and L.tn_factor_products_eligible(*dims, 1) == 1
    out, ref, calls, split = canonical(L, dims, 31)
    assert split and sum(calls) == 2 and np.array_equal(out, ref)
    out, ref, calls, split = canonical(L, dims, 31, first_batched=1)
    assert not split and calls == [0, 0, 0, 1] and np.array_equal(out, ref)


def test_switch_restores_the_two_launches(L):
    dims = (3, 4, 4, 17, 33, 17)
    out, ref, calls, _ = _with_env('TN_FACTOR_FUSED', '0', lambda: canonical(L, dims, 32))
    assert sum(calls) == 2 and np.array_equal(out, ref)


def test_gram_step_shape(L):
    """T2 = Wx (Gp A) as Chain::gram_step_structured issues it: ba = 2, Dl = 5, ps = 3, Dr = 7, pt bb = 10; z = (alpha, l), Wx q-major."""
    ba, Dl, ps, Dr, M = 2, 5, 3, 7, 10
    na, Q = Dl * ba, ba * ps
    Gp, Af, Wxt = rnd(41, na, ba, Dl), rnd(42, Dl, ps, Dr), rnd(43, Q, M)
    T1, ref = nans(na * ba, ps * Dr), nans(na, M, Dr)
    gemm(L, na * ba, ps * Dr, Dl, Gp, (Dl, 1), Af, (ps * Dr, 1), T1, (ps * Dr, 1), split=True)
    gemm(L, M, Dr, Q, Wxt, (1, M), T1, (Dr, 1), ref, (Dr, 1), batch=na, bs=(0, Q * Dr, M * Dr))
    out = nans(na, M, Dr)
    dims = (na, ba, ps, Dl, Dr, M)
    assert L.tn_factor_products_eligible(*dims, 0) == 1
    calls, _ = launches(L, lambda: fused(L, dims, Gp, (ba * Dl, Dl, 1), Af, (ps * Dr, Dr, 1), Wxt, (1, M), out, (M * Dr, 0, Dr, 1)))
    assert calls == [0, 0, 0, 1] and np.array_equal(out.cpu().numpy(), ref.cpu().numpy())


@pytest.mark.parametrize('hconj', [1, 0])
def test_attach_shape(L, hconj):
    """M = Wq (A C) as Chain::attach_through_factors issues it, r = 100 columns (two chunks): z = alpha, i = s, k = beta, j = rb.  With
    Hconj C is read as (beta rb) x r' and the result is (alpha, l, t, r'); without, C is (rb beta) x r', the first product is batched
    over rb and the rows (l, t) of item alpha go to (l, alpha, t, r'): compared with tn_gemm + tn_gemm + the permutation in numpy."""
    Dl, ps, Dr, ba, bb, pt, r = 3, 2, 5, 2, 3, 2, 100
    Q, M = ps * bb, ba * pt
    A, C, Wqt = rnd(51, Dl, ps, Dr), rnd(52, Dr * bb, r), rnd(53, Q, M)
    T, Mt = nans(Dl * ps, bb * r), nans(Dl, M, r)
    if hconj:
        gemm(L, Dl * ps, bb * r, Dr, A, (Dr, 1), C, (bb * r, 1), T, (bb * r, 1), split=True)
        sx, so, Mhi = (bb * r, r, 1), (M * r, 0, r, 1), 1
    else:
        gemm(L, Dl * ps, r, Dr, A, (Dr, 1), C, (r, 1), T, (bb * r, 1), batch=bb, bs=(0, Dr * r, r))
        sx, so, Mhi = (r, Dr * r, 1), (pt * r, Dl * pt * r, r, 1), ba
    gemm(L, M, r, Q, Wqt, (1, M), T, (r, 1), Mt, (r, 1), batch=Dl, bs=(0, Q * r, M * r))
    ref = Mt.cpu().numpy()
    if not hconj:
        ref = np.ascontiguousarray(ref.reshape(Dl, ba, pt, r).transpose(1, 0, 2, 3))
    out = nans(*ref.shape)
    dims = (Dl, ps, bb, Dr, r, M)
    assert L.tn_factor_products_eligible(*dims, 0 if hconj else 1) == 1
    calls, _ = launches(L, lambda: fused(L, dims, A, (ps * Dr, Dr, 1), C, sx, Wqt, (1, M), out, so, Mhi=Mhi, first_batched=0 if hconj else 1))
    assert calls == [0, 0, 0, 1] and np.isfinite(ref).all() and np.array_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize('hconj', [True, False])
def test_chain_driver_same_bits_with_and_without(hconj):
    """tn_compress_mps on the smallest chain whose rows reach the structured path (the weighted first pass needs an absorbed bond of
    512, its structured Gram step and the attach through the factors one of 256: MPS bonds 16, 32, 16 times MPO bonds 16) with
    TN_FACTOR_FUSED = 1 and 0: site tensors, bond dimensions, overlap and discarded weights equal bit for bit.  The `attach_fused`
    count of the returned info says that the attach went through the factors."""
    from tnac4o_amd import ops
    Dm, Do, p = [1, 16, 32, 16, 1], [1, 16, 16, 16, 1], 2
    sites = [rnd(60 + n, Dm[n], p, Dm[n + 1]) for n in range(4)]
    mpo = [rnd(70 + n, Do[n], p, Do[n + 1], p) for n in range(4)]

    def run():
        return ops.compress_mps_native(sites, mpo, hconj, 8, 1e-16, 1e-10, 4, True)
    a, b = _with_env('TN_FACTOR_FUSED', '1', run), _with_env('TN_FACTOR_FUSED', '0', run)
    assert a['info']['weighted_used'] and a['info']['attach_fused'] >= 2 and a['info']['attach_fused'] == b['info']['attach_fused']
    assert [tuple(t.shape) for t in a['A']] == [tuple(t.shape) for t in b['A']]
    assert all(torch.equal(x, y) for x, y in zip(a['A'], b['A']))
    assert a['overlap'] == b['overlap'] and a['discarded'] == b['discarded']
