"""The rank-32 updates of the QR panel loops through rank_update_kernel (csrc/rank_update.hip, TN_QR_RANK_UPDATE at its default)
against the K = 32 launches of the generic GEMM they replace (TN_QR_RANK_UPDATE=0): every output the same BIT FOR BIT.  The
shapes avoid the one-launch factorisation (<= 64 columns) and the single-workgroup one, so every case runs the panel loops."""
import ctypes as ct

import numpy as np
import pytest

from test_gpu_kernels import _with_env, check_qr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

PLAIN_SHAPES = [(200, 100), (333, 97), (96, 160)]       # (333, 97): row remainder, last panel of one column; (96, 160): m < n


@pytest.fixture(scope='module')
def ops():
    from tnac4o_amd import ops as o
    return o


def both(fn):
    """fn() with the rank-update kernel and with the generic launches."""
    return _with_env('TN_QR_RANK_UPDATE', '1', fn), _with_env('TN_QR_RANK_UPDATE', '0', fn)


def rn(seed, *shape):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator(device='cpu').manual_seed(seed))


def plain_input(shape, colmajor):
    m, n = shape
    return rn(7 * m + n, n, m).cuda().t() if colmajor else rn(7 * m + n, m, n).cuda()


@pytest.mark.parametrize('colmajor', [False, True])
@pytest.mark.parametrize('shape', PLAIN_SHAPES)
def test_plain_blocked_qr(ops, shape, colmajor):
    """Single-level tn_qr: the trailing updates of the forward loop and the per-panel Q accumulation (m k <= 256 * 512 folds the
    last reflector, so the merged form is not taken)."""
    T = plain_input(shape, colmajor)
    assert T.stride(0 if colmajor else 1) == 1
    (Q1, R1), (Q0, R0) = both(lambda: ops.qr(T))
    assert torch.equal(Q1, Q0) and torch.equal(R1, R0)


@pytest.mark.parametrize('shape', PLAIN_SHAPES)
def test_plain_blocked_qr_against_numpy(ops, shape):
    """Switch on: orthogonality and column-relative residual within the bounds of the tn_qr tests (check_qr of test_gpu_kernels)."""
    T = rn(7 * shape[0] + shape[1], *shape).numpy()
    _with_env('TN_QR_RANK_UPDATE', '1', lambda: check_qr(ops, T))


def test_merged_q_accumulation_is_reached(ops):
    """640 x 300: the trailing updates go through the kernel, Q through the merged reflectors (rank-128 products, generic GEMM)."""
    T = rn(11, 640, 300).cuda()
    (Q1, R1), (Q0, R0) = both(lambda: ops.qr(T))
    assert torch.equal(Q1, Q0) and torch.equal(R1, R0)


def test_two_level_blocking(ops):
    """1024 x 512 with outer blocks of 128 columns: the inner updates of qr_two_level."""
    T = rn(12, 1024, 512).cuda()
    (Q1, R1), (Q0, R0) = both(lambda: _with_env('TN_QR_NBO', '128', lambda: ops.qr(T)))
    assert torch.equal(Q1, Q0) and torch.equal(R1, R0)


@pytest.mark.parametrize('side', [0, 1])
def test_truncating_site_qr(ops, side):
    """tn_site_qr with rank_tol on a matrix of rank 50 (320 x 160, five panels): the rank-revealing exit fires after the second panel.
    side 0 factors the row-major (Dl p) x Dr matrix, side 1 the column-major (p Dr) x Dl one."""
    B = rn(13 + side, 320, 50) @ rn(15 + side, 50, 160)
    A = (B.contiguous().view(40, 8, 160) if side == 0 else B.t().contiguous().view(160, 8, 40)).cuda()

    def run():
        info = {}
        Q, R, k, _ = ops.site_qr(side, A.clone(), None, rank_tol=1e-10, normalise=False, info=info)
        return Q, R, k, info['dropped2']
    (Q1, R1, k1, d1), (Q0, R0, k0, d0) = both(run)
    assert k1 == k0 and 50 <= k1 < 160
    assert torch.equal(Q1, Q0) and torch.equal(R1, R0) and d1 == d0


@pytest.mark.parametrize('pivot_device', ['1', '0'])
@pytest.mark.parametrize('shape', [(256, 16, 24, 40), (300, 8, 33, 70)])
def test_pivoted_site_qr(ops, shape, pivot_device):
    """The pivoted, truncating factorisation of the weighted first pass (inputs of test_pivoted_site_qr_device_selection).  With the
    pivots chosen on the device the launches enqueued behind the exit meet *active == 0 and must leave the matrix alone."""
    Dl, p, r, keep = shape
    g = torch.Generator(device='cpu').manual_seed(5 + Dl)
    m = p * r
    nr = min(Dl, m, 3 * keep)
    U = torch.linalg.qr(torch.randn((Dl, nr), generator=g, dtype=torch.float64))[0]
    V = torch.linalg.qr(torch.randn((m, nr), generator=g, dtype=torch.float64))[0]
    sv = torch.logspace(0, -20, nr, dtype=torch.float64)
    B = ((U * sv[None, :]) @ V.t())
    B = B[torch.argsort(B.norm(dim=1), descending=True)].contiguous()
    tol = float(sv[min(keep, nr - 1)])

    def run():
        info = {}
        Qt, Ct, k, _ = ops.site_qr(1, B.cuda().view(Dl, p, r).clone(), None, rank_tol=tol, normalise=False, info=info, frobenius_exit=True,
                                   pivot=True)
        return Qt, Ct, k, info['perm'], info['dropped2']
    (Q1, R1, k1, p1, d1), (Q0, R0, k0, p0, d0) = _with_env('TN_PIVOT_DEVICE', pivot_device, lambda: both(run))
    assert k1 == k0 and torch.equal(p1, p0) and d1 == d0
    assert torch.equal(Q1, Q0) and torch.equal(R1, R0)


def test_the_kernel_really_ran(ops):
    """200 x 100 with profiling on the four GEMM tile families: the update is booked under the family the generic launch would have
    used, so the launch counts agree family by family; the kernel books C read AND written, the generic launch only once, so the
    booked bytes differ by exactly 8 sum M N over the updates of the call: the forward loop (m - 32 p) x (n - 32 p), p = 0 .. 3,
    then the Q accumulation backwards over the panels below the folded last one, (m - 32 p) x (k - 32 p), p = 2, 1, 0."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    m, n, nb = 200, 100, 32
    k = min(m, n)
    P = -(-k // nb)
    assert m * k <= 256 * 512                                   # the last reflector is folded into the launch that starts Q
    updates = [(m - nb * p, n - nb * p) for p in range(P)] + [(m - nb * p, k - nb * p) for p in range(P - 2, -1, -1)]
    T = plain_input((m, n), False)

    def counted():
        L.tn_profile_reset()
        L.tn_profile_sample(1)
        L.tn_profile_enable(0xF)
        try:
            ops.qr(T)
            torch.cuda.synchronize()
            calls, nbytes = [], 0.0
            for f in range(4):
                c, ms, fl, by = ct.c_uint64(0), ct.c_double(0), ct.c_double(0), ct.c_double(0)
                assert L.tn_profile_get(f, ct.byref(c), ct.byref(ms), ct.byref(fl), ct.byref(by)) == 0
                calls.append(int(c.value))
                nbytes += by.value
        finally:
            L.tn_profile_enable(0)
        return calls, nbytes
    (calls1, bytes1), (calls0, bytes0) = both(counted)
    assert calls1 == calls0 and sum(calls1) >= len(updates)
    assert bytes1 - bytes0 == 8.0 * sum(M * N for M, N in updates)
