"""The launch classes of tn_gemm that no other direct test reaches, each against numpy.

plan_gemm (csrc/gemm_f64.hip) picks the tile and the K split from M N K batch.  Every shape of test_gpu_kernels.py and
test_gpu_workspace.py stays below 2^30 multiply-adds and runs as 64 x 64, 128 x 32 or 32 x 128; the 128 x 128 tile (two
workgroups per CU, a two-slab prefetch of C in the beta epilogue), the split of the large products, the transposed product for a
column-major C, the grid.z slicing of long batches, beta through splitk_reduce, K = 0 and zero operand strides are reached here.
A case that names a class asserts it: the profile counters (families 0-3 the tiles, 4 splitk_reduce; the flops booked for family 4
are splits x M x N x batch) and tn_gemm_ws_bytes.  The classes were derived from plan_gemm at its defaults, so those cases are
skipped when a TN_GEMM_* variable is set (the plan reads them once per process).

References and bounds.  Integer-valued operands in [-3, 3]: every partial sum is an integer far below 2^53, whatever the
summation order, so the result must be BIT-EQUAL to numpy's.  Random-normal operands (u = 2^-53, gamma_m = m u / (1 - m u)): a
product of depth K in any summation order obeys |got - ref| <= gamma_(K+1) |A| |B| (steps_ref.gamma); with alpha and beta every term
passes one scaling and one addition more, |got - ref| <= gamma_(K+3) (|alpha| |A| |B| + |beta| |C0|).  The reference is longdouble,
except for the sampled items of the big batched product, which are compared with float64 numpy under twice the bound.

Every bounded case prints its largest error / bound (pytest -s); a ratio near 1 would mean the bound does no work, above 1 fails.
"""
import ctypes as ct
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
import steps_ref as sr  # noqa: E402

F64 = torch.float64
LD = np.longdouble
TILE_FAMILIES = (0, 1, 2, 3)          # gemm_kernel<128,128> / <128,32> / <32,128> / <64,64>
SPLITK = 4


@pytest.fixture(scope='module')
def L():
    from tnac4o_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def ops():
    from tnac4o_amd import ops as o
    return o


@pytest.fixture(scope='module')
def plan_defaults():
    names = sorted(k for k in os.environ if k.startswith('TN_GEMM_'))
    if names:
        pytest.skip('%s set: the launch classes of these cases were derived from the defaults of plan_gemm' % ', '.join(names))


def _st():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=F64).cuda()


def host(t):
    return t.detach().cpu().numpy()


def ints(rng, *shape):
    return rng.integers(-3, 4, shape).astype(np.float64)


def nan_tensor(*shape):
    return torch.full(shape, float('nan'), dtype=F64, device='cuda')


def _msg(L):
    buf = ct.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    return buf.value.decode()


def gemm(L, M, N, K, alpha, A, sa, B, sb, beta, C, sc, batch=1, bs=(0, 0, 0), ws=None, wsb=0):
    """tn_gemm on torch tensors with explicit (row, column) strides per operand and batch strides (bsa, bsb, bsc)."""
    rc = L.tn_gemm(M, N, K, alpha, A.data_ptr(), sa[0], sa[1], B.data_ptr(), sb[0], sb[1], beta, C.data_ptr(), sc[0], sc[1], batch,
                   bs[0], bs[1], bs[2], ws.data_ptr() if ws is not None else None, wsb, _st())
    assert rc == 0, (rc, _msg(L))


def workspace(L, M, N, K, batch):
    wsb = int(L.tn_gemm_ws_bytes(M, N, K, batch))
    return (torch.empty(wsb, dtype=torch.uint8, device='cuda') if wsb > 0 else None), wsb


class Counters:
    """Launch counts and booked flops of the GEMM families around a block of calls; profiling is switched off again whatever happens."""

    def __init__(self, L):
        self.L, self.calls, self.flops = L, {}, {}

    def __enter__(self):
        self.L.tn_profile_reset()
        self.L.tn_profile_enable(0x1F)
        return self

    def __exit__(self, *exc):
        try:
            torch.cuda.synchronize()
            for f in TILE_FAMILIES + (SPLITK,):
                c, ms, fl, by = ct.c_uint64(0), ct.c_double(0), ct.c_double(0), ct.c_double(0)
                assert self.L.tn_profile_get(f, ct.byref(c), ct.byref(ms), ct.byref(fl), ct.byref(by)) == 0
                self.calls[f], self.flops[f] = int(c.value), fl.value
        finally:
            self.L.tn_profile_enable(0)
        return False

    def tiles(self):
        return {f: self.calls[f] for f in TILE_FAMILIES if self.calls[f]}

    def splits(self, M, N, batch=1):
        """Split count of the one splitk_reduce launch (its booked flops are splits x M x N x batch)."""
        assert self.calls[SPLITK] == 1, self.calls
        return self.flops[SPLITK] / (M * N * batch)


RATIOS = {}


def within(name, got, ref, absref, g):
    """|got - ref| <= g absref elementwise; prints the largest error / bound of the case (recorded in the module docstring)."""
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
    bound = g * np.asarray(absref, dtype=LD)
    assert np.all(bound > 0)
    ratio = float((err / bound).max())
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print('error/bound %-28s %.3f (largest so far %.3f)' % (name, ratio, RATIOS[name]))
    assert ratio <= 1.0, (name, ratio)


# ------------------------------------------------------------------------------------------------ the 128 x 128 tile, batched
BM, BN, BK, BB = 130, 130, 72, 890          # 2 x 2 tiles x 890 items = 3560 workgroups, 1.008 x 2^30 multiply-adds: no split


@pytest.fixture(scope='module')
def batched_int():
    """One shared A (bsa = 0), B per item, an integer C0; the product computed once."""
    rng = np.random.default_rng(130)
    A, B, C0 = ints(rng, BM, BK), ints(rng, BB, BK, BN), ints(rng, BB, BM, BN)
    return dict(A=A, B=B, C0=C0, AB=np.matmul(A, B), Ad=dev(A), Bd=dev(B))


def test_big_tile_batched_no_split(L, plan_defaults, batched_int):
    d = batched_int
    assert BM * BN * BK * BB >= 2 ** 30 and L.tn_gemm_ws_bytes(BM, BN, BK, BB) == 0
    C = nan_tensor(BB, BM, BN)
    with Counters(L) as pc:
        gemm(L, BM, BN, BK, 1.0, d['Ad'], (BK, 1), d['Bd'], (BN, 1), 0.0, C, (BN, 1), BB, (0, BK * BN, BM * BN))
    assert pc.tiles() == {0: 1} and pc.calls[SPLITK] == 0, pc.calls
    assert np.array_equal(host(C), d['AB'])


def test_big_tile_batched_beta_epilogue(L, plan_defaults, batched_int):
    """alpha, beta != 0 on the big tile: the old values of C arrive through the two-slab prefetch cv[2] of the epilogue, which only
    the tiles with more than two 16-row slabs per wave (TM = 4 here) walk with both buffers."""
    d = batched_int
    C = dev(d['C0'])
    with Counters(L) as pc:
        gemm(L, BM, BN, BK, -2.0, d['Ad'], (BK, 1), d['Bd'], (BN, 1), 3.0, C, (BN, 1), BB, (0, BK * BN, BM * BN))
    assert pc.tiles() == {0: 1} and pc.calls[SPLITK] == 0, pc.calls
    assert np.array_equal(host(C), -2.0 * d['AB'] + 3.0 * d['C0'])


def test_big_tile_rounding_against_float64(L, plan_defaults):
    """Random-normal operands through the same launch: 8 sampled items against float64 numpy, twice the bound of the product (the
    reference carries the same bound itself)."""
    rng = np.random.default_rng(131)
    A, B = rng.standard_normal((BM, BK)), rng.standard_normal((BB, BK, BN))
    C = nan_tensor(BB, BM, BN)
    with Counters(L) as pc:
        gemm(L, BM, BN, BK, 1.0, dev(A), (BK, 1), dev(B), (BN, 1), 0.0, C, (BN, 1), BB, (0, BK * BN, BM * BN))
    assert pc.tiles() == {0: 1}, pc.calls
    items = [0, 1, 255, 256, 444, 511, 888, 889]
    got = host(C[items])
    assert not bool(torch.isnan(C).any())
    within('big tile vs float64 numpy', got, np.matmul(A, B[items]), np.matmul(np.abs(A), np.abs(B[items])), 2 * sr.gamma(BK))


@pytest.mark.parametrize('K', (17, 31, 33))
def test_big_tile_k_tails(L, plan_defaults, K):
    """K % 16 = 1, 15, 1 (one, two and three K steps of the big tile, the last one partial), A per item and B shared."""
    batch = -(-64000 // K)
    assert BM * BN * K * batch >= 2 ** 30 and L.tn_gemm_ws_bytes(BM, BN, K, batch) == 0
    rng = np.random.default_rng(K)
    A, B = ints(rng, batch, BM, K), ints(rng, K, BN)
    C = nan_tensor(batch, BM, BN)
    with Counters(L) as pc:
        gemm(L, BM, BN, K, 1.0, dev(A), (K, 1), dev(B), (BN, 1), 0.0, C, (BN, 1), batch, (BM * K, 0, BM * BN))
    assert pc.tiles() == {0: 1} and pc.calls[SPLITK] == 0, pc.calls
    assert np.array_equal(host(C), (A.reshape(batch * BM, K) @ B).reshape(batch, BM, BN))


def test_big_tile_single_matrix_no_split(L, ops, plan_defaults):
    """14 x 14 = 196 tiles: at least 192 workgroups, so the large product is not split."""
    M = N = 1792
    K = 336
    assert M * N * K >= 2 ** 30 and L.tn_gemm_ws_bytes(M, N, K, 1) == 0
    rng = np.random.default_rng(1792)
    A, B = ints(rng, M, K), ints(rng, K, N)
    C = nan_tensor(M, N)
    with Counters(L) as pc:
        ops.mm(dev(A), dev(B), out=C)
    assert pc.tiles() == {0: 1} and pc.calls[SPLITK] == 0, pc.calls
    assert np.array_equal(host(C), A @ B)


# ------------------------------------------------------------------------------------------------ the split of the large products
SM, SN, SK = 200, 136, 40000          # 2 x 2 big tiles < 192 workgroups, K >= 512: 64 splits planned, chunks of 640 -> 63 used


@pytest.fixture(scope='module')
def split_int():
    rng = np.random.default_rng(200)
    A, B, C0 = ints(rng, SM, SK), ints(rng, SK, SN), ints(rng, SM, SN)
    return dict(A=A, B=B, C0=C0, AB=A @ B, Ad=dev(A), Bd=dev(B))


def test_big_tile_split(L, plan_defaults, split_int):
    d = split_int
    assert SM * SN * SK >= 2 ** 30
    ws, wsb = workspace(L, SM, SN, SK, 1)
    assert wsb == 64 * SM * SN * 8
    C = nan_tensor(SM, SN)
    with Counters(L) as pc:
        gemm(L, SM, SN, SK, 1.0, d['Ad'], (SK, 1), d['Bd'], (SN, 1), 0.0, C, (SN, 1), ws=ws, wsb=wsb)
    assert pc.tiles() == {0: 1} and pc.splits(SM, SN) == 63, (pc.calls, pc.flops)
    assert np.array_equal(host(C), d['AB'])


def test_big_tile_split_beta(L, plan_defaults, split_int):
    d = split_int
    ws, wsb = workspace(L, SM, SN, SK, 1)
    C = dev(d['C0'])
    with Counters(L) as pc:
        gemm(L, SM, SN, SK, -2.0, d['Ad'], (SK, 1), d['Bd'], (SN, 1), 3.0, C, (SN, 1), ws=ws, wsb=wsb)
    assert pc.tiles() == {0: 1} and pc.splits(SM, SN) == 63, (pc.calls, pc.flops)
    assert np.array_equal(host(C), -2.0 * d['AB'] + 3.0 * d['C0'])


def test_big_tile_split_short_workspace(L, plan_defaults, split_int):
    """Half the queried workspace: as many splits as fit (32), nothing written past it, the same integers."""
    d = split_int
    wsb = int(L.tn_gemm_ws_bytes(SM, SN, SK, 1)) // 2
    guard = 4096
    buf = torch.full((wsb + guard,), 0xA5, dtype=torch.uint8, device='cuda')
    C = nan_tensor(SM, SN)
    with Counters(L) as pc:
        gemm(L, SM, SN, SK, 1.0, d['Ad'], (SK, 1), d['Bd'], (SN, 1), 0.0, C, (SN, 1), ws=buf, wsb=wsb)
    assert pc.tiles() == {0: 1} and pc.splits(SM, SN) == 32, (pc.calls, pc.flops)
    assert bool((buf[wsb:] == 0xA5).all())
    assert np.array_equal(host(C), d['AB'])


# ------------------------------------------------------------------------------------------------ column-major C: C^T = B^T A^T
ALPHA, BETA = -0.5, 2.0


def _operand(X, transposed):
    """The matrix X on the device, row-major or as the transposed view of a row-major buffer holding X^T."""
    return dev(X.T).t() if transposed else dev(X)


def _axpby_ref(A, B, C0):
    A, B, C0 = (np.asarray(x, dtype=LD) for x in (A, B, C0))
    return ALPHA * (A @ B) + BETA * C0, abs(ALPHA) * (np.abs(A) @ np.abs(B)) + abs(BETA) * np.abs(C0)


@pytest.mark.parametrize('ta', (False, True))
@pytest.mark.parametrize('tb', (False, True))
def test_column_major_out(ops, plan_defaults, ta, tb):
    M, N, K = 130, 70, 33
    rng = np.random.default_rng(10 + 2 * ta + tb)
    A, B, C0 = rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))
    buf = dev(C0.T)                                                      # (N, M) row-major
    out = buf.t()
    assert out.stride() == (1, M)
    ops.mm(_operand(A, ta), _operand(B, tb), out=out, alpha=ALPHA, beta=BETA)
    ref, absref = _axpby_ref(A, B, C0)
    within('column-major C (swap)', host(buf).T, ref, absref, sr.gamma(K, 1))


def test_column_major_out_strided(ops, plan_defaults):
    """C is every second row of a (2N, M) buffer, transposed: unit row stride, column stride 2M.  The rows between stay untouched."""
    M, N, K = 130, 70, 33
    rng = np.random.default_rng(14)
    A, B, big = rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((2 * N, M))
    buf = dev(big)
    out = buf[::2].t()
    assert out.stride() == (1, 2 * M) and tuple(out.shape) == (M, N)
    ops.mm(dev(A), dev(B), out=out, alpha=ALPHA, beta=BETA)
    got = host(buf)
    assert np.array_equal(got[1::2], big[1::2])
    ref, absref = _axpby_ref(A, B, big[::2].T)
    within('column-major C (swap)', got[::2].T, ref, absref, sr.gamma(K, 1))


def test_column_major_out_batched(L, plan_defaults):
    """Through the C-ABI: A shared by the items (bsa = 0), B per item; the transposed product swaps the two batch strides with
    the operands.  K is split (12 workgroups, K = 200: six chunks), so beta goes through splitk_reduce with the swapped strides."""
    M, N, K, batch = 70, 90, 200, 3
    rng = np.random.default_rng(15)
    A, B, C0 = rng.standard_normal((M, K)), rng.standard_normal((batch, K, N)), rng.standard_normal((batch, M, N))
    buf = dev(C0.transpose(0, 2, 1))                                     # (batch, N, M) row-major: item b is C_b^T
    ws, wsb = workspace(L, M, N, K, batch)
    assert wsb > 0
    with Counters(L) as pc:
        gemm(L, M, N, K, ALPHA, dev(A), (K, 1), dev(B), (N, 1), BETA, buf, (1, M), batch, (0, K * N, N * M), ws, wsb)
    assert pc.tiles() == {3: 1} and pc.calls[SPLITK] == 1, pc.calls
    ref, absref = _axpby_ref(A[None], B, C0)
    within('column-major C (swap)', host(buf).transpose(0, 2, 1), ref, absref, sr.gamma(K, 1))


# ------------------------------------------------------------------------------------------------ more than 65535 batch items
@pytest.mark.parametrize('shared_b', (False, True))
def test_grid_z_slicing(L, plan_defaults, shared_b):
    """70000 items run as slices of 65535 and 4465; the second slice starts at A + 65535 bsa, B + 65535 bsb, C + 65535 bsc."""
    M = N = K = 4
    batch = 70000
    rng = np.random.default_rng(16 + shared_b)
    A, B = ints(rng, batch, M, K), ints(rng, *((K, N) if shared_b else (batch, K, N)))
    C = nan_tensor(batch, M, N)
    with Counters(L) as pc:
        gemm(L, M, N, K, 1.0, dev(A), (K, 1), dev(B), (N, 1), 0.0, C, (N, 1), batch, (M * K, 0 if shared_b else K * N, M * N))
    assert pc.tiles() == {3: 2} and pc.calls[SPLITK] == 0, pc.calls
    got, ref = host(C), np.matmul(A, B)
    for item in (0, 65534, 65535, 65536, 69999):
        assert np.array_equal(got[item], ref[item]), item
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------------------------------------ beta through splitk_reduce
@pytest.mark.parametrize('M,N,K', [(64, 64, 64), (257, 129, 65)])
def test_beta_through_small_split(L, ops, plan_defaults, M, N, K):
    assert L.tn_gemm_ws_bytes(M, N, K, 1) == 2 * M * N * 8               # two chunks of K
    rng = np.random.default_rng(M + N + K)
    A, B, C0 = rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))
    C = dev(C0)
    with Counters(L) as pc:
        ops.mm(dev(A), dev(B), out=C, alpha=ALPHA, beta=BETA)
    assert pc.tiles() == {3: 1} and pc.splits(M, N) == 2, (pc.calls, pc.flops)
    ref, absref = _axpby_ref(A, B, C0)
    within('beta through the small split', host(C), ref, absref, sr.gamma(K, 1))


# ------------------------------------------------------------------------------------------------ edges of the arguments
@pytest.mark.parametrize('M,N,K', [(5, 7, 3), (64, 64, 64)])             # unsplit / split
def test_beta_zero_ignores_nan_in_c(ops, M, N, K):
    rng = np.random.default_rng(M)
    A, B = ints(rng, M, K), ints(rng, K, N)
    C = nan_tensor(M, N)
    ops.mm(dev(A), dev(B), out=C, alpha=1.0, beta=0.0)
    assert np.array_equal(host(C), A @ B)


@pytest.mark.parametrize('beta', (2.0, 0.0))
def test_k_zero(L, beta):
    """K = 0: C <- beta C exactly; with beta = 0 the old C (NaN here) is not read."""
    M, N = 37, 45
    rng = np.random.default_rng(37)
    C0 = rng.standard_normal((M, N))
    C = dev(C0) if beta != 0.0 else nan_tensor(M, N)
    dummy = torch.zeros(1, dtype=F64, device='cuda')
    assert L.tn_gemm_ws_bytes(M, N, 0, 1) == 0
    gemm(L, M, N, 0, 1.0, dummy, (0, 1), dummy, (N, 1), beta, C, (N, 1))
    assert np.array_equal(host(C), 2.0 * C0 if beta != 0.0 else np.zeros((M, N)))


def test_zero_strides(ops):
    """A = one row repeated (row stride 0), B = one column repeated (column stride 0), as expanded views."""
    M, N, K = 70, 50, 33
    rng = np.random.default_rng(70)
    x, y = rng.standard_normal(K), rng.standard_normal(K)
    A, B = dev(x).expand(M, K), dev(y)[:, None].expand(K, N)
    assert A.stride() == (0, 1) and B.stride() == (1, 0)
    got = host(ops.mm(A, B))
    xl, yl = np.asarray(x, dtype=LD), np.asarray(y, dtype=LD)
    within('zero strides', got, np.full((M, N), xl @ yl), np.full((M, N), np.abs(xl) @ np.abs(yl)), sr.gamma(K))
