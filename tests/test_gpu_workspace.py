"""Exact workspace and full-output contracts of the library's exports, called through the C-ABI directly.

include/tnpeps.h: the caller owns every workspace, sized by the *_ws_bytes queries.  The callers in the package hand out more than
they query (ops.workspace: 1.25 n + 4096 bytes), so a kernel that writes past its query, reads scratch before writing it, or leaves
part of an output unwritten passes every other test.  Here each call gets a workspace of exactly the queried size between two 4 KiB
guards (tests/guarded.py) and outputs framed the same way and pre-filled with NaN, and for every case:
  1. the guards of the workspace and of every output are intact;
  2. the results are bit-identical with the workspace filled with zeros, NaN and random bytes, and to the ops wrapper's (which
     runs with a slack workspace);
  3. no NaN survives in what the contract says is written;
  4. ws_bytes - 8 is rejected before any launch (tn_gemm instead accepts less and uses fewer splits: the result is still right).
The launches with in-kernel barriers keep their arrival counters in per-stream device state that the call clears itself
(cholqr_begin / cholqr_reset in csrc/cholqr.hip, the state blocks of csrc/smallqr.hip and csrc/small.hip), or, for a stream
beyond the state slots, in a head of the workspace that cholqr_begin clears with a memset before the first launch: nothing a
kernel spins on is taken from the poisoned bytes.  Every case also asserts that no such launch gave up (ops.fused_timeouts)."""
import ctypes as ct
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
from guarded import Guarded, same_bits  # noqa: E402

F64 = torch.float64
FILLS = (0x00, 0xFF, 'random')          # zeros, NaN (as float64), random bytes


@pytest.fixture(scope='module')
def L():
    from tnac4o_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def ops():
    from tnac4o_amd import ops as o
    return o


def _st():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(x, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _msg(L):
    buf = ct.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    return buf.value.decode()


def contract(L, ops, ws_bytes, outs, call, written=None, short=True, inout=()):
    """Run `call` with an exact workspace filled with zeros, NaN and random bytes, check points 1-4 of the module docstring, and
    return ({name: host array}, info) of the first run.  outs: {name: (dtype, shape)};  call(bufs, ws_ptr, ws_bytes) -> (rc, info)
    with bufs {name: Guarded};  written(name, array, info) -> the part of that output the contract writes (default: all of it);
    inout: outputs the call itself fills with its input first."""
    runs = []
    for i, fill in enumerate(FILLS):
        ws = Guarded(ws_bytes, fill, seed=i)
        bufs = {k: Guarded.of(dt, sh, 0xFF, seed=10 + j) for j, (k, (dt, sh)) in enumerate(outs.items())}
        ops.fused_timeouts()
        rc, info = call(bufs, ws.ptr, ws_bytes)
        torch.cuda.synchronize()
        assert rc == 0, (fill, rc, _msg(L))
        assert ops.fused_timeouts() == 0, fill
        assert ws.intact(), ('workspace guard overwritten', fill)
        res = {}
        for k, b in bufs.items():
            assert b.intact(), ('output guard overwritten', k, fill)
            a = b.host()
            part = written(k, a, info) if written else a
            if a.dtype.kind == 'f':
                assert not np.isnan(part).any(), ('output element left unwritten', k, fill)
            res[k] = a
        runs.append((res, info))
    for res, info in runs[1:]:
        assert info == runs[0][1], 'result depends on the workspace contents'
        for k in res:
            assert same_bits(res[k], runs[0][0][k]), ('result depends on the workspace contents', k)
    if short:
        ws = Guarded(max(ws_bytes - 8, 0), 0x00)
        bufs = {k: Guarded.of(dt, sh, 0xFF) for k, (dt, sh) in outs.items()}
        rc, _ = call(bufs, ws.ptr, ws_bytes - 8)
        torch.cuda.synchronize()
        assert rc < 0 and 'too small' in _msg(L), (rc, _msg(L))
        assert ws.intact() and all(b.intact() and (k in inout or b.untouched(0xFF)) for k, b in bufs.items())
    return runs[0]


# ------------------------------------------------------------------------------------------------------------------ tn_gemm
GEMM_SHAPES = [(1, 1, 1), (5, 7, 3), (64, 64, 64), (130, 70, 33), (257, 129, 65), (16, 300, 1024), (300, 16, 2048),
               (32, 1000, 4100), (1024, 24, 40), (200, 200, 1), (128, 128, 16)]          # (those of test_gpu_kernels.py)


@pytest.mark.parametrize('M,N,K', GEMM_SHAPES)
@pytest.mark.parametrize('batch', (1, 3))
def test_gemm_workspace(L, ops, M, N, K, batch):
    rng = np.random.default_rng(M + 3 * N + 7 * K + batch)
    A, B = rng.standard_normal((batch, M, K)), rng.standard_normal((batch, K, N))
    Ad, Bd = dev(A), dev(B)
    wsb = int(L.tn_gemm_ws_bytes(M, N, K, batch))

    def call(b, ws, wsb_):
        return L.tn_gemm(M, N, K, 1.0, Ad.data_ptr(), K, 1, Bd.data_ptr(), N, 1, 0.0, b['C'].ptr, N, 1, batch, M * K, K * N, M * N,
                         ws if wsb_ > 0 else None, max(wsb_, 0), _st()), None
    res, _ = contract(L, ops, wsb, {'C': (F64, (batch, M, N))}, call, short=False)
    ref = A @ B
    tol = 1e-13 * max(1.0, K ** 0.5) * max(1.0, np.abs(ref).max())
    assert np.abs(res['C'] - ref).max() <= tol
    if batch == 1:
        assert same_bits(res['C'][0], host(ops.mm(Ad[0], Bd[0])))
    if wsb > 0:                        # less than the query: accepted with fewer splits, still right, nothing written outside
        ws, Cg = Guarded(wsb - 8), Guarded.of(F64, (batch, M, N))
        rc, _ = call({'C': Cg}, ws.ptr, wsb - 8)
        torch.cuda.synchronize()
        assert rc == 0, _msg(L)
        assert ws.intact() and Cg.intact()
        assert np.abs(Cg.host() - ref).max() <= tol


# ------------------------------------------------------------------------------------------------------------------ tn_qr
QR_CASES = [  # m, n, nb, rank_tol, TN_QR_NBO, rank of the input (None: full)
    (1, 1, 32, 0.0, '0', None), (31, 1, 32, 0.0, '0', None), (33, 65, 32, 0.0, '0', None), (65, 63, 64, 0.0, '0', None),
    (257, 255, 32, 0.0, '0', None), (300, 257, 64, 0.0, '0', None), (1000, 300, 32, 1e-10, '0', 40), (1000, 300, 64, 1e-10, '0', 40),
    (2048, 512, 32, 0.0, '128', None), (2048, 512, 32, 0.0, '256', None), (16384, 1024, 32, 0.0, '256', None)]


@pytest.mark.parametrize('m,n,nb,rank_tol,nbo,rank', QR_CASES)
def test_qr_workspace(L, ops, m, n, nb, rank_tol, nbo, rank):
    rng = np.random.default_rng(3 * m + n + nb)
    A = rng.standard_normal((m, n)) if rank is None else rng.standard_normal((m, rank)) @ rng.standard_normal((rank, n))
    Ad = dev(A)
    k = min(m, n)
    wsb = int(L.tn_qr_ws_bytes(m, n, nb))

    def call(b, ws, wsb_):
        T = Ad.clone()                                           # (consumed)
        keff = ct.c_int64(k)
        rc = L.tn_qr(T.data_ptr(), n, 1, m, n, b['Q'].ptr, k, 1, b['R'].ptr, n, 1, nb, rank_tol, ct.byref(keff), ws, wsb_, _st())
        return rc, int(keff.value)

    def written(name, a, keff):
        return a[:, :keff] if name == 'Q' else a[:keff]
    saved = os.environ.get('TN_QR_NBO')
    os.environ['TN_QR_NBO'] = nbo                                # (read per call)
    try:
        res, keff = contract(L, ops, wsb, {'Q': (F64, (m, k)), 'R': (F64, (k, n))}, call, written)
        Q = torch.empty((m, k), dtype=F64, device='cuda')
        R = torch.empty((k, n), dtype=F64, device='cuda')
        _, _, keff2 = ops.qr_into(Ad, Q, R, nb=nb, rank_tol=rank_tol)
    finally:
        if saved is None:
            os.environ.pop('TN_QR_NBO', None)
        else:
            os.environ['TN_QR_NBO'] = saved
    assert keff2 == keff
    assert same_bits(host(Q)[:, :keff], res['Q'][:, :keff]) and same_bits(host(R)[:keff], res['R'][:keff])
    assert (keff < k) == (rank is not None and nb == 32)        # (the early exit is a feature of the nb = 32 path)
    assert np.abs(res['Q'][:, :keff] @ res['R'][:keff] - A).max() <= 1e-12 * np.abs(A).max() * max(1.0, n ** 0.5)


# ------------------------------------------------------------------------------------------------------------------ tn_panel_orth
@pytest.mark.parametrize('nrows,b', [(1, 1), (33, 32), (65, 7), (1000, 32), (4097, 31)])
@pytest.mark.parametrize('method', (0,))
def test_panel_orth_workspace(L, ops, nrows, b, method):
    X = np.random.default_rng(nrows + b + method).standard_normal((nrows, b))
    Xd = dev(X)
    wsb = int(L.tn_panel_orth_ws_bytes(nrows, b))

    def call(bf, ws, wsb_):
        return L.tn_panel_orth(Xd.data_ptr(), b, 1, nrows, b, bf['Y'].ptr, b, 1, method, None, None, ws, wsb_, _st()), None
    res, _ = contract(L, ops, wsb, {'Y': (F64, (nrows, b))}, call)
    assert same_bits(res['Y'], host(ops.panel_orth(Xd, method)))


# ------------------------------------------------------------------------------------------------------------------ tn_svd_trunc / tn_svdvals
SVD_SHAPES = [(1, 1), (1, 7), (7, 1), (40, 40), (33, 65), (65, 33), (64, 64), (31, 100), (257, 63)]


@pytest.mark.parametrize('k,n', SVD_SHAPES)
def test_svd_trunc_workspace(L, ops, k, n):
    Cm = np.random.default_rng(k * 5 + n).standard_normal((k, n))
    Cd = dev(Cm)
    cap = min(k, n)
    wsb = int(L.tn_svd_ws_bytes(k, n, 1))

    def call(b, ws, wsb_):
        keep, disc, sw, info = ct.c_int64(0), ct.c_double(0.0), ct.c_int(0), ct.c_int(0)
        rc = L.tn_svd_trunc(Cd.data_ptr(), n, 1, k, n, cap, 0.0, b['U'].ptr, cap, 1, b['S'].ptr, b['Vt'].ptr, n, 1, ct.byref(keep),
                            ct.byref(disc), ct.byref(sw), ct.byref(info), ws, wsb_, _st())
        return rc, (int(keep.value), disc.value, sw.value, info.value)

    def written(name, a, info):
        return a[:, :info[0]] if name == 'U' else a[:info[0]]
    res, info = contract(L, ops, wsb, {'U': (F64, (k, cap)), 'S': (F64, (cap,)), 'Vt': (F64, (cap, n))}, call, written)
    assert info[3] == 0 and info[0] == cap
    U, S, Vt, kp, _, _ = ops._svd_trunc_raw(Cd, cap, 0.0)
    assert kp == info[0]
    assert same_bits(host(U), res['U'][:, :kp]) and same_bits(host(S), res['S'][:kp]) and same_bits(host(Vt), res['Vt'][:kp])


@pytest.mark.parametrize('k,n', SVD_SHAPES)
def test_svdvals_workspace(L, ops, k, n):
    Cm = np.random.default_rng(k * 7 + n).standard_normal((k, n))
    Cd = dev(Cm)
    cap = min(k, n)
    wsb = int(L.tn_svd_ws_bytes(k, n, 0))

    def call(b, ws, wsb_):
        S = (ct.c_double * cap)()
        sw, info = ct.c_int(0), ct.c_int(0)
        rc = L.tn_svdvals(Cd.data_ptr(), n, 1, k, n, S, ct.byref(sw), ct.byref(info), ws, wsb_, _st())
        return rc, (tuple(S), sw.value, info.value)
    _, info = contract(L, ops, wsb, {}, call)
    assert info[2] == 0
    assert same_bits(np.array(info[0]), ops.svdvals(Cd))
    assert np.abs(np.array(info[0]) - np.linalg.svd(Cm, compute_uv=False)).max() <= 1e-13 * max(k, n) * np.linalg.norm(Cm, 2)


# ------------------------------------------------------------------------------------------------------------------ tn_site_qr
SITE_CASES = [  # side, Dl, p, Dr, kc (None: no attach), rank_tol, frobenius_exit, pivot, rank of the site (None: full)
    (0, 1, 2, 1, None, 0.0, 0, 0, None), (0, 20, 4, 33, None, 0.0, 0, 0, None), (1, 33, 4, 20, None, 0.0, 0, 0, None),
    (0, 16, 2, 65, 15, 0.0, 0, 0, None), (1, 65, 2, 16, 17, 0.0, 0, 0, None), (0, 64, 4, 257, None, 1e-10, 0, 0, 24),
    (1, 257, 4, 64, None, 1e-10, 1, 0, 24), (0, 64, 4, 257, 63, 1e-10, 1, 0, 24), (0, 64, 4, 257, None, 1e-10, 0, 1, 24),
    (1, 257, 4, 64, 65, 1e-10, 0, 1, 24)]


@pytest.mark.parametrize('side,Dl,p,Dr,kc,rank_tol,frob,pivot,rank', SITE_CASES)
def test_site_qr_workspace(L, ops, side, Dl, p, Dr, kc, rank_tol, frob, pivot, rank):
    """The query takes neither rank_tol nor pivot: every variant must fit in it."""
    rng = np.random.default_rng(Dl + 3 * Dr + 5 * side + pivot)
    if rank is None:
        A = rng.standard_normal((Dl, p, Dr))
    elif side == 0:
        A = (rng.standard_normal((Dl * p, rank)) @ rng.standard_normal((rank, Dr))).reshape(Dl, p, Dr)
    else:
        A = (rng.standard_normal((Dl, rank)) @ rng.standard_normal((rank, p * Dr))).reshape(Dl, p, Dr)
    attach = kc is not None
    Ad = dev(A)
    Cd = dev(rng.standard_normal((kc, Dl) if side == 0 else (Dr, kc))) if attach else None
    m, n = ((kc if attach else Dl) * p, Dr) if side == 0 else (p * (kc if attach else Dr), Dl)
    kf = min(m, n)
    wsb = int(L.tn_site_qr_ws_bytes(side, Dl, p, Dr, kc or 0, 1 if attach else 0))

    def call(b, ws, wsb_):
        T = Ad.clone()                                           # (consumed without an attach)
        keff, normd, drop2 = ct.c_int64(kf), ct.c_int(0), ct.c_double(0.0)
        piv = (ct.c_int64 * n)() if pivot else None
        rc = L.tn_site_qr(side, T.data_ptr(), Dl, p, Dr, Cd.data_ptr() if attach else None, kc or 0, b['Q'].ptr, b['R'].ptr, rank_tol,
                          ct.byref(keff), b['nf'].ptr, ct.byref(normd), ct.byref(drop2), frob, piv, ws, wsb_, _st())
        return rc, (int(keff.value), int(normd.value), drop2.value, tuple(piv) if pivot else None)

    def written(name, a, info):
        k = info[0]
        if name == 'nf':
            return a if info[1] else a[:0]
        if name == 'Q':
            return a[:, :k] if side == 0 else a[:k]
        return a[:k] if side == 0 else a[:, :k]
    outs = {'Q': (F64, (m, kf) if side == 0 else (kf, m)), 'R': (F64, (kf, n) if side == 0 else (n, kf)), 'nf': (F64, (2,))}
    res, info = contract(L, ops, wsb, outs, call, written)
    k = info[0]
    if rank is not None:
        assert k < kf
    Q, R, k2, nf = ops.site_qr(side, Ad.clone(), Cd, rank_tol, True, None, bool(frob), bool(pivot))
    assert k2 == k
    assert same_bits(host(Q), written('Q', res['Q'], info))
    if info[1]:
        assert same_bits(host(R), written('R', res['R'], info)) and same_bits(host(nf), res['nf'])


# ------------------------------------------------------------------------------------------------------------------ site steps
@pytest.mark.parametrize('c,a,s,a2,c2', [(1, 1, 1, 1, 1), (33, 31, 4, 65, 63), (64, 64, 2, 64, 64), (257, 255, 2, 33, 1),
                                         (16, 256, 4, 256, 16)])
def test_rar_workspace(L, ops, c, a, s, a2, c2):
    rng = np.random.default_rng(c + a + s + a2 + c2)
    RL, A, RR = dev(rng.standard_normal((c, a))), dev(rng.standard_normal((a, s, a2))), dev(rng.standard_normal((a2, c2)))
    wsb = int(L.tn_rar_ws_bytes(c, a, s, a2, c2))

    def call(b, ws, wsb_):
        return L.tn_rar(RL.data_ptr(), A.data_ptr(), RR.data_ptr(), c, a, s, a2, c2, b['out'].ptr, ws, wsb_, _st()), None
    res, _ = contract(L, ops, wsb, {'out': (F64, (c, s, c2))}, call)
    assert same_bits(res['out'], host(ops.rar(RL, A, RR)))


@pytest.mark.parametrize('side', (0, 1))
@pytest.mark.parametrize('a,s,a2,c,c2', [(1, 1, 1, 1, 1), (33, 4, 31, 65, 63), (64, 2, 64, 64, 64), (255, 2, 257, 32, 1)])
def test_env_mix_workspace(L, ops, side, a, s, a2, c, c2):
    rng = np.random.default_rng(a + s + a2 + c + c2 + side)
    Rm = dev(rng.standard_normal((c, a) if side == 0 else (a2, c2)))
    A, Ac = dev(rng.standard_normal((a, s, a2))), dev(rng.standard_normal((c, s, c2)))
    wsb = int(L.tn_env_mix_ws_bytes(side, a, s, a2, c, c2))

    def call(b, ws, wsb_):
        return L.tn_env_mix(side, Rm.data_ptr(), A.data_ptr(), Ac.data_ptr(), a, s, a2, c, c2, b['out'].ptr, ws, wsb_, _st()), None
    res, _ = contract(L, ops, wsb, {'out': (F64, (c2, a2) if side == 0 else (a, c))}, call)
    assert same_bits(res['out'], host(ops.env_mix(side, Rm, A, Ac)))


@pytest.mark.parametrize('Dl,p,k0,keep,k1,p2,Dr', [(1, 1, 1, 1, 1, 1, 1), (16, 4, 33, 31, 65, 2, 63), (64, 2, 64, 64, 64, 2, 64),
                                                  (257, 1, 255, 1, 256, 4, 1)])
def test_apply_truncation_workspace(L, ops, Dl, p, k0, keep, k1, p2, Dr):
    rng = np.random.default_rng(Dl + k0 + keep + k1 + Dr)
    Al, Ar = dev(rng.standard_normal((Dl, p, k0))), dev(rng.standard_normal((k1, p2, Dr)))
    U = dev(rng.standard_normal((k0, keep + 3)))[:, :keep]       # strided views, as the SVD's outputs are sliced
    Vt = dev(rng.standard_normal((keep + 2, k1)))[:keep]
    S = dev(-np.sort(-rng.random(keep)))
    ml, nr = Dl * p, p2 * Dr
    wsb = int(L.tn_apply_truncation_ws_bytes(ml, k0, keep, k1, nr))

    def call(b, ws, wsb_):
        return L.tn_apply_truncation(Al.data_ptr(), ml, k0, U.data_ptr(), U.stride(0), U.stride(1), keep, Vt.data_ptr(), Vt.stride(0),
                                     Vt.stride(1), Ar.data_ptr(), k1, nr, S.data_ptr(), b['Al'].ptr, b['Ar'].ptr, b['Cd'].ptr, ws, wsb_,
                                     _st()), None
    res, _ = contract(L, ops, wsb, {'Al': (F64, (ml, keep)), 'Ar': (F64, (keep, nr)), 'Cd': (F64, (keep, keep))}, call)
    Aln, Arn, Cdg = ops.apply_truncation(Al, U, S, Vt, Ar)
    assert same_bits(res['Al'], host(Aln).reshape(ml, keep)) and same_bits(res['Ar'], host(Arn).reshape(keep, nr))
    assert same_bits(res['Cd'], host(Cdg))


# ------------------------------------------------------------------------------------------------------------------ thermal marginals
ENV3_DIMS = [(1, 1, 1, 1, 1, 1, 1, 1), (4, 2, 4, 2, 2, 2, 4, 4), (33, 4, 31, 4, 4, 4, 17, 65), (64, 2, 65, 2, 2, 2, 63, 64)]


@pytest.mark.parametrize('dims', ENV3_DIMS)
@pytest.mark.parametrize('side', (0, 1))
@pytest.mark.parametrize('half', (False, True))
def test_env3_workspace(L, ops, dims, side, half):
    Dt, pd, Dt2, bl, br, pu, Db, Db2 = dims
    rng = np.random.default_rng(sum(dims) + side + 2 * half)
    E = dev(rng.random((bl, Dt, Db) if side == 0 else (br, Dt2, Db2)))
    At, W, Ab = dev(rng.random((Dt, pd, Dt2))), dev(rng.random((bl, pd, br, pu))), dev(rng.random((Db, pu, Db2)))
    wsb = int(L.tn_env3_ws_bytes(side, *dims))
    outs = {'out': (F64, (br, Dt2, Db2) if side == 0 else (bl, Dt, Db)), 'lg': (F64, (1,))}
    if half:
        outs['half'] = (F64, (bl, pd, Dt2, Db) if side == 0 else (pu, br, Dt2, Db))

    def call(b, ws, wsb_):
        return L.tn_env3(side, E.data_ptr(), At.data_ptr(), W.data_ptr(), Ab.data_ptr(), *dims, None, b['out'].ptr, b['lg'].ptr,
                         b['half'].ptr if half else None, ws, wsb_, _st()), None
    res, _ = contract(L, ops, wsb, outs, call)
    ref = ops.env3(side, E, At, W, Ab, keep_half=half)
    assert same_bits(res['out'], host(ref[0])) and same_bits(res['lg'], host(ref[1]))
    if half:
        assert same_bits(res['half'], host(ref[2]))


CM_SHAPES = [  # q, bl, pd, br, pu, Dt2, Db
    (256, 16, 16, 16, 16, 8, 9),        # a chimera cell: 8 spins, 4 of them on each boundary
    (8, 8, 8, 8, 8, 33, 31),            # an RMF cell of d = 8
    (1, 1, 1, 1, 1, 1, 1)]


def _cell(q, bl, pd, br, pu, Dt2, Db, rng):
    HL, HR = dev(rng.random((bl, pd, Dt2, Db))), dev(rng.random((pu, br, Dt2, Db)))
    F = dev(rng.random((q, bl, pu)))
    dm = dev(rng.integers(0, pd, q), torch.int32)
    rm = dev(rng.integers(0, br, q), torch.int32)
    return HL, HR, F, dm, rm


@pytest.mark.parametrize('shape', CM_SHAPES)
def test_cluster_marginal_workspace(L, ops, shape):
    q, bl, pd, br, pu, Dt2, Db = shape
    HL, HR, F, dm, rm = _cell(*shape, np.random.default_rng(q + Dt2))
    K = Dt2 * Db
    wsb = int(L.tn_cluster_marginal_ws_bytes(bl, pd, br, pu, K))

    def call(b, ws, wsb_):
        return L.tn_cluster_marginal(HL.data_ptr(), HR.data_ptr(), F.data_ptr(), dm.data_ptr(), rm.data_ptr(), q, bl, pd, br, pu, K, None,
                                     None, b['P'].ptr, b['mP'].ptr, b['lz'].ptr, ws, wsb_, _st()), None
    res, _ = contract(L, ops, wsb, {'P': (F64, (q,)), 'mP': (F64, (1,)), 'lz': (F64, (1,))}, call)
    ref = ops.cluster_marginal(HL, HR, F, dm, rm)
    for k, t in zip(('P', 'mP', 'lz'), ref):
        assert same_bits(res[k], host(t)), k


@pytest.mark.parametrize('shape', CM_SHAPES)
def test_cluster_bond_marginal_workspace(L, ops, shape):
    q, bl, pd, br, pu, Dt2, Db = shape
    HL, HR, F, dm, rm = _cell(*shape, np.random.default_rng(q + Db + 1))
    K = Dt2 * Db
    wsb = int(L.tn_cluster_bond_marginal_ws_bytes(q, bl, pd, br, pu, K))

    def call(b, ws, wsb_):
        return L.tn_cluster_bond_marginal(HL.data_ptr(), HR.data_ptr(), F.data_ptr(), dm.data_ptr(), rm.data_ptr(), q, bl, pd, br, pu, K,
                                          None, None, b['Pl'].ptr, b['Pu'].ptr, b['mB'].ptr, b['lz'].ptr, ws, wsb_, _st()), None
    outs = {'Pl': (F64, (q, bl)), 'Pu': (F64, (q, pu)), 'mB': (F64, (1,)), 'lz': (F64, (1,))}
    res, _ = contract(L, ops, wsb, outs, call)
    ref = ops.cluster_bond_marginal(HL, HR, F, dm, rm)
    for k, t in zip(('Pl', 'Pu', 'mB', 'lz'), ref):
        assert same_bits(res[k], host(t)), k


# ------------------------------------------------------------------------------------------------------------------ small helpers
@pytest.mark.parametrize('n', (1, 1000, 70000, 2200000))
def test_normalize_pow2_scratch(L, ops, n):
    """The fixed 8 KiB scratch, exactly; it is all needed from 1024 x 2048 values on, where 8 bytes less is rejected."""
    x = np.random.default_rng(n).standard_normal(n) * 3e5
    xd = dev(x)

    def call(b, ws, wsb_):
        b['x'].tensor().copy_(xd)                                # (normalised in place)
        return L.tn_normalize_pow2(b['x'].ptr, n, b['o'].ptr, ws, wsb_, _st()), None
    res, _ = contract(L, ops, 8192, {'x': (F64, (n,)), 'o': (F64, (2,))}, call, short=n > 1024 * 2048, inout=('x',))
    y = xd.clone()
    o = ops.normalize_pow2_(y)
    assert same_bits(res['x'], host(y)) and same_bits(res['o'], host(o))


@pytest.mark.parametrize('side', (0, 1))
@pytest.mark.parametrize('k', (1, 2, 63, 64, 65, 256))
def test_bond_deflate_workspace(L, ops, side, k):
    """ws: k doubles."""
    rng = np.random.default_rng(k + side)
    n, m = 37, 70
    S = rng.integers(-3, 4, (k, n)).astype(np.float64)
    S[:, 0] = np.where(S[:, 0] == 0, 1.0, S[:, 0])
    S[1::4] *= 2.0 ** -60                                        # a quarter of the bond carries nothing
    Cm = S if side == 0 else np.ascontiguousarray(S.T)
    Q = rng.standard_normal((m, k) if side == 0 else (k, m))
    Cd, Qd = dev(Cm), dev(Q)

    def call(b, ws, wsb_):
        kk, d2 = ct.c_int64(-1), ct.c_double(-1.0)
        rc = L.tn_bond_deflate(side, Cd.data_ptr(), k, n, Qd.data_ptr(), m, b['C'].ptr, b['Q'].ptr, ct.byref(kk), ct.byref(d2), ws, wsb_,
                               _st())
        return rc, (int(kk.value), d2.value)

    def written(name, a, info):
        kk = info[0]
        return a.reshape(-1)[:(kk * n if name == 'C' else m * kk) if kk < k else 0]
    res, (kk, d2) = contract(L, ops, k * 8, {'C': (F64, Cm.shape), 'Q': (F64, Q.shape)}, call, written)
    assert kk == k - len(range(1, k, 4))
    if kk == k:                                                  # k = 1: nothing written
        assert np.all(res['C'].view(np.uint8) == 0xFF) and np.all(res['Q'].view(np.uint8) == 0xFF)
        return
    site = Qd.view(m, 1, k) if side == 0 else Qd.view(k, 1, m)
    Co, So, k2, d2o = ops.bond_deflate(side, Cd, site)
    assert (k2, d2o) == (kk, d2)
    assert same_bits(res['C'].reshape(-1)[:Co.numel()], host(Co).reshape(-1))
    assert same_bits(res['Q'].reshape(-1)[:So.numel()], host(So).reshape(-1))
