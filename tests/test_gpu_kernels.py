"""GPU parity tests of the individual C-ABI entry points (through tnac4o_amd.ops) against numpy / the oracle /
the golden vectors.  Integer-free path: tolerances are stated per test (fp64)."""
import os

import numpy as np
import pytest

import golden_inputs as gi
from oracle import mps_ref as mr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).cuda()


def host(t):
    return t.detach().cpu().numpy()


def load(name):
    return np.load(os.path.join(gi.GOLDEN_DIR, name))


@pytest.fixture(scope='module')
def ops():
    from tnac4o_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------ GEMM
GEMM_SHAPES = [(1, 1, 1), (5, 7, 3), (64, 64, 64), (130, 70, 33), (257, 129, 65), (16, 300, 1024), (300, 16, 2048),
               (32, 1000, 4100), (1024, 24, 40), (200, 200, 1), (128, 128, 16)]


@pytest.mark.parametrize('M,N,K', GEMM_SHAPES)
@pytest.mark.parametrize('ta,tb', [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gemm(ops, M, N, K, ta, tb):
    rng = np.random.default_rng(M * 7 + N * 3 + K + ta * 2 + tb)
    A = rng.standard_normal((K, M) if ta else (M, K))
    B = rng.standard_normal((N, K) if tb else (K, N))
    dA, dB = dev(A), dev(B)
    out = ops.mm(dA.t() if ta else dA, dB.t() if tb else dB)
    ref = (A.T if ta else A) @ (B.T if tb else B)
    assert np.abs(host(out) - ref).max() <= 1e-13 * max(1.0, K ** 0.5) * max(1.0, np.abs(ref).max())


def test_gemm_asymmetric_identity(ops):
    # A = I with an asymmetric B catches a transposed C write (cdna guide §3)
    B = np.arange(64 * 48, dtype=float).reshape(64, 48)
    out = ops.mm(dev(np.eye(64)), dev(B))
    assert np.array_equal(host(out), B)


def test_gemm_alpha_beta_strided_out(ops):
    rng = np.random.default_rng(3)
    A, B, C0 = rng.standard_normal((70, 50)), rng.standard_normal((50, 90)), rng.standard_normal((140, 100))
    C = dev(C0)
    view = C[::2, 5:95]                         # strided output view
    ops.mm(dev(A), dev(B), out=view, alpha=-0.5, beta=2.0)
    ref = C0.copy()
    ref[::2, 5:95] = -0.5 * (A @ B) + 2.0 * C0[::2, 5:95]
    assert np.abs(host(C) - ref).max() < 1e-12


def test_gemm_batched(ops):
    rng = np.random.default_rng(4)
    A, B = rng.standard_normal((1, 96, 40)), rng.standard_normal((37, 40, 18))
    out = ops.bmm(dev(A), dev(B))
    assert np.abs(host(out) - A @ B).max() < 1e-12
    A2 = rng.standard_normal((9, 33, 20))
    B2 = rng.standard_normal((9, 20, 70))
    assert np.abs(host(ops.bmm(dev(A2), dev(B2))) - A2 @ B2).max() < 1e-12


def test_gemm_wide_dynamic_range(ops):
    rng = np.random.default_rng(5)
    A = np.exp(-120 * rng.uniform(0, 1, (200, 300)))
    B = np.exp(-120 * rng.uniform(0, 1, (300, 150)))
    ref = A @ B
    assert np.abs(host(ops.mm(dev(A), dev(B))) / ref - 1).max() < 1e-12      # positive terms: relative accuracy


# ------------------------------------------------------------------------------------------------ absorb (G2)
def test_absorb_golden(ops):
    g = load('g2_absorb.npz')
    tags = sorted({k[:-2] for k in g.files if k.endswith('_A')})
    for tag in tags:
        hconj = bool(int(tag.split('_')[-1]))
        T = host(ops.absorb(dev(g[tag + '_A']), dev(g[tag + '_W']), hconj))
        assert tuple(T.shape) == tuple(g[tag + '_shape'])
        if tag + '_T' in g.files:
            np.testing.assert_allclose(T, g[tag + '_T'], rtol=0, atol=1e-14)
        else:
            np.testing.assert_allclose(T[::7, ::3, ::5], g[tag + '_Tsub'], rtol=0, atol=1e-13)
            np.testing.assert_allclose([T.sum(), np.abs(T).sum()], g[tag + '_Tsum'], rtol=1e-12)


@pytest.mark.parametrize('dims', [(1, 1, 1, 1, 1, 1, 1), (1, 16, 1, 1, 16, 16, 16), (5, 8, 3, 2, 8, 4, 6), (16, 16, 16, 16, 16, 16, 16),
                                  (64, 16, 64, 16, 16, 16, 16), (7, 4, 130, 1, 4, 16, 2),
                                  # edge sites of a sweep: any MPS bond (padded to 16-wide tiles in LDS by the matrix-core kernel)
                                  (13, 16, 23, 16, 16, 16, 16), (45, 16, 58, 16, 16, 16, 16), (60, 16, 1, 16, 16, 16, 16), (1, 16, 13, 1, 16, 16, 16),
                                  (23, 16, 112, 16, 16, 16, 16)])
@pytest.mark.parametrize('hconj', [True, False])
def test_absorb_vs_oracle(ops, dims, hconj):
    Dl, p, Dr, ba, po, bb, pi = dims
    rng = np.random.default_rng(sum(dims))
    if hconj:
        po = p
    else:
        pi = p
    A, W = rng.standard_normal((Dl, p, Dr)), rng.standard_normal((ba, po, bb, pi))
    got = host(ops.absorb(dev(A), dev(W), hconj))
    ref = mr.absorb_site(A, W, hconj)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() < 1e-13 * max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------------------------------------ nfactor (K6)
def test_nfactor_probe(ops):
    g = load('g1_linalg.npz')
    for x, y in zip(g['nfactor_probe_in'], g['nfactor_probe_out']):
        f = host(ops.nfactor_dev(dev(np.array([x, -x / 3, 0.0]))))
        assert f[0] == y and f[1] == 1.0 / y
    X = np.random.default_rng(0).standard_normal((100, 1000)) * 1e-40
    f = host(ops.nfactor_dev(dev(X)))
    assert f[0] == mr.pow2_floor_max(X)
    d = dev(X)
    f2 = host(ops.normalize_pow2_(d))
    assert np.array_equal(host(d), X / mr.pow2_floor_max(X))
    assert f2[0] == mr.pow2_floor_max(X) and f2[1] == 1.0 / f2[0]
    for shape in ((1, 1), (3, 5), (300, 7000), (4096, 1024)):          # one block ... the 1024-block cap of the two-launch form
        Z = np.random.default_rng(shape[0]).standard_normal(shape) * 10.0 ** np.random.default_rng(shape[1]).uniform(-30, 30)
        dz = dev(Z)
        fz = host(ops.normalize_pow2_(dz))
        assert fz[0] == mr.pow2_floor_max(Z) and np.array_equal(host(dz), Z / mr.pow2_floor_max(Z))
    Y = np.random.default_rng(1).standard_normal((5, 77))
    dY = dev(Y)
    ops.nfactor_batched_(dY)
    for b in range(5):
        assert np.array_equal(host(dY)[b], Y[b] / mr.pow2_floor_max(Y[b]))


# ------------------------------------------------------------------------------------------------ QR (K3, G1)
def check_qr(ops, T, nb=None, tol_orth=5e-14, tol_res=5e-14):
    m, n = T.shape
    k = min(m, n)
    Q, R = ops.qr(dev(T), nb=nb)
    Q, R = host(Q), host(R)
    assert Q.shape == (m, k) and R.shape == (k, n)
    cn = np.sqrt((T * T).sum(0))
    cn[cn == 0] = 1.0
    assert (np.abs(Q @ R - T) / cn).max() < tol_res, 'column-relative residual'
    assert np.abs(Q.T @ Q - np.eye(k)).max() < tol_orth, 'orthogonality'
    assert np.abs(np.tril(R[:, :k], -1)).max() == 0.0
    assert (np.diag(R) >= 0).all()
    return Q, R


@pytest.mark.parametrize('shape', gi.G1_SHAPES)
@pytest.mark.parametrize('kind', ['plain', 'rankdef', 'graded'])
def test_qr_golden(ops, shape, kind):
    g = load('g1_linalg.npz')
    T = gi.g1_matrix(shape, kind)
    Q, R = check_qr(ops, T)
    tag = '%dx%d_%s' % (shape[0], shape[1], kind)
    if kind != 'rankdef':          # R is unique (up to rounding amplified by the conditioning) only at full rank
        want = g[tag + '_absdiagR']
        tol = 1e-12 if kind == 'plain' else 1e-9
        np.testing.assert_allclose(np.diag(R), want, rtol=tol, atol=1e-14 * want.max())


@pytest.mark.parametrize('shape', [(1, 1), (1, 5), (5, 1), (31, 31), (33, 32), (64, 64), (65, 33), (100, 257), (2000, 96),
                                   (4096, 160)])
@pytest.mark.parametrize('nb', [32, 64])
def test_qr_shapes(ops, shape, nb):
    rng = np.random.default_rng(shape[0] * 13 + shape[1])
    check_qr(ops, rng.standard_normal(shape), nb=nb)


def test_qr_strided_views(ops):
    rng = np.random.default_rng(9)
    T = rng.standard_normal((300, 80))
    d = dev(T.T.copy()).t()                     # column-major view, like orth_right's
    k = 80
    Qt = torch.empty((k, 300), dtype=torch.float64, device='cuda')
    Rt = torch.empty((80, k), dtype=torch.float64, device='cuda')
    ops.qr_into(d, Qt.t(), Rt.t())
    Q, R = host(Qt).T, host(Rt).T
    assert np.abs(Q @ R - T).max() < 1e-13 and np.abs(Q.T @ Q - np.eye(k)).max() < 1e-13
    assert (np.diag(R) >= 0).all() and np.abs(np.tril(R, -1)).max() == 0


def test_qr_graded_and_dependent(ops):
    rng = np.random.default_rng(11)
    # columns spanning 60 orders of magnitude, rows graded too, exact zero columns and exact duplicates
    T = rng.standard_normal((700, 96)) * np.exp(-140 * rng.uniform(0, 1, (1, 96))) * np.exp(-60 * rng.uniform(0, 1, (700, 1)))
    T[:, 10] = 0.0
    T[:, 50] = T[:, 3]
    T[:, 70:80] = T[:, 20:30] @ rng.standard_normal((10, 10))
    check_qr(ops, T, tol_orth=1e-13, tol_res=1e-13)
    check_qr(ops, np.zeros((50, 40)))
    check_qr(ops, np.ones((90, 70)))


# ------------------------------------------------------------------------------------------------ SVD (K4/K5, G1)
def check_svd(ops, T, Dmax, tol, want_keep=None, want_disc=None, Sref=None, keep_slack=0):
    U, S, Vt, keep, disc, info = ops.svd_trunc(dev(T), Dmax, tol)
    U, S, Vt = host(U), host(S), host(Vt)
    assert info['info'] == 0
    if Sref is None:
        Sref = np.linalg.svd(T, compute_uv=False)
    assert U.shape == (T.shape[0], keep) and Vt.shape == (keep, T.shape[1]) and S.shape == (keep,)
    np.testing.assert_allclose(S, Sref[:keep], rtol=0, atol=1e-13 * Sref[0])
    assert np.abs(U.T @ U - np.eye(keep)).max() < 5e-13
    assert np.abs(Vt @ Vt.T - np.eye(keep)).max() < 5e-13
    # best rank-keep approximation
    Ur, Sr, Vr = np.linalg.svd(T, full_matrices=False)
    gap_ok = keep == len(Sref) or Sref[keep - 1] - Sref[keep] > 1e-8 * Sref[0]
    if gap_ok:
        assert np.abs((U * S) @ Vt - (Ur[:, :keep] * Sr[:keep]) @ Vr[:keep]).max() < 1e-12 * Sref[0]
    # sign gauge (mps.py:35-39) is a fixed point
    flip = (np.abs(U.min(0)) > U.max(0)) & (np.abs(Vt.min(1)) > Vt.max(1))
    assert not flip.any()
    if want_keep is not None:
        assert abs(keep - want_keep) <= keep_slack
    if want_disc is not None:
        assert disc == pytest.approx(want_disc, rel=1e-6, abs=1e-14)
    return keep, disc


@pytest.mark.parametrize('shape', gi.G1_SHAPES)
@pytest.mark.parametrize('kind', ['plain', 'rankdef', 'graded'])
def test_svd_golden(ops, shape, kind):
    g = load('g1_linalg.npz')
    T = gi.g1_matrix(shape, kind)
    tag = '%dx%d_%s' % (shape[0], shape[1], kind)
    for Dmax, tol in ((8, 1e-16), (10 ** 6, 1e-16), (10 ** 6, 1e-3)):
        want = g[tag + '_trunc_%d_%g' % (Dmax, tol)]
        pinned = kind != 'rankdef' or tol > 1e-10 or Dmax == 8         # eps-level rank decisions are noise
        # graded spectrum: sigma_k = 10^(-k/2) crosses eps*S0 between k=31 and k=32, where LAPACK's absolute error
        # (~eps*S0) decides; the Jacobi kernel resolves sigma_31 = 3.2e-16 > eps, so allow one vector of slack there
        # (the same knife edge exists at tol = 1e-3: sigma_6 = 1e-3 * S0 exactly, decided by the last bit)
        edge = kind == 'graded' and Dmax > 8
        check_svd(ops, T, min(Dmax, min(shape)), tol, int(want[0]) if pinned else None,
                  want[1] if pinned and not edge else None, Sref=g[tag + '_S'], keep_slack=1 if edge else 0)
    S = ops.svdvals(dev(T))
    np.testing.assert_allclose(S, g[tag + '_svdS'], rtol=0, atol=2e-14 * g[tag + '_S'][0])


@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (9, 1), (3, 3), (64, 64), (65, 65), (130, 70), (70, 130), (300, 300)])
def test_svd_shapes(ops, shape):
    rng = np.random.default_rng(shape[0] + 31 * shape[1])
    T = rng.standard_normal(shape)
    check_svd(ops, T, min(shape), 1e-16)
    check_svd(ops, T, max(1, min(shape) // 2), 1e-16)


def _svd_case(k, n, seed, decay=0.25):
    g = np.random.default_rng(seed)
    r = min(k, n)
    U, _ = np.linalg.qr(g.standard_normal((k, r)))
    V, _ = np.linalg.qr(g.standard_normal((n, r)))
    A = (U * np.exp(-decay * np.arange(r))) @ V.T
    return np.triu(A) if seed % 2 else A


@pytest.mark.parametrize('shape', [(128, 200), (192, 600), (192, 900), (100, 100), (65, 65), (64, 700), (130, 70), (256, 500), (70, 3000),
                                   (256, 700, 0.05), (230, 1024, 0.06), (256, 256, 0.04), (200, 260, 0.02)])
def test_svd_rounds_in_one_launch_bit_identical_to_separate_launches(ops, shape, monkeypatch):
    """All Jacobi rounds of a truncated SVD in ONE launch (svdl_kernel: the vectors resident in LDS, grid barriers between the
    phases) against three launches per round and a read-back per sweep (TN_SVD_FUSED=0): same arithmetic in the same order -- U, S,
    V^T, the kept rank, the discarded weight and the number of sweeps agree bit for bit.  (Shapes with more than 256 live vectors or
    more chunks than the co-residency budget holds stay on the separate launches in both runs.)  A third entry is the decay rate of the
    spectrum: the slow ones keep up to 256 vectors alive (the one-launch form's limit since round 5; 192 before)."""
    for seed in (1, 2):
        T = dev(_svd_case(shape[0], shape[1], seed, *shape[2:]))
        outs = []
        for mode in ('0', '1'):
            monkeypatch.setenv('TN_SVD_FUSED', mode)
            outs.append(ops.svd_trunc(T, 64, 1e-8))
        (U0, S0, V0, k0, d0, i0), (U1, S1, V1, k1, d1, i1) = outs
        assert k0 == k1 and d0 == d1 and i0['sweeps'] == i1['sweeps']
        assert torch.equal(U0, U1) and torch.equal(S0, S1) and torch.equal(V0, V1)
        Sr = np.linalg.svd(T.cpu().numpy(), compute_uv=False)
        np.testing.assert_allclose(S1.cpu().numpy(), Sr[:k1], rtol=0, atol=1e-14 * Sr[0])


SVD_TIMEOUT_CHILD = r'''
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import numpy as np, torch
from tnac4o_amd import ops
from test_gpu_kernels import _svd_case
ok = True
for (k, n) in ((128, 300), (192, 600)):
    T = torch.as_tensor(_svd_case(k, n, 1)).cuda()
    os.environ['TN_SVD_FUSED'] = '0'
    U0, S0, V0, k0, d0, i0 = ops.svd_trunc(T, 64, 1e-8)
    os.environ['TN_SVD_FUSED'] = '1'
    st = torch.cuda.Stream()              # a fresh stream per case: a stream that has given up stays off the single-launch forms
    with torch.cuda.stream(st):
        U1, S1, V1, k1, d1, i1 = ops.svd_trunc(T, 64, 1e-8)
    st.synchronize()
    ok &= bool(k0 == k1 and d0 == d1 and torch.equal(U0, U1) and torch.equal(S0, S1) and torch.equal(V0, V1))
    ok &= bool(torch.isfinite(U1).all() and torch.isfinite(S1).all() and torch.isfinite(V1).all())
print('CHILD_OK' if ok else 'CHILD_FAIL')
'''


def test_svd_one_launch_rounds_that_give_up_are_redone_as_separate_launches():
    """TN_PANEL_SPIN_LIMIT=0: every barrier of svdl_kernel gives up at once.  The launch reports it in its status word, tn_svd_trunc
    sets the vectors up again and runs the rounds as separate launches: the result is the one of TN_SVD_FUSED=0 bit for bit, the
    library says so on stderr, nothing non-finite comes back."""
    out = _run_child(SVD_TIMEOUT_CHILD, {'TN_PANEL_SPIN_LIMIT': '0'})
    assert 'CHILD_OK' in out, out
    assert out.count('[libtnpeps] the one-launch Jacobi rounds') == 2, out
    out = _run_child(SVD_TIMEOUT_CHILD, {})
    assert 'CHILD_OK' in out and '[libtnpeps]' not in out, out


def test_svd_one_launch_rounds_under_uneven_load(ops):
    """The grid barriers and hand-offs of svdl_kernel (partial Gram matrices, J, status) under uneven load: four chains run truncated
    SVDs of different shapes on four streams while a fifth keeps the device full of large GEMMs; every result equals the one obtained
    alone, bit for bit, and no launch gave up (no fallback message would change the bits, so the sweep counts are compared too)."""
    import threading
    mats = [dev(_svd_case(128, 300, 1)), dev(_svd_case(192, 600, 2)), dev(_svd_case(192, 900, 1)), dev(_svd_case(100, 1000, 2))]
    ref = [ops.svd_trunc(T, 64, 1e-8) for T in mats]
    torch.cuda.synchronize()
    g = torch.Generator(device='cpu').manual_seed(43)
    big_a = torch.randn(4096, 4096, dtype=torch.float64, generator=g).cuda()
    big_b = torch.randn(4096, 4096, dtype=torch.float64, generator=g).cuda()
    streams = [torch.cuda.Stream() for _ in range(5)]
    bad, err = [0] * 4, []
    stop = threading.Event()

    def chain(i):
        try:
            with torch.cuda.stream(streams[i]):
                for _ in range(12):
                    U, S, V, k, d, info = ops.svd_trunc(mats[i], 64, 1e-8)
                    same = (k == ref[i][3] and d == ref[i][4] and info['sweeps'] == ref[i][5]['sweeps'] and torch.equal(U, ref[i][0])
                            and torch.equal(S, ref[i][1]) and torch.equal(V, ref[i][2]))
                    if not same:
                        bad[i] += 1
                streams[i].synchronize()
        except BaseException as e:          # noqa: BLE001
            err.append(e)

    def load():
        with torch.cuda.stream(streams[4]):
            while not stop.is_set():
                ops.mm(big_a, big_b)
                streams[4].synchronize()
    th = [threading.Thread(target=chain, args=(i,)) for i in range(4)]
    tl = threading.Thread(target=load)
    tl.start()
    for t in th:
        t.start()
    for t in th:
        t.join()
    stop.set()
    tl.join()
    assert not err, err
    assert bad == [0, 0, 0, 0], bad


def test_svd_triangular_lowrank(ops):
    # the shape the sweep produces: an upper-triangular factor of a numerically low-rank matrix
    rng = np.random.default_rng(21)
    A = (rng.standard_normal((2000, 40)) * 10.0 ** (-np.arange(40) / 3.0)) @ rng.standard_normal((40, 300))
    R = np.linalg.qr(A)[1]
    keep, disc = check_svd(ops, R, 64, 1e-16)
    Sref = np.linalg.svd(R, compute_uv=False)
    assert keep == min(int((Sref > Sref[0] * 2.220446049250313e-16).sum()), 64)
    check_svd(ops, R.T.copy(), 64, 1e-16)


# ------------------------------------------------------------------------------------------------ K7 builder
@pytest.mark.parametrize('rot', [0, 1])
def test_peps_factor_and_mpo_builder(ops, rot):
    import tnac4o_amd
    s = tnac4o_amd.tnac4o(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 3), beta=3.0)
    if rot:
        s.rotate_graph(rot)
    rng = np.random.default_rng(rot)
    s.Xu, s.Xd = rng.uniform(0.5, 2, s.Xu.shape), rng.uniform(0.5, 2, s.Xd.shape)
    s.Xl, s.Xr = rng.uniform(0.5, 2, s.Xl.shape), rng.uniform(0.5, 2, s.Xr.shape)
    for ny in range(4):
        for nx in range(4):
            F, dmap, rmap, pd, br = s._peps_factor(ny, nx)                 # host twin
            Fd, dm, rm, pd2, br2 = s._peps_factor_dev(ny, nx)
            assert (pd, br) == (pd2, br2)
            assert np.array_equal(host(dm.double()), dmap) and np.array_equal(host(rm.double()), rmap)
            np.testing.assert_allclose(host(Fd), F, rtol=4e-16 * 8, atol=0)
            np.testing.assert_allclose(host(s._mpo_site_dev(ny, nx)), s._mpo_site(ny, nx), rtol=1e-14, atol=0)
        # the row form (all cells of a row through one packed copy) gives the per-cell results bit for bit
        row = s._row_mpo(ny)
        for nx in range(4):
            assert torch.equal(row.W[nx], s._mpo_site_dev(ny, nx))
    J = gi.minimal_rmf()
    r = tnac4o_amd.tnac4o(mode='RMF', Nx=J['Nx'], Ny=J['Ny'], J=J, beta=2.0)
    for ny in range(r.Ny):
        for nx in range(r.Nx):
            np.testing.assert_allclose(host(r._mpo_site_dev(ny, nx)), r._mpo_site(ny, nx), rtol=1e-14, atol=0)
        row = r._row_mpo(ny)
        for nx in range(r.Nx):
            assert torch.equal(row.W[nx], r._mpo_site_dev(ny, nx))


def test_linalg_fuzz_against_numpy():
    """Randomised shapes / structures (plain, graded, rank deficient, zero columns, 1e+-120 scaling, all ones; both memory
    layouts) through tn_qr, tn_svd_trunc and tn_svdvals: tools/fuzz_linalg.py with a fixed seed."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'fuzz_linalg.py'), '7', '60'], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ K9 environments, balancing
ENV_SHAPES = [(64, 16, 64, 16, 16, 16, 40), (128, 8, 128, 8, 8, 8, 33), (5, 3, 7, 2, 4, 3, 6), (1, 16, 16, 1, 16, 16, 3),
              (64, 16, 1, 16, 1, 16, 2)]


@pytest.mark.parametrize('Dl,p,Dr,bl,br,pu,nk', ENV_SHAPES)
def test_env_rr_batched(ops, Dl, p, Dr, bl, br, pu, nk):
    """tn_env_rr_batched against the reference's two tensordots + nfactor (tnac4o.py:1779-1781), key by key, incl. an
    all-zero parent environment and strongly graded data (the nfactor must be the exact power of two)."""
    rng = np.random.default_rng(Dl * 3 + p + nk)
    nprev = max(2, nk // 3)
    A = rng.standard_normal((Dl, p, Dr))
    RRp = rng.standard_normal((nprev, Dr, br)) * np.exp(-40 * rng.uniform(0, 1, (nprev, 1, 1)))
    RRp[1] = 0.0
    W = np.exp(-20 * rng.uniform(0, 1, (bl, p, br, pu)))
    parent = rng.integers(0, nprev, nk).astype(np.int32)
    parent[0] = 1
    uidx = rng.integers(0, pu, nk).astype(np.int32)
    out = host(ops.env_rr(dev(A), dev(RRp), dev(W), torch.as_tensor(parent).cuda(), torch.as_tensor(uidx).cuda()))
    assert out.shape == (nk, Dl, bl)
    for k in range(nk):
        T = np.tensordot(A, RRp[parent[k]], axes=(2, 0))
        ref = np.tensordot(T, W[:, :, :, uidx[k]], axes=([1, 2], [1, 2]))
        nf = mr.pow2_floor_max(ref)
        ref = ref * (1 / nf)
        assert np.abs(out[k] - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max())
        m = np.abs(out[k]).max()
        assert m == 0.0 or 1.0 <= m < 2.0                     # normalised by a power of two


def test_env_rl_batched(ops):
    rng = np.random.default_rng(11)
    npref, p, Dr, nk = 9, 16, 64, 50
    T1 = rng.standard_normal((npref, p, Dr)) * np.exp(-60 * rng.uniform(0, 1, (npref, p, 1)))
    T1[2, 3] = 0.0
    par = rng.integers(0, npref, nk).astype(np.int32)
    d = rng.integers(0, p, nk).astype(np.int32)
    par[0], d[0] = 2, 3
    out = host(ops.env_rl(dev(T1), torch.as_tensor(par).cuda(), torch.as_tensor(d).cuda()))
    for k in range(nk):
        row = T1[par[k], d[k]]
        assert np.array_equal(out[k], row * (1 / mr.pow2_floor_max(row)))      # power-of-two scaling: bit-exact


@pytest.mark.parametrize('kind', ['normal', 'wide', 'graded', 'sparse'])
def test_balance_bit_exact_vs_scipy(ops, kind):
    """tn_balance = LAPACK dgebal (job 'S') as called by the reference (scipy.linalg.matrix_balance(permute=False,
    separate=True), tnac4o.py:1845) followed by its clamp (:1847): the scale factors are powers of two, so the agreement
    must be bit-exact."""
    import scipy.linalg
    from oracle.gebal_ref import gebal_scale
    rng = np.random.default_rng({'normal': 1, 'wide': 2, 'graded': 3, 'sparse': 4}[kind])
    for t in range(40):
        n = int(rng.integers(1, 33)) if t else 16
        if kind == 'normal':
            A = rng.standard_normal((n, n))
        elif kind == 'wide':
            A = np.exp(rng.uniform(-40, 40, (n, n)))
        elif kind == 'graded':
            dd = np.exp(rng.uniform(-30, 30, n))
            A = np.abs(rng.standard_normal((n, n))) * dd[:, None] / dd[None, :]
        else:
            A = np.exp(rng.uniform(-20, 0, (n, n)))
            A[rng.random((n, n)) < 0.3] = 0
        _, sc = scipy.linalg.matrix_balance(A, permute=False, separate=True)
        assert np.array_equal(sc[0], gebal_scale(A)[0])
        got = host(ops.balance(dev(A)))
        assert np.array_equal(got, sc[0]), (kind, t, n)
        ms = 32.0
        got = host(ops.balance(dev(A).t().contiguous().t(), ms))               # strided view + clamp
        assert np.array_equal(got, np.minimum(np.maximum(sc[0], 1 / ms), ms))


def test_balance_on_preconditioner_environments():
    """The bond environments the 'balancing' preconditioner actually meets (droplet L=128 #1, the G7 pre=1 case): every
    tn_balance result equals scipy's on the same matrix."""
    import scipy.linalg
    import tnac4o_amd
    from tnac4o_amd import ops as o
    seen = []
    orig = o.balance

    def spy(env, max_scale=0.0):
        sc = orig(env, max_scale)
        seen.append((env.detach().cpu().numpy().copy(), max_scale, sc.detach().cpu().numpy().copy()))
        return sc
    o.balance = spy
    try:
        s = tnac4o_amd.tnac4o(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=3.0)
        s.precondition(mode='balancing')
    finally:
        o.balance = orig
    assert len(seen) == 2 * 3 * 4 * 2                         # 2 conditioning passes x 3 bonds rows x 4 columns x 2 directions
    for env, ms, sc in seen:
        _, ref = scipy.linalg.matrix_balance(env, permute=False, separate=True)
        assert np.array_equal(sc, np.minimum(np.maximum(ref[0], 1 / ms), ms))
    g = load('g4_peps.npz')
    np.testing.assert_allclose(s.Xu, g['L128_pre1_Xu'], rtol=1e-12)
    np.testing.assert_allclose(s.Xd, g['L128_pre1_Xd'], rtol=1e-12)
    np.testing.assert_allclose(s.overlaps_ud, g['L128_pre1_overlaps_ud'], rtol=1e-9)


@pytest.mark.parametrize('m,n,tol', [(16384, 1024, 0.0), (4096, 1024, 0.0), (4096, 1024, 1e-12), (16384, 512, 0.0)])
def test_qr_bit_identical_across_runs(ops, m, n, tol):
    """tn_qr run twice on the same graded low-rank input (so the early exit triggers when tol > 0): Q, R and the revealed rank
    must be bit-identical between the runs."""
    g = torch.Generator(device='cuda').manual_seed(m + n)
    r = 300
    T = (torch.randn((m, r), dtype=torch.float64, device='cuda', generator=g)
         * torch.exp(-30.0 * torch.rand((1, r), dtype=torch.float64, device='cuda', generator=g))) \
        @ torch.randn((r, n), dtype=torch.float64, device='cuda', generator=g)
    k = min(m, n)
    res = []
    for _ in range(2):
        Q = torch.zeros((m, k), dtype=torch.float64, device='cuda')
        R = torch.zeros((k, n), dtype=torch.float64, device='cuda')
        _, _, keff = ops.qr_into(T.clone(), Q, R, overwrite=True, rank_tol=tol)
        torch.cuda.synchronize()
        res.append((Q, R, keff))
    (Q0, R0, keff0), (Q1, R1, keff1) = res
    assert keff1 == keff0
    assert torch.equal(Q1[:, :keff0], Q0[:, :keff0]) and torch.equal(R1[:keff0], R0[:keff0])
    if tol > 0:
        assert keff0 < k


def test_svd_general_ill_conditioned_uses_qr_preconditioning(ops):
    """A dense matrix with nearly parallel rows and condition 1e14 (not a triangular factor): the plain Jacobi run hits its
    sweep cap, ops.svd_trunc then preconditions with two QRs.  Values against LAPACK, orthogonality, reconstruction, the
    reference's sign gauge, and svdvals on the same input."""
    g = torch.Generator(device='cuda').manual_seed(5)
    n = 512
    U0, _ = torch.linalg.qr(torch.randn((n, n), dtype=torch.float64, device='cuda', generator=g))
    S0 = torch.logspace(0, -14, n, dtype=torch.float64, device='cuda')
    C = (U0 * S0) @ torch.randn((n, n), dtype=torch.float64, device='cuda', generator=g)
    U, S, Vt, keep, disc, info = ops.svd_trunc(C, n, 1e-17)
    Sref = torch.linalg.svdvals(C.cpu()).cuda()
    assert keep == int((Sref > Sref[0] * 2.220446049250313e-16).sum()) or abs(keep - n) <= 2
    assert float((S - Sref[:keep]).abs().max()) < 1e-13 * float(Sref[0])
    I = torch.eye(keep, dtype=torch.float64, device='cuda')
    assert float((ops.mm(U.t(), U) - I).abs().max()) < 1e-12 and float((ops.mm(Vt, Vt.t()) - I).abs().max()) < 1e-12
    assert float((ops.mm(U * S, Vt) - C).abs().max()) < 1e-12 * float(Sref[0])
    flip = (U.min(dim=0).values.abs() > U.max(dim=0).values) & (Vt.min(dim=1).values.abs() > Vt.max(dim=1).values)
    assert not bool(flip.any())                                   # gauge fixed point (mps.py:35-39)
    sv = ops.svdvals(C)
    assert np.abs(sv[:keep] - Sref[:keep].cpu().numpy()).max() < 1e-13 * float(Sref[0])


# ------------------------------------------------------------------------------------------------ strided batches
@pytest.mark.parametrize('hconj', [True, False])
def test_absorb_batched_matches_single_calls(ops, hconj):
    """tn_absorb with batch = 4 (the same site of the 4 rotations' boundary MPS) in one launch: bit-identical to 4 calls, for
    a per-item MPO site and for one shared MPO site (stride 0), on the MFMA bulk shape and on a ragged VALU shape."""
    for (Dl, p, Dr, ba, bb) in [(64, 16, 64, 16, 16), (5, 3, 7, 2, 3)]:
        g = torch.Generator(device='cuda').manual_seed(Dl + p)
        A = torch.randn((4, Dl, p, Dr), dtype=torch.float64, device='cuda', generator=g)
        for bw in (4, 1):
            W = torch.randn((bw, ba, p, bb, p), dtype=torch.float64, device='cuda', generator=g)
            out = ops.absorb_batched(A, W, hconj)
            for i in range(4):
                assert torch.equal(out[i], ops.absorb(A[i], W[i if bw > 1 else 0], hconj))


@pytest.mark.parametrize('m,n,nside', [(4096, 256, 4), (1024, 64, 2), (16384, 1024, 4), (300, 40, 0)])
def test_qr_batched_concurrent_items_bit_identical(ops, m, n, nside):
    """tn_qr_batched: 4 independent QRs whose kernel chains interleave on side streams (forked from and joined into the
    caller's stream inside the call, no host threads) give exactly the factors of 4 separate tn_qr calls."""
    g = torch.Generator(device='cuda').manual_seed(m + n)
    T = torch.randn((4, m, n), dtype=torch.float64, device='cuda', generator=g) * \
        torch.exp(-20.0 * torch.rand((4, 1, n), dtype=torch.float64, device='cuda', generator=g))
    ref = [ops.qr(T[i]) for i in range(4)]
    sides = [torch.cuda.Stream() for _ in range(nside)]
    Q, R, keff = ops.qr_batched(T.clone(), side_streams=sides)
    after = Q.sum() + R.sum()                      # consumer on the caller's stream: must see the joined results
    torch.cuda.synchronize()
    assert keff == [min(m, n)] * 4 and bool(torch.isfinite(after))
    for i in range(4):
        assert torch.equal(Q[i], ref[i][0]) and torch.equal(R[i], ref[i][1])


def test_svd_trunc_batched_matches_single_calls(ops):
    g = torch.Generator(device='cuda').manual_seed(9)
    Rs = []
    for i in range(3):
        A = torch.randn((512, 96), dtype=torch.float64, device='cuda', generator=g) * \
            (10.0 ** (-torch.arange(96, dtype=torch.float64, device='cuda') / (6.0 + i)))
        Rs.append(ops.qr(A @ torch.randn((96, 128), dtype=torch.float64, device='cuda', generator=g))[1])
    Cm = torch.stack(Rs)
    out = ops.svd_trunc_batched(Cm, 64, 1e-17)
    for i in range(3):
        U, S, Vt, keep, disc, _ = ops.svd_trunc(Cm[i], 64, 1e-17)
        assert out[i][3] == keep and out[i][4] == disc
        assert torch.equal(out[i][0], U) and torch.equal(out[i][1], S) and torch.equal(out[i][2], Vt)


@pytest.mark.parametrize('nbo', [128, 256])
@pytest.mark.parametrize('colmajor', [False, True])
def test_qr_two_level_blocking(ops, nbo, colmajor):
    """The two-level blocked factorisation (outer blocks of 128 / 256 columns with merged T factors, csrc/qr.hip) on the
    pass-1 shape against the single-level one: same R up to rounding (diag >= 0 fixes the gauge), column-relative residual,
    orthogonality of Q, on a graded numerically rank-deficient matrix and on a full-rank one."""
    m, n = 16384, 1024
    g = torch.Generator(device='cuda').manual_seed(77)
    lowrank = (torch.randn((m, 200), dtype=torch.float64, device='cuda', generator=g) @
               torch.randn((200, n), dtype=torch.float64, device='cuda', generator=g)) * \
        torch.exp(-60.0 * torch.rand((1, n), dtype=torch.float64, device='cuda', generator=g))
    full = torch.randn((m, n), dtype=torch.float64, device='cuda', generator=g)
    saved = os.environ.get('TN_QR_NBO')
    try:
        for T in (lowrank, full):
            view = T.t().contiguous().t() if colmajor else T
            os.environ['TN_QR_NBO'] = '0'
            Q0, R0 = ops.qr(view)
            os.environ['TN_QR_NBO'] = str(nbo)
            Q, R = ops.qr(view)
            cn = torch.linalg.vector_norm(T, dim=0)
            assert float(((ops.mm(Q, R) - T).abs().max(dim=0).values / cn).max()) < 1e-13
            G = ops.mm(Q.t(), Q)
            assert float((G - torch.eye(n, dtype=torch.float64, device='cuda')).abs().max()) < 1e-13
            assert float(torch.tril(R, -1).abs().max()) == 0.0 and bool((torch.diagonal(R) >= 0).all())
            if T is full:          # well conditioned: the factors themselves agree with the single-level ones
                assert float((R - R0).abs().max()) < 1e-11 * float(R0.abs().max())
                assert float((Q - Q0).abs().max()) < 1e-11
    finally:
        if saved is None:
            os.environ.pop('TN_QR_NBO', None)
        else:
            os.environ['TN_QR_NBO'] = saved


# ------------------------------------------------------------------------------------------------ panel step of tn_qr
def _panel_cases():
    g = torch.Generator(device='cpu').manual_seed(7)
    rn = lambda *sh: torch.randn(*sh, dtype=torch.float64, generator=g).cuda()
    out = [('randn 16384x32', rn(16384, 32)), ('col-major', rn(32, 5000).t()), ('ragged 300x32', rn(300, 32)), ('square', rn(32, 32)),
           ('narrow 1000x17', rn(1000, 17)), ('single column', rn(5000, 1)),
           ('graded columns', rn(8192, 32) * torch.logspace(0, -30, 32, dtype=torch.float64).cuda()[None, :])]
    for kappa in (1e4, 1e8, 1e12, 1e15):
        U, _ = torch.linalg.qr(rn(4096, 32))
        V, _ = torch.linalg.qr(rn(32, 32))
        out.append(('kappa %.0e' % kappa, (U * torch.logspace(0, -float(np.log10(kappa)), 32, dtype=torch.float64).cuda()[None, :]) @ V.t()))
    X = rn(4096, 32)
    X[:, 5] = 0.0
    X[:, 9] = X[:, 2]
    X[:, 20] = 2.0 * X[:, 3]
    X[:, 31] = X[:, 0] + 1e-13 * X[:, 31]
    out += [('zero / duplicate / dependent columns', X), ('all zero', torch.zeros(2048, 32, dtype=torch.float64).cuda()),
            ('rank 3', rn(4096, 3) @ rn(3, 32)), ('scaled 1e-200', rn(2048, 32) * 1e-200), ('one block 1e150 larger', rn(4096, 32))]
    out[-1][1][:256] *= 1e150
    return out


def _panel_quality(X, Y):
    b = X.shape[1]
    orth = (Y.t() @ Y - torch.eye(b, dtype=torch.float64, device=X.device)).abs().max().item()
    cn = X.norm(dim=0)
    res = ((X - Y @ (Y.t() @ X)).norm(dim=0) / torch.where(cn > 0, cn, torch.ones_like(cn))).max().item()
    return orth, res


@pytest.mark.parametrize('method', [0])
def test_panel_orth_basis_of_the_column_space(ops, method):
    """tn_panel_orth (the panel step of tn_qr: iterated Cholesky-QR with deferral): an orthonormal basis to 2e-14 whose span contains every column of the panel to 2e-14 of its norm, on well-conditioned, graded,
    nearly dependent (kappa up to 1e15), rank-deficient, zero and badly scaled panels; the input is left untouched."""
    for name, X in _panel_cases():
        Xc = X.clone()
        Y = ops.panel_orth(X, method)
        assert torch.equal(X, Xc), name
        orth, res = _panel_quality(X, Y)
        assert orth < 2e-14 and res < 2e-14, (name, orth, res)


def test_panel_orth_state_and_reproducibility(ops):
    """A well-conditioned panel converges in one substitution pass, kappa = 1e12 needs deferrals and more passes, a zero column is
    refilled; two runs on the same panel are bit-identical (partial Gram matrices are summed in block order)."""
    cases = dict(_panel_cases())
    Y, st, dev = ops.panel_orth(cases['randn 16384x32'], 0, state=True)
    assert st[1] == 1 and st[3] == 1 and st[6] == 0 and st[7] == 0 and st[8] == 0 and dev[1] < 5e-15
    Y2 = ops.panel_orth(cases['randn 16384x32'], 0)
    assert torch.equal(Y, Y2)
    _, st, _ = ops.panel_orth(cases['kappa 1e+12'], 0, state=True)
    assert st[1] == 1 and st[3] >= 2 and st[6] > 0 and st[8] == 0
    _, st, _ = ops.panel_orth(cases['zero / duplicate / dependent columns'], 0, state=True)
    assert st[7] >= 1 and st[8] == 0


def test_qr_fused_panel_matches_lapack(ops):
    """tn_qr with the fused Cholesky-QR panel chain (orthonormalisation + Householder reconstruction + reflector products in
    cholqr.hip): a QR factorisation to rounding that agrees in |R| with LAPACK's Householder QR of the same matrix."""
    g = torch.Generator(device='cpu').manual_seed(11)
    rn = lambda *sh: torch.randn(*sh, dtype=torch.float64, generator=g).cuda()
    A = (rn(8192, 256) * torch.logspace(0, -20, 256, dtype=torch.float64).cuda()[None, :]) @ torch.linalg.qr(rn(256, 256))[0]
    mats = [rn(4096, 256), rn(300, 1000).t(), rn(300, 1000), rn(50, 7), rn(4096, 64) @ rn(64, 512), A]
    for T in mats:
        Q, R = ops.qr(T)
        k = Q.shape[1]
        rel = ((Q @ R - T).norm(dim=0) / T.norm(dim=0).clamp_min(1e-300)).max().item()
        orth = (Q.t() @ Q - torch.eye(k, dtype=torch.float64, device='cuda')).abs().max().item()
        assert rel < 1e-13 and orth < 1e-13, (tuple(T.shape), rel, orth)
        assert (torch.diagonal(R) >= 0).all()
        Th = T.cpu().numpy()
        Rref = np.linalg.qr(Th, mode='r')
        assert Rref.shape == tuple(R.shape)
        assert np.abs(np.abs(R.cpu().numpy()) - np.abs(Rref)).max() / np.abs(Th).max() < 1e-12, tuple(T.shape)


def _with_env(name, value, fn):
    saved = os.environ.get(name)
    try:
        os.environ[name] = value
        return fn()
    finally:
        if saved is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = saved


def test_panel_single_launch_bit_identical_to_chain(ops):
    """The single-launch panel step (cq_fused_kernel: <= 16 workgroups meeting at in-kernel barriers, every workgroup reducing /
    factoring redundantly) against the six-launch chain (TN_PANEL_FUSED=0) on every panel case of up to 4096 rows: the same basis
    bit for bit, the same pass / deferral / refill record."""
    n = 0
    for name, X in _panel_cases():
        if X.shape[0] > 8192:
            continue
        Y1, st1, dev1 = _with_env('TN_PANEL_FUSED', '1', lambda: ops.panel_orth(X, 0, state=True))
        Y0, st0, dev0 = _with_env('TN_PANEL_FUSED', '0', lambda: ops.panel_orth(X, 0, state=True))
        assert torch.equal(Y0, Y1), name
        assert st0[1] == st1[1] == 1 and st0[3] == st1[3] and st0[6:9] == st1[6:9], (name, st0, st1)
        assert dev0[:st0[3] + 1] == dev1[:st1[3] + 1], (name, dev0, dev1)
        n += 1
    assert n >= 12


def test_small_truncated_svd_single_launch(ops):
    """tn_svd_trunc with both dimensions <= 64 runs in ONE launch (svd_trunc_small_kernel: Hestenes sweeps with the rotations kept
    beside the vectors, truncation rule, sign gauge and outputs in the same workgroup): factors orthonormal, U S Vt = C to rounding,
    and kept rank / values / discarded weight as the block path (TN_SVD_SMALL=0) gives them -- square, wide, tall, rank-deficient,
    graded, 1 x 1 and strided inputs, with and without a truncation to Dmax."""
    g = torch.Generator(device='cpu').manual_seed(21)
    rn = lambda *sh: torch.randn(*sh, dtype=torch.float64, generator=g)
    graded = (rn(60, 60) * torch.logspace(0, -18, 60, dtype=torch.float64)[None, :]) @ torch.linalg.qr(rn(60, 60))[0]
    lowrank = rn(40, 7) @ rn(7, 33)
    cases = [('1x1', rn(1, 1), 64), ('16x16', rn(16, 16), 64), ('64x64', rn(64, 64), 64), ('64x64 Dmax 20', rn(64, 64), 20), ('15x60', rn(15, 60), 64),
             ('60x15', rn(60, 15), 8), ('graded', graded, 64), ('low rank', lowrank, 64), ('view', rn(50, 90)[:40, 10:70:2], 64),
             ('scaled', rn(30, 30) * 1e120, 64)]
    for name, Ch, Dmax in cases:
        Cm = Ch.cuda()
        k, n = Cm.shape
        U, S, Vt, keep, disc, info = ops.svd_trunc(Cm, Dmax, 1e-16)
        Sh = S.cpu().numpy()
        U0, S0, Vt0, keep0, disc0, info0 = _with_env('TN_SVD_SMALL', '0', lambda: ops.svd_trunc(Cm, Dmax, 1e-16))
        assert keep == keep0, (name, keep, keep0)
        S0h = S0.cpu().numpy()
        assert np.abs(Sh - S0h).max() <= 1e-13 * S0h[0], name
        assert abs(disc - disc0) <= 1e-12 * max(disc0, 1e-300) + 1e-15, (name, disc, disc0)
        Uh, Vh = U.cpu().numpy(), Vt.cpu().numpy()
        assert np.abs(Uh.T @ Uh - np.eye(keep)).max() < 1e-13 and np.abs(Vh @ Vh.T - np.eye(keep)).max() < 1e-13, name
        full = np.linalg.svd(Ch.numpy(), compute_uv=False)
        assert np.abs(Sh - full[:keep]).max() <= 1e-13 * full[0], name
        err = np.abs((Uh * Sh[None, :]) @ Vh - Ch.numpy()).max()
        tail = full[keep] if keep < full.size else 0.0
        assert err <= 1e-12 * full[0] + 1.01 * tail, (name, err, tail)
        # the reference's sign gauge holds on both sides
        flip = (np.abs(Uh.min(0)) > Uh.max(0)) & (np.abs(Vh.min(1)) > Vh.max(1))
        assert not flip.any(), name


def test_tiny_qr_single_workgroup(ops):
    """tn_qr on matrices of at most 4096 elements with min(m, n) <= 32 runs in ONE workgroup (tiny_qr_kernel: Householder in LDS):
    Q orthonormal, Q R = A, R upper triangular with diag(R) >= 0 -- on full-rank, rank-deficient, zero and badly scaled inputs -- and
    the same factors as the blocked path (TN_QR_TINY=0) where they are unique."""
    g = torch.Generator(device='cpu').manual_seed(11)
    rn = lambda *sh: torch.randn(*sh, dtype=torch.float64, generator=g)
    dup = rn(200, 12)
    dup[:, 5] = dup[:, 2]
    dup[:, 9] = 0.0
    cases = [('1x1', rn(1, 1)), ('1x1 negative', -rn(1, 1).abs()), ('1x300', rn(1, 300)), ('300x1', rn(300, 1)), ('16x16', rn(16, 16)),
             ('256x16', rn(256, 16)), ('128x32', rn(128, 32)), ('5x700', rn(5, 700)), ('32x128', rn(32, 128)), ('4096x1', rn(4096, 1)),
             ('dependent', dup), ('zero', torch.zeros(40, 8, dtype=torch.float64)), ('scaled', rn(100, 20) * 1e150),
             ('small', rn(100, 20) * 1e-150), ('transposed view', rn(24, 150).t())]
    for name, Th in cases:
        T = Th.cuda()
        m, n = T.shape
        k = min(m, n)
        Q, R = ops.qr(T)
        Qh, Rh, A = Q.cpu().numpy(), R.cpu().numpy(), Th.numpy()
        sc = max(np.abs(A).max(), 1e-300)
        assert np.abs(Qh.T @ Qh - np.eye(k)).max() < 1e-13, name
        assert np.abs(Qh @ Rh - A).max() <= 1e-13 * sc, name
        assert np.abs(np.tril(Rh, -1)).max() == 0.0 and (np.diag(Rh) >= 0).all(), name
        if name not in ('dependent', 'zero'):
            Q0, R0 = _with_env('TN_QR_TINY', '0', lambda: ops.qr(T))
            assert np.abs(R0.cpu().numpy() - Rh).max() <= 1e-12 * sc, name
            assert np.abs(Q0.cpu().numpy() - Qh).max() <= 1e-11, name


def test_q_accumulation_through_merged_reflectors(ops):
    """Single-level tn_qr from two panels on applies the reflectors to Q four panels at a time (apply_merged_T_kernel: block back
    substitution with the panels' T factors and the Gram matrix of the reflectors) -- against the panel-by-panel accumulation
    (TN_QR_MERGED_Q=0): the same R bit for bit (the forward loop is untouched), Q to rounding, orthonormal, Q R = A; widths that are
    not multiples of 32 or 128, both memory layouts, a graded matrix, and the pivoted truncating site factorisation."""
    g = torch.Generator(device='cpu').manual_seed(23)
    rn = lambda *sh: torch.randn(*sh, dtype=torch.float64, generator=g)
    graded = rn(3000, 300) * torch.logspace(0, -12, 300, dtype=torch.float64)[None, :]
    cases = [('2000x73', rn(2000, 73)), ('1500x200', rn(1500, 200)), ('4096x300', rn(4096, 300)), ('700x480', rn(700, 480)),
             ('row-major view', rn(260, 2500).t()), ('wide', rn(600, 900)), ('graded', graded), ('129 columns', rn(5000, 129))]
    for name, Th in cases:
        T = Th.cuda()
        m, n = T.shape
        k = min(m, n)
        Q, R = ops.qr(T)
        Q0, R0 = _with_env('TN_QR_MERGED_Q', '0', lambda: ops.qr(T))
        Qh, Rh, A = Q.cpu().numpy(), R.cpu().numpy(), Th.numpy()
        sc = np.abs(A).max()
        assert torch.equal(R, R0), name
        assert np.abs(Qh.T @ Qh - np.eye(k)).max() < 2e-13, name
        assert np.abs(Qh @ Rh - A).max() <= 2e-13 * sc, name
        assert np.abs(Q0.cpu().numpy() - Qh).max() <= 1e-12, name
    # pivoted, truncating (the first pass's factorisation): same rank, same permuted triangular factor, the bases agree to rounding
    U = torch.linalg.qr(rn(768, 200))[0]
    V = torch.linalg.qr(rn(16 * 150, 200))[0]
    B = ((U * torch.logspace(0, -18, 200, dtype=torch.float64)[None, :]) @ V.t()).contiguous()
    B = B[torch.argsort(B.norm(dim=1), descending=True)].contiguous().view(768, 16, 150).cuda()
    outs = []
    for mode in ('1', '0'):
        info = {}
        outs.append(_with_env('TN_QR_MERGED_Q', mode, lambda: ops.site_qr(1, B.clone(), None, rank_tol=1e-9, normalise=False, info=info,
                                                                        frobenius_exit=True, pivot=True)) + (info,))
    (Q1, R1, k1, _, i1), (Q2, R2, k2, _, i2) = outs
    assert k1 == k2 and 64 < k1 < 200
    assert torch.equal(R1, R2)
    assert float((Q1 - Q2).abs().max()) <= 1e-12
    Q1f = Q1.reshape(k1, -1)
    assert float((Q1f @ Q1f.t() - torch.eye(k1, dtype=torch.float64, device='cuda')).abs().max()) < 2e-13


def test_hard_panels_of_a_real_sweep(ops):
    """tests/golden/g12_hard_panels.npz: the panels of tn_qr that needed FOUR substitution passes in the boundary-MPS sweep of the
    headline instance (chimera L = 2048, chi = 64, seed 20260004; 11 of 6 025 panels, the nine of <= 4096 rows kept; condition numbers
    1e16 .. 1e23; captured with tools/capture_panels.py).  Both forms of the panel step must still take them in four passes without
    the Householder fallback, return an orthonormal basis that spans the panel, and agree bit for bit."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g12_hard_panels.npz'))
    n = 0
    while 'panel%d' % n in g:
        Xh = g['panel%d' % n]
        X = torch.as_tensor(Xh).cuda()
        Y1, st1, dev1 = _with_env('TN_PANEL_FUSED', '1', lambda: ops.panel_orth(X, 0, state=True))
        Y0, st0, dev0 = _with_env('TN_PANEL_FUSED', '0', lambda: ops.panel_orth(X, 0, state=True))
        assert torch.equal(Y0, Y1), n
        assert st0[3] == st1[3] == int(g['passes%d' % n][0]) and st0[8] == st1[8] == 0, (n, st0, st1)
        Y = Y1.cpu().numpy()
        b = Xh.shape[1]
        assert np.abs(Y.T @ Y - np.eye(b)).max() < 1e-13, n
        assert np.linalg.norm(Xh - Y @ (Y.T @ Xh)) <= 1e-13 * np.linalg.norm(Xh), n
        n += 1
    assert n == 9


def test_panel_statistics_are_kept_per_stream(ops):
    """tn_panel_stats_stream: the diagnostic counters of the panel step belong to the launching stream (concurrent chains do not mix
    their counts); tn_panel_stats is their sum over the streams."""
    g = torch.Generator(device='cpu').manual_seed(3)
    A = torch.randn(1024, 96, dtype=torch.float64, generator=g).cuda()
    B = torch.randn(2048, 80, dtype=torch.float64, generator=g).cuda()        # (more than 64 columns: the panel path)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ops.panel_stats(reset=True)
    with torch.cuda.stream(s1):
        ops.qr(A)
        ops.qr(A)
    with torch.cuda.stream(s2):
        ops.qr(B)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        st1 = ops.panel_stats(stream=True)
    with torch.cuda.stream(s2):
        st2 = ops.panel_stats(stream=True)
    tot = ops.panel_stats()
    assert st1['panels'] == 6 and st2['panels'] == 3 and tot['panels'] == 9
    for k in ops.PANEL_STAT_KEYS:
        assert st1[k] + st2[k] == tot[k], k
    with torch.cuda.stream(s1):
        ops.panel_stats(reset=True, stream=True)               # resetting one stream leaves the other alone
        assert ops.panel_stats(stream=True)['panels'] == 0
    assert ops.panel_stats()['panels'] == 3


TALL_PANEL_CHILD = r'''
import os, sys
sys.path.insert(0, %(root)r)
import torch
from tnac4o_amd import ops
g = torch.Generator(device='cpu').manual_seed(5)
ok = True
for rows in (16384, 12000, 8200):
    X = (torch.randn(rows, 32, dtype=torch.float64, generator=g) * torch.logspace(0, -9, 32, dtype=torch.float64)[None, :]).cuda()
    res = {}
    for big in ('1', '0'):
        os.environ['TN_PANEL_FUSED_BIG'] = big
        ops.panel_stats(reset=True)
        Q, R = ops.qr(X)
        torch.cuda.synchronize()
        res[big] = (Q, R, ops.panel_stats())
    ok &= torch.equal(res['1'][0], res['0'][0]) and torch.equal(res['1'][1], res['0'][1])
    ok &= res['1'][2]['single_launch_panels'] == 1 and res['0'][2]['single_launch_panels'] == 0
    ok &= float((res['1'][0].t() @ res['1'][0] - torch.eye(32, dtype=torch.float64, device='cuda')).abs().max()) < 1e-13
print('TALL_OK' if ok else 'TALL_FAIL')
'''


def test_tall_panels_single_launch_when_admitted(ops):
    """Panels of more than 8192 rows (up to 64 workgroups) take the single-launch form when the co-residency budget admits them
    (csrc/fused.hip: FusedTallLaunch): in a fresh process with one stream they always are -- same bits as the six-launch chain
    (TN_PANEL_FUSED_BIG=0), and the statistics show which form ran."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop('TN_PANEL_FUSED_BIG', None)
    out = subprocess.run([sys.executable, '-c', TALL_PANEL_CHILD % dict(root=root)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'TALL_OK' in out.stdout, out.stdout[-2000:]


def test_qr_single_launch_panels_bit_identical_to_chain(ops):
    """tn_qr with the single-launch panel step (orthonormalisation + Householder reconstruction + reflector products in ONE
    kernel per panel) against the six-launch chain: Q and R bit-identical on tall, wide, ragged, rank-deficient and graded
    matrices, plain and with the rank-revealing early exit; also through the Householder fallback (TN_PANEL_MAXPASS is read once
    per process, so that path is covered by the dedicated fallback test below when the variable is set)."""
    g = torch.Generator(device='cpu').manual_seed(23)
    rn = lambda *sh: torch.randn(*sh, dtype=torch.float64, generator=g).cuda()
    A = (rn(4096, 256) * torch.logspace(0, -20, 256, dtype=torch.float64).cuda()[None, :]) @ torch.linalg.qr(rn(256, 256))[0]
    mats = [rn(4096, 256), rn(300, 1000).t(), rn(300, 1000), rn(50, 7), rn(4096, 64) @ rn(64, 512), A, rn(2048, 1024), rn(33, 33),
            rn(1500, 700), torch.zeros(512, 64, dtype=torch.float64).cuda(), rn(8192, 160), rn(8000, 96) @ rn(96, 300)]
    for T in mats:
        for tol in (0.0, 2.0 ** -56):
            def run():
                m, nn = T.shape
                k = min(m, nn)
                Q = torch.zeros((m, k), dtype=torch.float64, device='cuda')
                R = torch.zeros((k, nn), dtype=torch.float64, device='cuda')
                _, _, ke = ops.qr_into(T, Q, R, rank_tol=tol)
                return Q[:, :ke].clone(), R[:ke].clone(), ke
            # (TN_QR_SMALL=0: matrices of up to 64 columns would otherwise take the one-launch factorisation, not the panel step)
            Q1, R1, k1 = _with_env('TN_QR_SMALL', '0', lambda: _with_env('TN_PANEL_FUSED', '1', run))
            Q0, R0, k0 = _with_env('TN_QR_SMALL', '0', lambda: _with_env('TN_PANEL_FUSED', '0', run))
            assert k0 == k1 and torch.equal(Q0, Q1) and torch.equal(R0, R1), (tuple(T.shape), tol, k0, k1)
            if float(T.abs().max()) > 0:
                # column by column; after an exit every column may miss by tol x the largest column norm (the header's contract)
                cn = T.norm(dim=0)
                res = (Q1 @ R1 - T).norm(dim=0)
                assert bool((res <= 1e-13 * cn + tol * cn.max()).all()), (tuple(T.shape), tol, (res / cn.clamp_min(1e-300)).max().item())


def test_qr_single_launch_panels_under_uneven_load(ops):
    """The in-kernel barriers of the single-launch panel step under uneven load: four chains factor different matrices on four
    streams while a fifth stream keeps the device full of large GEMMs; every result equals the one obtained alone (bit for bit).
    (Guideline 16 of the MI355X guide: hand-offs must be tested with busy, L1-warm consumers.)"""
    import threading
    g = torch.Generator(device='cpu').manual_seed(29)
    rn = lambda *sh: torch.randn(*sh, dtype=torch.float64, generator=g).cuda()
    mats = [rn(8192, 256), rn(3000, 256), rn(6000, 384), rn(1024, 1024)]          # (8192 rows: 32 workgroups per panel launch)
    ref = [ops.qr(T) for T in mats]
    torch.cuda.synchronize()
    big_a, big_b = rn(4096, 4096), rn(4096, 4096)
    streams = [torch.cuda.Stream() for _ in range(5)]
    out, err = [None] * 4, []
    stop = threading.Event()

    def chain(i):
        try:
            with torch.cuda.stream(streams[i]):
                for _ in range(6):
                    out[i] = ops.qr(mats[i])
                streams[i].synchronize()
        except BaseException as e:          # noqa: BLE001
            err.append(e)

    def load():
        with torch.cuda.stream(streams[4]):
            while not stop.is_set():
                ops.mm(big_a, big_b)
                streams[4].synchronize()
    th = [threading.Thread(target=chain, args=(i,)) for i in range(4)]
    tl = threading.Thread(target=load)
    tl.start()
    for t in th:
        t.start()
    for t in th:
        t.join()
    stop.set()
    tl.join()
    assert not err, err
    for i in range(4):
        assert torch.equal(out[i][0], ref[i][0]) and torch.equal(out[i][1], ref[i][1]), i


# ------------------------------------------------------------------------------------------------ one-launch factorisation (smallqr.hip)
def _smallqr_cases():
    g = torch.Generator(device='cpu').manual_seed(31)
    rn = lambda *sh: torch.randn(*sh, dtype=torch.float64, generator=g)
    dep = rn(900, 64)
    dep[:, 7] = dep[:, 2]
    dep[:, 40] = 0.0
    dep[:, 50:58] = dep[:, 10:18] @ rn(8, 8)
    graded = rn(1024, 64) * torch.logspace(0, -14, 64, dtype=torch.float64)[None, :]
    illc = rn(2000, 48) @ (torch.linalg.qr(rn(48, 48))[0] * torch.logspace(0, -12, 48, dtype=torch.float64)[None, :]) @ torch.linalg.qr(rn(48, 48))[0]
    return [('1024x64', rn(1024, 64)), ('1000x60', rn(1000, 60)), ('129x64', rn(129, 64)), ('64x64', rn(64, 64)), ('65x33', rn(65, 33)),
            ('4096x64', rn(4096, 64)), ('4000x37', rn(4000, 37)), ('256x16', rn(256, 16)), ('300x32', rn(300, 32)), ('8192x32', rn(8192, 32)),
            ('7000x20', rn(7000, 20)), ('130x1', rn(130, 1) + 3.0), ('column-major', rn(64, 1500).t()), ('column-major 24', rn(24, 5000).t()),
            ('dependent', dep), ('zero', torch.zeros(700, 40, dtype=torch.float64)), ('ones', torch.ones(900, 64, dtype=torch.float64)),
            ('graded', graded), ('ill-conditioned', illc), ('scaled up', rn(1500, 50) * 1e150), ('scaled down', rn(1500, 50) * 1e-150),
            ('row graded', rn(2048, 64) * torch.logspace(0, -200, 2048, dtype=torch.float64)[:, None])]


def test_smallqr_single_launch(ops):
    """tn_qr on matrices of up to 64 columns (m >= n, at most 32 workgroups of rows) runs as ONE launch (csrc/smallqr.hip: explicit-Q
    iterated Cholesky-QR across workgroups that meet at in-kernel barriers): Q orthonormal, Q R = A column-wise to rounding, R upper
    triangular with diag(R) >= 0 on full-rank, dependent, zero, graded, ill-conditioned, badly scaled and strided inputs; the same R as
    the blocked Householder path (TN_QR_SMALL=0) where it is unique; bit-reproducible; the input untouched."""
    ops.smallqr_stats(reset=True)
    ncall = 0
    for name, Th in _smallqr_cases():
        T = Th.cuda()
        keep = T.clone()
        m, n = T.shape
        Q, R = ops.qr(T)
        ncall += 0 if (m * n <= 4096 and n <= 32) else 1          # (the tiniest ones stay with tiny_qr_kernel)
        assert torch.equal(T, keep), name
        Qh, Rh, A = Q.cpu().numpy(), R.cpu().numpy(), Th.numpy()
        cn = np.sqrt((A * A).sum(0))
        cn[cn == 0] = 1.0
        assert np.abs(Qh.T @ Qh - np.eye(n)).max() < 2e-14, name
        assert (np.abs(Qh @ Rh - A) / cn).max() < 5e-14, name
        assert np.abs(np.tril(Rh, -1)).max() == 0.0 and (np.diag(Rh) >= 0).all(), name
        Q2, R2 = ops.qr(T)
        ncall += 0 if (m * n <= 4096 and n <= 32) else 1
        assert torch.equal(Q, Q2) and torch.equal(R, R2), name
        if name not in ('dependent', 'zero', 'ones', 'ill-conditioned', 'graded'):
            Q0, R0 = _with_env('TN_QR_SMALL', '0', lambda: ops.qr(T))
            sc = np.abs(A).max()
            assert np.abs(R0.cpu().numpy() - Rh).max() <= 1e-12 * sc, name
            assert np.abs(Q0.cpu().numpy() - Qh).max() <= 1e-11, name
    st = ops.smallqr_stats()
    # (63 exact copies of one column -- 'ones' -- is the one case whose passes run out: Householder fallback, valid factors all the same)
    assert st['calls'] == ncall and st['householder_fallbacks'] <= 2 and st['timeouts'] == 0, st
    assert st['passes'] <= 2.0 * ncall, st


def test_smallqr_fused_normalisation_in_site_qr(ops):
    """tn_site_qr on a site whose matrix takes the one-launch path: the triangular factor comes out divided by its power-of-two norm
    factor (mps.py:76-85) from the same launch -- same Q, R and factor as the blocked path followed by tn_normalize_pow2 give up to
    rounding, and the factor is the exact power of two."""
    g = torch.Generator(device='cpu').manual_seed(32)
    for side, shape, cshape in ((0, (64, 16, 64), None), (1, (64, 16, 64), None), (0, (48, 16, 60), (40, 48)), (1, (60, 16, 48), (48, 40))):
        A = (torch.randn(*shape, dtype=torch.float64, generator=g) * 37.0).cuda()
        Cm = torch.randn(*cshape, dtype=torch.float64, generator=g).cuda() if cshape else None
        Q1, R1, k1, nf1 = ops.site_qr(side, A.clone(), Cm)
        Q0, R0, k0, nf0 = _with_env('TN_QR_SMALL', '0', lambda: ops.site_qr(side, A.clone(), Cm))
        assert k1 == k0
        assert float(nf1[0]) == float(nf0[0]) and float(nf1[0] * nf1[1]) == 1.0
        assert float((R1 - R0).abs().max()) < 1e-12 and float((Q1 - Q0).abs().max()) < 1e-11
        assert 0.5 <= float(R1.abs().max()) and float(R1.abs().max()) < 2.0


SMALLQR_CHILD = r'''
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
from tnac4o_amd import ops
g = torch.Generator(device='cpu').manual_seed(7)
ok = True
for shape in ((1024, 64), (3000, 40), (200, 64), (5000, 17)):
    # condition number 1e9 that no column scaling removes: one substitution pass cannot orthonormalise these
    Th = torch.randn(*shape, dtype=torch.float64, generator=g) @ (torch.logspace(0, -9, shape[1], dtype=torch.float64)[:, None] * torch.randn(shape[1], shape[1], dtype=torch.float64, generator=g))
    T = Th.cuda()
    Q, R = ops.qr(T)
    Qh, Rh, A = Q.cpu().numpy(), R.cpu().numpy(), Th.numpy()
    cn = np.sqrt((A * A).sum(0))
    ok &= bool(np.abs(Qh.T @ Qh - np.eye(shape[1])).max() < 1e-13 and (np.abs(Qh @ Rh - A) / cn).max() < 1e-13)
    ok &= bool(np.abs(np.tril(Rh, -1)).max() == 0.0 and (np.diag(Rh) >= 0).all())
    ok &= bool(np.isfinite(Qh).all() and np.isfinite(Rh).all())
st = ops.smallqr_stats()
print('STATS', st)
print('CHILD_OK' if ok else 'CHILD_FAIL')
'''


def _run_child(code, env_extra):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, '-c', code % dict(root=root)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout + '\n--- stderr ---\n' + r.stderr


def test_smallqr_householder_fallback():
    """TN_PANEL_MAXPASS=1 leaves the passes no chance on graded inputs: workgroup 0 of the launch redoes the factorisation with
    Householder reflections (sq_fallback_householder) -- valid factors all the same, and the counter shows the path ran."""
    out = _run_child(SMALLQR_CHILD, {'TN_PANEL_MAXPASS': '1'})
    assert 'CHILD_OK' in out, out
    assert "'householder_fallbacks': 0" not in out, out


def test_barrier_timeouts_are_recovered_not_returned():
    """TN_PANEL_SPIN_LIMIT=0 makes every in-kernel barrier with more than one workgroup give up at once (what happens when the
    co-residency budget does not hold: another tenant on the card): the launch poisons its outputs and books the time-out, the entry
    point notices at its read-back and redoes the factorisation through the blocked path -- the caller never sees NaN, and the
    counters show that launches did give up."""
    out = _run_child(SMALLQR_CHILD, {'TN_PANEL_SPIN_LIMIT': '0'})
    assert 'CHILD_OK' in out, out
    assert "'timeouts': 0" not in out, out


def test_smallqr_under_uneven_load(ops):
    """The in-kernel barriers and hand-offs of the one-launch factorisation under uneven load: four chains factor 1024 x 64-class
    matrices on four streams while a fifth keeps the device full of large GEMMs; every result equals the one obtained alone, bit for
    bit (Guideline 16 of the MI355X guide: hand-offs must be tested with busy, L1-warm consumers, every word checked)."""
    import threading
    g = torch.Generator(device='cpu').manual_seed(41)
    rn = lambda *sh: torch.randn(*sh, dtype=torch.float64, generator=g).cuda()
    mats = [rn(1024, 64), rn(4096, 64) * torch.logspace(0, -8, 64, dtype=torch.float64).cuda()[None, :], rn(3000, 48), rn(8192, 32)]
    ref = [ops.qr(T) for T in mats]
    torch.cuda.synchronize()
    big_a, big_b = rn(4096, 4096), rn(4096, 4096)
    streams = [torch.cuda.Stream() for _ in range(5)]
    bad, err = [0] * 4, []
    stop = threading.Event()

    def chain(i):
        try:
            with torch.cuda.stream(streams[i]):
                for _ in range(40):
                    Q, R = ops.qr(mats[i])
                    if not (torch.equal(Q, ref[i][0]) and torch.equal(R, ref[i][1])):
                        bad[i] += 1
                streams[i].synchronize()
        except BaseException as e:          # noqa: BLE001
            err.append(e)

    def load():
        with torch.cuda.stream(streams[4]):
            while not stop.is_set():
                ops.mm(big_a, big_b)
                streams[4].synchronize()
    th = [threading.Thread(target=chain, args=(i,)) for i in range(4)]
    tl = threading.Thread(target=load)
    tl.start()
    for t in th:
        t.start()
    for t in th:
        t.join()
    stop.set()
    tl.join()
    assert not err, err
    assert bad == [0, 0, 0, 0], bad


TIMEOUT_CHILD = r'''
import os, sys, hashlib
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import numpy as np
import torch
import golden_inputs as gi
import tnac4o_amd
from tnac4o_amd import ops
g = torch.Generator(device='cpu').manual_seed(13)
h = hashlib.sha256()
# (a) a whole sweep + search through tn_compress_mps on the default stream (droplet L = 128 #1, chi = 32: site matrices of several
# workgroups): the first row whose launches give up is redone by the library
s = tnac4o_amd.tnac4o(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=3.0)
s.search_ground_state(M=256, relative_P_cutoff=1e-8, Dmax=32)
ok = True
for m in s.rhoT:
    for a in m.A:
        ok &= bool(torch.isfinite(a).all())
        h.update(a.cpu().numpy().tobytes())
h.update(np.asarray(s.energy[:1]).tobytes()); h.update(np.asarray(s.probability[:1]).tobytes())
seen = ops.smallqr_stats()['timeouts']
# (b) tn_qr through the Python wrapper on a FRESH stream (the default one has been taken off the single-launch forms by now): panels of
# 16 workgroups (4096 rows), graded columns; the wrapper retries from its clone after -7
with torch.cuda.stream(torch.cuda.Stream()):
    T = (torch.randn(4096, 256, dtype=torch.float64, generator=g) * torch.logspace(0, -8, 256, dtype=torch.float64)[None, :]).cuda()
    Q, R = ops.qr(T)
    torch.cuda.current_stream().synchronize()
    ok &= bool(torch.isfinite(Q).all() and torch.isfinite(R).all())
    ok &= float((Q.t() @ Q - torch.eye(256, dtype=torch.float64, device='cuda')).abs().max()) < 1e-13
    h.update(Q.cpu().numpy().tobytes()); h.update(R.cpu().numpy().tobytes())
print('TIMEOUTS_SEEN', seen)
print('DIGEST', h.hexdigest())
print('CHILD_OK' if ok else 'CHILD_FAIL')
'''


def test_barrier_timeouts_recovered_bit_identical_to_the_multi_launch_forms():
    """A process in which EVERY in-kernel barrier of more than one workgroup gives up at once (TN_PANEL_SPIN_LIMIT=0: what a
    co-residency budget that does not hold looks like) against a process that never uses the single-launch forms (TN_PANEL_FUSED=0):
    tn_qr (via the wrapper's retry from its clone after -7) and a whole contraction + search through tn_compress_mps (which checks once
    per row and redoes the row) return finite results that agree BIT FOR BIT with the multi-launch forms -- NaN never leaves the library."""
    out_t = _run_child(TIMEOUT_CHILD, {'TN_PANEL_SPIN_LIMIT': '0'})
    out_c = _run_child(TIMEOUT_CHILD, {'TN_PANEL_FUSED': '0'})
    assert 'CHILD_OK' in out_t and 'CHILD_OK' in out_c, (out_t, out_c)
    # launches did give up in the first process (the library says so on stderr, once per recovery), on both streams
    assert out_t.count('[libtnpeps]') >= 2 and '[libtnpeps]' not in out_c, (out_t, out_c)
    dig = lambda o: [l for l in o.splitlines() if l.startswith('DIGEST')][0]
    assert dig(out_t) == dig(out_c), (out_t, out_c)


@pytest.mark.parametrize('shape', [(256, 16, 24, 40), (1024, 16, 40, 100), (300, 8, 33, 70), (64, 4, 100, 20)])
def test_pivoted_site_qr_device_selection(ops, shape):
    """The pivoted, truncating site QR of the weighted first pass (tn_site_qr side 1, Frobenius exit, panel pivoting) with the pivots
    chosen on the device (pivot_select_kernel: norms added up, exit test, rank counting, swap list and permutation in device memory,
    the host one panel ahead) against the host selection (TN_PIVOT_DEVICE=0): Q orthonormal, Q^T-form factors reproduce the permuted
    input up to the dropped block, the dropped norm is what is really left, and both forms accept the same rank (ties aside they
    choose the same columns: R agrees to rounding)."""
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
    outs = []
    for mode in ('1', '0'):
        info = {}
        Bd = B.cuda().view(Dl, p, r).clone()
        Qt, Ct, k, _ = _with_env('TN_PIVOT_DEVICE', mode, lambda: ops.site_qr(1, Bd, None, rank_tol=tol, normalise=False, info=info,
                                                                                frobenius_exit=True, pivot=True))
        perm = info['perm'].cpu().numpy()
        assert sorted(perm.tolist()) == list(range(Dl))
        Qh, Ch = Qt.cpu().numpy(), Ct.cpu().numpy()              # Q^T (k x m), R^T (Dl x k): B[perm]^T = Q R  <=>  B[perm] = R^T Q^T
        assert np.abs(Qh @ Qh.T - np.eye(k)).max() < 1e-13
        Bp = B.numpy()[perm]
        # factored in the pivoted order: R^T is lower trapezoidal (row j of R^T = input column perm[j])
        assert np.abs(np.triu(Ch[:k, :k], 1)).max() <= 1e-13 * np.abs(Ch).max()
        res = Bp - Ch @ Qh
        fro = np.linalg.norm(B.numpy())
        assert abs(np.linalg.norm(res) - np.sqrt(info['dropped2'])) <= 1e-12 * fro + 1e-3 * np.sqrt(info['dropped2'])
        assert np.linalg.norm(res) <= tol * fro * 1.0000001 or k == min(m, Dl)
        assert np.all(np.diag(Ch[:k, :k]) >= 0)
        outs.append((k, perm, Ch, info['dropped2']))
    (k1, p1, C1, d1), (k0, p0, C0, d0) = outs
    assert k1 == k0
    if np.array_equal(p1[:k1], p0[:k0]):            # (the columns behind the accepted ones may sit in another order: compare by input column)
        A1, A0 = np.empty_like(C1), np.empty_like(C0)
        A1[p1], A0[p0] = C1, C0
        assert np.abs(A1[:, :k1] - A0[:, :k0]).max() <= 1e-12 * np.abs(C0).max()
        assert abs(d1 - d0) <= 1e-9 * max(d0, 1e-300)


@pytest.mark.parametrize('shape,gap', [((128, 300), 1e-10), ((192, 192), 1e-12), ((100, 100), 1e-11), ((64, 64), 1e-10)])
def test_svd_clustered_spectrum_orthogonality(ops, shape, gap):
    """Singular values that are close but distinct (relative gaps 1e-10 .. 1e-12: rotation angles inside a cluster are O(1) however
    small the off-diagonals) -- the case the quadratic-convergence shortcut of the Jacobi sweeps (a sweep that met nothing above 1e-9
    is not followed by a verification sweep) has to survive: U and V^T orthonormal to 1e-13, values to 1e-13 S0, U S V^T = C."""
    k, n = shape
    r = min(k, n)
    g = np.random.default_rng(int(1e12 * gap) + k)
    U0, _ = np.linalg.qr(g.standard_normal((k, r)))
    V0, _ = np.linalg.qr(g.standard_normal((n, r)))
    sv = np.exp(-0.05 * np.arange(r))
    for c0 in (0, 10, r // 2):                       # three clusters of 8 values each
        sv[c0:c0 + 8] = sv[c0] * (1.0 - gap * np.arange(8))
    sv = np.sort(sv)[::-1]
    A = (U0 * sv) @ V0.T
    U, S, Vt, keep, disc, info = ops.svd_trunc(dev(A), r, 1e-16)
    Uh, Sh, Vh = U.cpu().numpy(), S.cpu().numpy(), Vt.cpu().numpy()
    assert keep == r and info['info'] == 0
    assert np.abs(Uh.T @ Uh - np.eye(r)).max() < 1e-13 and np.abs(Vh @ Vh.T - np.eye(r)).max() < 1e-13
    assert np.abs(Sh - sv).max() <= 1e-13 * sv[0]
    assert np.abs((Uh * Sh) @ Vh - A).max() <= 1e-13 * sv[0]
