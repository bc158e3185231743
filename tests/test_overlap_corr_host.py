"""Host side of tnac4o.calculate_overlap_correlations (tnac4o_amd/overlap.py) and the argument errors of tn_pair_moments.  No GPU."""
import numpy as np
import pytest

import overlap_corr_ref as cref
import overlap_ref as oref
from overlap_ref import droplet, ising3x3, last_error, rmf
from tnac4o_amd import overlap as ov


# ---------------------------------------------------------------------------------------------- 1. pack_groups
@pytest.mark.parametrize('lanes16', [False, True])
def test_pack_groups_round_trips(lanes16):
    """Group g of the packed rows holds exactly the columns whose group index is g, in their order; the padding is zero.  Uneven
    sizes, empty groups, a group of more than one word."""
    rng = np.random.default_rng(5)
    per = 4 if lanes16 else 64
    G = 6
    sizes = [3, 0, per + 1, 1, 0, per]                                 # groups 1 and 4 are empty, group 2 takes two words
    group = rng.permutation(np.repeat(np.arange(G), sizes))
    X = rng.integers(0, 32768 if lanes16 else 2, (9, group.size))
    rows, wpg = ov.pack_groups(X, group, G, lanes16)
    assert wpg == 2 and rows.dtype == np.uint64 and rows.shape == (9, G * wpg)
    for g in range(G):
        U = oref.unpack_rows(rows[:, g * wpg:(g + 1) * wpg], wpg * per, lanes16)
        assert np.array_equal(U[:, :sizes[g]], X[:, group == g]), g
        assert not U[:, sizes[g]:].any(), g
    # one group of everything is the dense packing
    dense, w1 = ov.pack_groups(X, np.zeros(group.size, dtype=int), 1, lanes16)
    assert np.array_equal(dense, ov.pack_lanes16(X) if lanes16 else ov.pack_bits(X)) and w1 == dense.shape[1]
    # no columns at all: one zero word per group
    none, w0 = ov.pack_groups(np.zeros((2, 0), dtype=int), np.zeros(0, dtype=int), 3, lanes16)
    assert w0 == 1 and none.shape == (2, 3) and not none.any()
    for bad in (np.full(group.size, G), np.full(group.size, -1), np.zeros(group.size + 1, dtype=int)):
        with pytest.raises(ValueError):
            ov.pack_groups(X, bad, G, lanes16)


# ---------------------------------------------------------------------------------------------- 2. line_groups
@pytest.mark.parametrize('which', ['droplet', 'ising3x3'])
def test_line_groups(which):
    s = droplet() if which == 'droplet' else ising3x3()
    Nx, Ny = (4, 4) if which == 'droplet' else (3, 3)
    act = np.sort(np.concatenate([np.asarray(a) for row in s.ind0 for a in row]))
    where = {int(i): (ny, nx) for ny in range(Ny) for nx in range(Nx) for i in s.ind0[ny][nx]}
    for axis, G in (('x', Nx), ('y', Ny)):
        group, sizes = ov.line_groups(s, axis, 'spin')
        assert group.shape == (s.active,) and sizes.shape == (G,) and sizes.sum() == s.active
        assert np.array_equal(sizes, np.bincount(group, minlength=G))
        for k, spin in enumerate(act):                                 # bit k of spin_bits is active spin act[k]
            assert group[k] == where[int(spin)][1 if axis == 'x' else 0], (axis, k)
        cg, cs = ov.line_groups(s, axis, 'cell')
        assert cg.tolist() == [(k % Nx) if axis == 'x' else (k // Nx) for k in range(Nx * Ny)] and cs.tolist() == [Nx * Ny // G] * G
    if which == 'ising3x3':                                            # spin 9 has no term: it is in no cell's list and in no group
        assert 9 not in where and s.active == 17 and ov.line_groups(s, 'x', 'spin')[0].size == 17
        assert ov.line_groups(s, 'x', 'spin')[1].tolist() == [6, 5, 6] and ov.line_groups(s, 'y', 'spin')[1].tolist() == [6, 5, 6]
    for bad in (('z', 'spin'), ('x', 'link')):
        with pytest.raises(ValueError):
            ov.line_groups(s, *bad)
    with pytest.raises(ValueError):
        ov.line_groups(rmf(), 'x', 'spin')
    assert ov.line_groups(rmf(), 'y', 'cell')[0].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]


# ---------------------------------------------------------------------------------------------- 3. quantise(W, wmax)
def _quantise_before(W):
    """quantise as it stood before it took wmax (restated)."""
    WMAX = 2 ** 32 - 1
    W = np.asarray(W, dtype=np.float64)
    if W.size == 0:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=bool), 1.0
    if np.all(W == np.rint(W)) and W.max() <= WMAX:
        wq, scale = W, 1.0
    else:
        full = WMAX / float(W.max())
        best = None
        for sc in (full, 2.0 ** np.floor(np.log2(full))):
            q = np.minimum(np.rint(W * sc), WMAX)
            err = float(np.sum(np.abs(q / sc - W)))
            if best is None or err < best[0]:
                best = (err, q, sc)
        _, wq, scale = best
    wq = wq.astype(np.uint32)
    return wq, wq > 0, float(scale)


def test_quantise_with_wmax():
    rng = np.random.default_rng(8)
    c = rng.integers(1, 700, 3000).astype(np.float64)
    inputs = [np.array([3.0, 1.0, 0.0, 2.0 ** 32 - 1]), np.array([2.0 ** 32, 1.0, 0.0]), np.array([0.3, 0.7, 1e-3, 0.7e-11, 2.1e-10]),
              c * (1.0 - 1e-12 * rng.random(3000)), 10.0 ** rng.uniform(-12, 0, 500), np.zeros(0)]
    for W in inputs:                                                   # the default is what it was
        got, want = ov.quantise(W), _quantise_before(W)
        assert np.array_equal(got[0], want[0]) and got[0].dtype == np.uint32 and np.array_equal(got[1], want[1]) and got[2] == want[2]
    for wmax in (1, 1000, (2 ** 32 - 1) // 128, (2 ** 32 - 1) // 2048):
        for W in inputs[:-1]:
            wq, keep, scale = ov.quantise(W, wmax=wmax)
            assert wq.max() <= wmax and np.array_equal(keep, wq > 0)
            if np.all(W == np.rint(W)) and W.max() <= wmax:
                assert scale == 1.0 and np.array_equal(wq, W)
            else:                                                      # within half a unit of one of the two scales, the largest at most wmax
                assert scale <= wmax / W.max() and scale >= 0.5 * wmax / W.max()
                assert np.all(np.abs(wq - W * scale) <= 0.5)
    assert ov.quantise(np.array([5.0, 1000.0]), wmax=1000)[2] == 1.0   # integers up to wmax pass through
    assert ov.quantise(np.array([5.0, 1001.0]), wmax=1000)[2] < 1.0
    for bad in (0, 2 ** 32):
        with pytest.raises(ValueError):
            ov.quantise(np.ones(3), wmax=bad)


# ---------------------------------------------------------------------------------------------- 4. chi and xi by hand
def test_chi_and_xi_closed_forms():
    """The reference is the closed form: sum_{g,g'} cos(k_m (g - g')) = G^2 [m = 0], and sum_{g,g'} cos(k_a (g - g')) cos(k_m (g - g'))
    = G^2 / 2 [m = a] for 0 < a < G / 2 (G^2 for a = G / 2), 0 otherwise."""
    G, n = 8, 5.0
    N = G * n
    QQ = np.full((G, G), n * n)                                        # every Q_g = n_g: all of it at k = 0
    chi, xi = ov.correlation_length(QQ, N)
    assert chi.shape == (G // 2 + 1,) and chi[0] == pytest.approx(G * G * n * n / N, rel=1e-12)
    assert np.all(np.abs(chi[1:]) <= 1e-12 * chi[0])
    assert np.isnan(xi)                                                # chi(k_1) is zero to rounding: no ratio
    dg = np.arange(G)[:, None] - np.arange(G)[None, :]
    for a in (1, 2, 3, 4):
        A = 3.7
        chi = ov.chi_of_k(A * np.cos(2 * np.pi * a * dg / G), N)
        want = np.zeros(G // 2 + 1)
        want[a] = A * G * G / N * (1.0 if a == G // 2 else 0.5)
        assert chi[a] == pytest.approx(want[a], rel=1e-12)
        assert np.all(np.abs(chi - want) <= 1e-12 * want[a])
    # a constant plus the first mode: chi(0) = c G^2 / N, chi(k_1) = A G^2 / (2 N), xi from their ratio
    c, A = 2.0, 0.5
    chi, xi = ov.correlation_length(c + A * np.cos(2 * np.pi * dg / G), N)
    assert chi[0] == pytest.approx(c * G * G / N, rel=1e-12) and chi[1] == pytest.approx(A * G * G / (2 * N), rel=1e-12)
    assert xi == pytest.approx(np.sqrt(c / (A / 2) - 1.0) / (2 * np.sin(np.pi / G)), rel=1e-12)
    # the ratio below 1, and G = 1
    assert np.isnan(ov.correlation_length(0.1 + A * np.cos(2 * np.pi * dg / G), N)[1])
    chi1, xi1 = ov.correlation_length(np.array([[9.0]]), 3.0)
    assert chi1.tolist() == [3.0] and np.isnan(xi1)
    # G = 2: k_1 = pi
    chi2, xi2 = ov.correlation_length(np.array([[4.0, 1.0], [1.0, 4.0]]), 4.0)
    assert chi2 == pytest.approx([2.5, 1.5], rel=1e-12) and xi2 == pytest.approx(np.sqrt(2.5 / 1.5 - 1.0) / 2.0, rel=1e-12)


# ---------------------------------------------------------------------------------------------- 5. integers -> <Q_g Q_g'>
@pytest.mark.parametrize('kind', ['spin', 'cell'])
def test_pipeline_on_the_host(kind):
    """pack_groups, condense, quantise, the brute-force integers in place of the device call, second_moments: against the weighted
    means over all ordered pairs in float64, M = 200 with duplicates, integer and real weights."""
    rng = np.random.default_rng(12)
    M, G = 200, 5
    lanes16 = kind == 'cell'
    group = rng.permutation(np.repeat(np.arange(G), [7, 0, 70, 3, 9] if not lanes16 else [3, 0, 6, 1, 2]))
    pool = rng.integers(0, 300 if lanes16 else 2, (40, group.size))
    X = pool[rng.integers(0, 40, M)]
    X[M // 2:] = rng.integers(0, 300 if lanes16 else 2, (M - M // 2, group.size))
    sizes = np.bincount(group, minlength=G)
    for name, w in (('uniform', np.ones(M)), ('integer', rng.integers(0, 50, M).astype(np.float64)), ('real', 10.0 ** rng.uniform(-6, 0, M))):
        rows, wpg = ov.pack_groups(X, group, G, lanes16)
        wmax = ov.WMAX // ((4 if lanes16 else 64) * wpg)
        urows, W, D0 = ov.condense(rows, w)
        wq, keep, scale = ov.quantise(W, wmax)
        out = cref.pair_moments_ref(urows[keep], G, wpg, wq[keep], wmax, lanes16)
        mean, QQ = ov.second_moments(cref.limbs3(out), sizes, kind, scale, D0)
        ref = cref.correlations_ref(X, group, G, w, kind)
        K = urows.shape[0]
        tol = 1e-13 if name != 'real' else 2.0 * K / wmax              # exact integers; quantised weights as in DESIGN section 16
        nn = np.outer(sizes, sizes).astype(np.float64)
        ok = nn > 0
        assert (scale == 1.0) == (name != 'real')
        assert np.all(np.abs(QQ[ok] / nn[ok] - ref['C'][ok]) <= tol), name
        assert np.all(QQ[~ok] == 0)
        assert np.all(np.abs(mean[sizes > 0] / sizes[sizes > 0] - ref['mean'][sizes > 0]) <= tol), name
        assert np.allclose(ov.chi_of_k(QQ, sizes.sum()), cref.chi_ref(QQ, sizes.sum()), rtol=1e-12, atol=1e-12)


def test_second_moments_by_hand():
    """Two groups of 2 and 1 bits, rows 00|0 (weight 1), 11|0 (weight 2), 11|1 (weight 3): pairs (d_0, d_1; p) = (2, 0; 2), (2, 1; 3),
    (0, 1; 6)."""
    bits = np.array([[0, 0, 0], [1, 1, 0], [1, 1, 1]])
    rows, wpg = ov.pack_groups(bits, [0, 0, 1], 2, False)
    out = cref.pair_moments_ref(rows, 2, wpg, [1, 2, 3], None, False)
    assert out == [[20, 6, 10], [6, 9, 9], [10, 9, 11]]
    mean, QQ = ov.second_moments(cref.limbs3(out), [2, 1], 'spin')
    # Q_0 = 2 - 2 d_0, Q_1 = 1 - 2 d_1: (-2, 1), (-2, -1), (2, -1)
    assert np.array_equal(mean, np.array([-2 * 2 - 2 * 3 + 2 * 6, 2 - 3 - 6]) / 11.0)
    assert np.array_equal(QQ, np.array([[4 * 11, -4 + 6 - 12], [-4 + 6 - 12, 11]]) / 11.0)
    # a self term of 5 units with scale 1 enters as an integer: five more units of weight at Q = n
    mean5, QQ5 = ov.second_moments(cref.limbs3(out), [2, 1], 'spin', 1.0, 5.0)
    assert np.array_equal(QQ5, np.array([[4 * 16, -10 + 5 * 2], [-10 + 5 * 2, 16]]) / 16.0)
    # ... and as a float next to a scale
    _, QQs = ov.second_moments(cref.limbs3([[100 * v for v in r] for r in out]), [2, 1], 'spin', 10.0, 5.5)
    assert np.allclose(QQs, np.array([[4 * 16.5, -10 + 5.5 * 2], [-10 + 5.5 * 2, 16.5]]) / 16.5, rtol=1e-15, atol=1e-15)
    # 'cell': Q = n - d
    _, QQc = ov.second_moments(cref.limbs3(out), [2, 1], 'cell')
    assert np.array_equal(QQc, np.array([[0 * 2 + 0 * 3 + 4 * 6, 0 + 0 + 0], [0, 2]]) / 11.0)
    with pytest.raises(ValueError):
        ov.second_moments(np.zeros((3, 3, 2), dtype=np.uint64), [2, 1], 'spin')


# ---------------------------------------------------------------------------------------------- the public call refuses ...
def test_public_call_errors_before_any_device_work():
    s = droplet()
    with pytest.raises(ValueError):                                    # no states
        s.calculate_overlap_correlations()
    s.states = np.random.default_rng(4).integers(0, 256, (5, 16)).astype(s.indtype)
    for kw in (dict(kind='link'), dict(kind='bond'), dict(axis='z'), dict(weights='boltzmann'), dict(weights='importance'), dict(weights=np.ones(4))):
        with pytest.raises(ValueError):
            s.calculate_overlap_correlations(**kw)
    r = rmf()
    r.states = np.zeros((5, 9), dtype=r.indtype)
    for kind in ('spin', 'link'):
        with pytest.raises(ValueError):
            r.calculate_overlap_correlations(kind=kind)
    r.Nx_model = 65                                                    # a lattice of 65 columns
    with pytest.raises(NotImplementedError, match='64'):
        r.calculate_overlap_correlations()
    with pytest.raises(NotImplementedError, match='64'):
        r.calculate_overlap_correlations(axis='x')
    r.Nx_model, r.Ny_model = 129, 1                                    # one row of 129 cells: 33 words
    with pytest.raises(NotImplementedError, match='32'):
        r.calculate_overlap_correlations(axis='y')
    assert not hasattr(s, 'overlap_line_correlations') and not hasattr(r, 'overlap_chi')


# ---------------------------------------------------------------------------------------------- argument errors of the export
def test_pair_moments_argument_errors():
    """rc < 0 with a message and nothing launched: the pointers below are not device memory, they are never followed."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    p = 4096                                                           # stands for a non-null pointer
    M, G, wpg = 300, 16, 2
    wmax = (2 ** 32 - 1) // 128
    need = int(L.tn_pair_moments_ws_bytes(M, G, wpg, 0))
    assert need >= (G + 1) * (G + 2) // 2 * 16 and need % 16 == 0
    assert int(L.tn_pair_moments_ws_bytes(1, G, wpg, 0)) > 0           # M < 2 is a valid call
    for args in ((None, M, G, wpg, 32, None, wmax, 0, p, p, need, None), (p, M, G, wpg, 32, None, wmax, 0, None, p, need, None),
                 (p, M, G, wpg, 32, None, wmax, 0, p, None, need, None)):
        assert L.tn_pair_moments(*args) == -1
        assert 'null operand' in last_error(L)
    assert L.tn_pair_moments(p, M, G, wpg, 31, None, wmax, 0, p, p, need, None) == -1
    assert 'ldr' in last_error(L)
    assert L.tn_pair_moments(p, -1, G, wpg, 32, None, wmax, 0, p, p, need, None) == -1
    assert L.tn_pair_moments(p, 2 ** 31, G, wpg, 32, None, wmax, 0, p, p, need, None) == -1
    for bad_G in (0, 65):
        assert int(L.tn_pair_moments_ws_bytes(M, bad_G, wpg, 0)) == 0
        assert L.tn_pair_moments(p, M, bad_G, wpg, 4096, None, wmax, 0, p, p, 1 << 30, None) == -1
        assert '64' in last_error(L)
    assert int(L.tn_pair_moments_ws_bytes(M, G, 33, 0)) == 0
    assert L.tn_pair_moments(p, M, G, 33, 4096, None, 1, 0, p, p, 1 << 30, None) == -1
    assert '32' in last_error(L)
    assert L.tn_pair_moments(p, M, G, wpg, 32, None, 0, 0, p, p, need, None) == -1
    assert 'wmax' in last_error(L)
    for lanes16, dmax in ((0, 128), (1, 8)):                           # wmax dmax = 2^32 is one too many, 2^32 - dmax is the largest
        assert L.tn_pair_moments(p, M, G, wpg, 32, None, 2 ** 32 // dmax, lanes16, p, p, need, None) == -1
        assert '4294967295' in last_error(L)
        assert L.tn_pair_moments(p, M, G, wpg, 32, None, 2 ** 32 // dmax - 1, lanes16, p, p, need - 1, None) == -3
        assert 'workspace too small' in last_error(L)
