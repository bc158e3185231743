"""Host side of tnac4o.calculate_sample_correlations (tnac4o_amd/overlap.py), with the reference's integers in place of the device
call, and the argument errors of tn_spin_moments.  No GPU."""
import numpy as np
import pytest

import spin_moments_ref as sref
from overlap_ref import droplet, ising3x3, last_error, rmf
from tnac4o_amd import overlap as ov


def host_pipeline(bits, w):
    """sample_correlations without a solver and without a device: pack, condense, quantise, the reference's integers, estimators."""
    urows, W, _ = ov.condense(ov.pack_bits(bits), w)
    wq, keep, scale = ov.quantise(W, ov.WMAX)
    w = np.asarray(w, dtype=np.float64)
    out = sref.spin_moments_ref(urows[keep], bits.shape[1], wq[keep].astype(np.uint64), int(wq.max()))
    return ov.spin_estimators(out, float(np.sum(w * w)) * scale * scale, scale), urows.shape[0], scale


# ---------------------------------------------------------------------------------------------- 1. the reference itself
def test_reference_matches_the_definition():
    rows = sref.make_rows(9, 70, seed=3)
    for name, (w, wmax) in sref.weight_sets(9, seed=5).items():
        want = sref.spin_moments_slow(rows, 70, w, wmax)
        got = sref.spin_moments_ref(rows, 70, w, wmax)
        assert got.tolist() == want, name
    n = 70
    out = sref.spin_moments_ref(rows, n, *sref.weight_sets(9, seed=5)['random'])
    X = sref.bits_with_pseudo(rows, n)
    w = [int(v) for v in sref.weight_sets(9, seed=5)['random'][0]]
    assert out[n, n + 1] == sum(w) and out[n, n] == 0 and out[n + 1, n + 1] == 0
    for i in range(n):
        assert out[i, n] == sum(w[a] for a in range(9) if X[a, i]) and out[i, n] + out[i, n + 1] == sum(w)


def test_by_hand():
    """Three samples 00, 01, 11 with weights 1, 2, 3."""
    out = sref.spin_moments_ref(ov.pack_bits(np.array([[0, 0], [0, 1], [1, 1]])), 2, [1, 2, 3])
    assert out.tolist() == [[0, 2, 3, 3], [2, 0, 5, 1], [3, 5, 0, 6], [3, 1, 6, 0]]
    m, C, QQ = ov.spin_estimators(out, 1 + 4 + 9)
    assert np.array_equal(m, np.array([(3 - 3) / 6.0, (5 - 1) / 6.0]))             # sigma = +1 where the bit is 1
    assert np.array_equal(C, np.array([[1.0, 2 / 6.0], [2 / 6.0, 1.0]]))
    # pairs (a, b; p; q_0 q_1): (0, 1; 2; -1), (0, 2; 3; 1), (1, 2; 6; -1)
    assert np.array_equal(QQ, np.array([[1.0, (-2 + 3 - 6) / 11.0], [(-2 + 3 - 6) / 11.0, 1.0]]))
    with pytest.raises(ValueError, match='no pair of distinct samples'):
        ov.spin_estimators(sref.spin_moments_ref(ov.pack_bits(np.array([[0, 1]])), 2, [7]), 49)
    with pytest.raises(ValueError, match='no pair of distinct samples'):
        ov.spin_estimators(np.zeros((4, 4), dtype=np.int64), 0)
    with pytest.raises(ValueError):
        ov.spin_estimators(np.zeros((4, 5), dtype=np.int64), 0)


# ---------------------------------------------------------------------------------------------- 2. the pair identity, in integers
def test_pair_identity_in_integers():
    """(W - 2 D_ij)^2 - S2 = 2 sum_{a<b} w_a w_b q_i(ab) q_j(ab) and W^2 - S2 = 2 sum_{a<b} w_a w_b, exactly, for integer weights up to
    2^32 - 1 (the Python-integer branch of spin_estimators) and for small ones (the int64 branch)."""
    rng = np.random.default_rng(2)
    M, n = 40, 11
    bits = rng.integers(0, 2, (M, n))
    bits[7] = bits[3]
    for w in ([1] * M, rng.integers(0, 9, M).tolist(), rng.integers(0, 2 ** 32, M).tolist()):
        out = sref.spin_moments_ref(ov.pack_bits(bits), n, w)
        W, S2 = int(out[n, n + 1]), sum(int(v) ** 2 for v in w)
        assert W == sum(w)
        num, den = sref.pair_sums_int(bits, w)
        A = W - 2 * out[:n, :n]
        assert np.array_equal(A * A - S2, 2 * num) and W * W - S2 == 2 * den
        if S2 < 2 ** 53:
            _, _, QQ = ov.spin_estimators(out, float(S2))
            assert np.array_equal(QQ, (2 * num).astype(np.float64) / float(2 * den))
    # the two exact branches agree: the same integers below and, scaled by 2^31, above the int64 range
    out = sref.spin_moments_ref(ov.pack_bits(bits), n, [3] * M)
    big = out * 2 ** 31
    a, b = ov.spin_estimators(out, 9.0 * M), ov.spin_estimators(big, 9.0 * M * 2.0 ** 62)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- 3. estimators against all pairs
def test_estimators_against_all_pairs_of_samples():
    """M = 200 with duplicated rows through condense.  Uniform and integer weights: both sides are ratios of exactly representable
    integers.  Real weights over 6 decades: each quantised weight is off by half a unit at most and sum w_q >= wmax / 2, which bounds
    |dC| by 2 K / wmax and |d<q_i q_j>| by (K / wmax) (4 / (1 - s) + 2 s / (1 - s)^2), s = sum w^2 / (sum w)^2."""
    rng = np.random.default_rng(12)
    M, n = 200, 70
    pool = rng.integers(0, 2, (40, n))
    bits = pool[rng.integers(0, 40, M)]
    bits[M // 2:] = rng.integers(0, 2, (M - M // 2, n))
    for name, w in (('uniform', np.ones(M)), ('integer', rng.integers(0, 50, M).astype(np.float64)), ('real', 10.0 ** rng.uniform(-6, 0, M))):
        (m, C, QQ), K, scale = host_pipeline(bits, w)
        ref = sref.sample_ref(bits, w)
        assert K < M and (scale == 1.0) == (name != 'real')
        assert np.array_equal(C, C.T) and np.array_equal(QQ, QQ.T) and np.all(np.diag(C) == 1.0)
        if name != 'real':
            assert np.allclose(m, ref['m'], rtol=1e-13, atol=0.0), name
            assert np.allclose(C, ref['C'], rtol=1e-13, atol=0.0), name
            assert np.allclose(QQ, ref['QQ'], rtol=1e-13, atol=0.0), name
        else:
            s = float(np.sum(w * w) / w.sum() ** 2)
            d = K / float(ov.WMAX)
            assert np.max(np.abs(m - ref['m'])) <= 2 * d and np.max(np.abs(C - ref['C'])) <= 2 * d
            assert np.max(np.abs(QQ - ref['QQ'])) <= d * (4 / (1 - s) + 2 * s / (1 - s) ** 2)
            assert np.allclose(np.diag(QQ), 1.0, rtol=1e-13, atol=0.0)


# ---------------------------------------------------------------------------------------------- 4. chi on the grid of wave vectors
def test_chi_2d_against_loops_and_line_sums():
    s = droplet()
    rng = np.random.default_rng(7)
    gx, gy = ov.line_groups(s, 'x', 'spin')[0], ov.line_groups(s, 'y', 'spin')[0]
    bits = rng.integers(0, 2, (50, 128))
    bits[:, :40] = bits[:, :1]                                         # correlated spins: something at k != 0
    (_, _, QQ), _, _ = host_pipeline(bits, np.ones(50))
    chi = ov.chi_sg_2d(QQ, gx, gy, 4, 4)
    ref = sref.chi2d_ref(QQ, gx, gy, 4, 4)
    assert chi.shape == (4, 4) and np.allclose(chi, ref, rtol=0.0, atol=1e-12 * ref[0, 0])
    assert chi[0, 0] == pytest.approx(QQ.sum() / 128.0, rel=1e-13)
    for mx in range(4):
        for my in range(4):
            assert chi[mx, my] == chi[-mx % 4, -my % 4]
    # chi(m, 0) and chi(0, m) are chi_of_k of the line sums
    for ax, g in (('x', gx), ('y', gy)):
        Z = np.zeros((128, 4))
        Z[np.arange(128), g] = 1.0
        line = ov.chi_of_k(Z.T @ QQ @ Z, 128)
        got = chi[:3, 0] if ax == 'x' else chi[0, :3]
        assert np.allclose(got, line, rtol=0.0, atol=1e-12 * chi[0, 0]), ax
    # closed forms: everything correlated sits at k = 0; a plane wave along x sits at its own wave vector and the opposite one
    one = ov.chi_sg_2d(np.ones((128, 128)), gx, gy, 4, 4)
    assert one[0, 0] == pytest.approx(128.0, rel=1e-13) and np.all(np.abs(one.ravel()[1:]) <= 1e-12 * 128.0)
    dx = gx[:, None] - gx[None, :]
    wave = ov.chi_sg_2d(np.cos(2 * np.pi * dx / 4), gx, gy, 4, 4)
    want = np.zeros((4, 4))
    want[1, 0] = want[3, 0] = 128.0 / 2                                # 32 spins per column: (1 / N) (N^2 / 2)
    assert np.allclose(wave, want, rtol=0.0, atol=1e-11)
    # an uneven lattice: 3 x 3 with 6, 5, 6 spins per line
    t = ising3x3()
    gx3, gy3 = ov.line_groups(t, 'x', 'spin')[0], ov.line_groups(t, 'y', 'spin')[0]
    (_, _, Q3), _, _ = host_pipeline(rng.integers(0, 2, (30, 17)), np.ones(30))
    assert np.allclose(ov.chi_sg_2d(Q3, gx3, gy3, 3, 3), sref.chi2d_ref(Q3, gx3, gy3, 3, 3), rtol=0.0, atol=1e-12 * Q3.sum() / 17)


# ---------------------------------------------------------------------------------------------- 5. the public call refuses ...
STORED = ('sample_spins', 'sample_magnetization', 'sample_correlations', 'sample_overlap_correlations', 'sample_chi_sg')


def test_public_call_errors_before_any_device_work():
    s = droplet()
    with pytest.raises(ValueError):                                    # no states
        s.calculate_sample_correlations()
    s.states = np.random.default_rng(4).integers(0, 256, (5, 16)).astype(s.indtype)
    for weights in ('boltzmann', 'importance', np.ones(4), -np.ones(5), np.zeros(5), np.array([1, np.nan, 1, 1, 1]), [1, 'a', 1, 1, 1]):
        with pytest.raises(ValueError):
            s.calculate_sample_correlations(weights=weights)
    with pytest.raises(ValueError, match='no pair of distinct samples'):                 # one sample carries all the weight
        s.calculate_sample_correlations(weights=np.array([0.0, 0.0, 2.5, 0.0, 0.0]))
    with pytest.raises(ValueError, match='no pair of distinct samples'):                 # ... up to the rounding of the weights
        s.calculate_sample_correlations(weights=np.array([0.0, 1e-30, 2.5, 0.0, 0.0]))
    r = rmf()
    r.states = np.zeros((5, 9), dtype=r.indtype)
    with pytest.raises(ValueError, match='Ising'):
        r.calculate_sample_correlations()
    assert not any(hasattr(s, a) or hasattr(r, a) for a in STORED) and not hasattr(s, 'overlap_ess')


def test_ops_wrapper_refuses_before_the_library_call():
    import torch
    from tnac4o_amd import ops
    with pytest.raises(RuntimeError, match='GPU tensors only'):
        ops.spin_moments(torch.zeros((4, 2), dtype=torch.int64), 70)


# ---------------------------------------------------------------------------------------------- argument errors of the export
def test_spin_moments_argument_errors(monkeypatch):
    """rc < 0 with a message and nothing launched: the pointers below are not device memory, they are never followed."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv('TN_SPIN_MOMENTS_WGS', raising=False)
    p = 4096                                                           # stands for a non-null pointer
    M, n, wmax = 2565, 70, 2 ** 32 - 1
    need = int(L.tn_spin_moments_ws_bytes(M, n, wmax))
    KW, NB = -(-M // 64), 2
    assert need >= 8 * (NB * 64 * KW + 32 * KW) and need % 8 == 0      # the transpose and the planes at least
    assert int(L.tn_spin_moments_ws_bytes(0, n, wmax)) > 0             # M = 0 is a valid call
    assert int(L.tn_spin_moments_ws_bytes(M, n, 1)) < need             # one plane instead of 32
    monkeypatch.setenv('TN_SPIN_MOMENTS_WGS', '1')                     # one workgroup: every tile whole, no slabs
    assert int(L.tn_spin_moments_ws_bytes(M, n, wmax)) == 8 * (NB * 64 * KW + 32 * KW) < need
    monkeypatch.setenv('TN_SPIN_MOMENTS_WGS', '4')                     # two slabs of 4096 sums per workgroup
    assert int(L.tn_spin_moments_ws_bytes(M, n, wmax)) == 8 * (NB * 64 * KW + 32 * KW + 2 * 4 * 4096)
    monkeypatch.delenv('TN_SPIN_MOMENTS_WGS', raising=False)
    for args in ((None, M, n, 2, None, wmax, p, n + 2, p, need, None), (p, M, n, 2, None, wmax, None, n + 2, p, need, None),
                 (p, M, n, 2, None, wmax, p, n + 2, None, need, None)):
        assert L.tn_spin_moments(*args) == -1
        assert 'null operand' in last_error(L)
    assert L.tn_spin_moments(p, M, n, 1, None, wmax, p, n + 2, p, need, None) == -1
    assert 'ldr' in last_error(L)
    assert L.tn_spin_moments(p, M, n, 2, None, wmax, p, n + 1, p, need, None) == -1
    assert 'ldo' in last_error(L)
    for bad_M in (-1, 2 ** 32):
        assert int(L.tn_spin_moments_ws_bytes(bad_M, n, wmax)) == 0
        assert L.tn_spin_moments(p, bad_M, n, 2, None, wmax, p, n + 2, p, 1 << 40, None) == -1
        assert '4294967296' in last_error(L)
    for bad_n in (0, 65535):
        assert int(L.tn_spin_moments_ws_bytes(M, bad_n, wmax)) == 0
        assert L.tn_spin_moments(p, M, bad_n, 1024, None, wmax, p, 65537, p, 1 << 40, None) == -1
        assert '65534' in last_error(L)
    assert int(L.tn_spin_moments_ws_bytes(M, n, 0)) == 0
    assert L.tn_spin_moments(p, M, n, 2, None, 0, p, n + 2, p, need, None) == -1
    assert 'wmax' in last_error(L)
    assert L.tn_spin_moments(p, M, n, 2, None, wmax, p, n + 2, p, need - 1, None) == -3
    assert 'workspace too small' in last_error(L)
