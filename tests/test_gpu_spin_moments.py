"""tn_spin_moments and tnac4o.calculate_sample_correlations on the GPU: the kernel against brute force in Python integers, its ties to
tn_pair_hist and tn_pair_moments, independence of the grid, the workspace and output contract, the host pipeline against loops over
the samples and over all pairs of samples in float64 and against the existing public calls, and the correlations of
sample_boltzmann's samples against the enumerated law."""
import math

import numpy as np
import pytest

import overlap_corr_ref as cref
import spin_moments_ref as sref
from guarded import Guarded
from overlap_ref import WMAX, droplet, first_diffs, last_error, states_with_duplicates

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

MS = (1, 2, 63, 64, 65, 300)
NBITS = (1, 2, 62, 63, 64, 65, 130)
WGS = ('1', '2', '3', '4', '7', None)


def run(rows, nbits, w, wmax):
    """ops.spin_moments on host arrays (rows as a strided view of the padded array) -> (nbits + 2, nbits + 2) Python integers."""
    from tnac4o_amd import ops
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    d_w = None if w is None else torch.as_tensor(np.asarray(w, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    out = ops.spin_moments(d_rows[:, :-(-nbits // 64)], nbits, d_w, wmax)
    assert out.shape == (nbits + 2, nbits + 2) and out.dtype == torch.int64
    return sref.to_ints(out.cpu().numpy())


def check_properties(got, nbits, total):
    n = nbits
    assert np.array_equal(got, got.T) and not np.diag(got).any()
    assert got[n, n + 1] == total
    assert all(got[i, n] + got[i, n + 1] == total for i in range(n))


def check_exact(M, nbits):
    rows = sref.make_rows(M, nbits, seed=1000 * M + nbits)
    assert rows.shape[1] == -(-nbits // 64) + sref.PAD
    for name, (w, wmax) in sref.weight_sets(M, seed=M + nbits).items():
        want = sref.spin_moments_ref(rows, nbits, w, wmax)
        got = run(rows, nbits, w, wmax)
        assert np.array_equal(got, want), (name, first_diffs(got, want))
        check_properties(got, nbits, M if w is None else sum(min(int(v), wmax) for v in w))


# ---------------------------------------------------------------------------------------------- 1. kernel against brute force
@pytest.mark.parametrize('nbits', NBITS)
@pytest.mark.parametrize('M', MS)
def test_spin_moments_is_exact(M, nbits):
    check_exact(M, nbits)


def test_one_word_passes_32_bits():
    """M = 128, two complementary columns, every weight 2^32 - 1: each word of 64 samples adds 64 (2^32 - 1) > 2^38 to one entry."""
    M = 128
    bits = np.zeros((M, 2), dtype=np.int64)
    bits[:, 0] = np.random.default_rng(1).integers(0, 2, M)
    bits[:, 1] = 1 - bits[:, 0]
    from tnac4o_amd import overlap
    got = run(overlap.pack_bits(bits), 2, np.full(M, WMAX, dtype=np.uint64), WMAX)
    assert got[0, 1] == got[1, 0] == 128 * WMAX and got[2, 3] == 128 * WMAX
    assert got[0, 2] == int(bits[:, 0].sum()) * WMAX and got[0, 3] == got[1, 2]
    check_properties(got, 2, 128 * WMAX)


# ---------------------------------------------------------------------------------------------- 2. ties to the sibling kernels
def test_ties_to_pair_hist_and_pair_moments():
    """With n1_i = out[i][n], n0_i = out[i][n+1]: sum_i n1_i n0_i is the first moment of tn_pair_hist's histogram of the same bits, and
    sum_{i,j} (n11 n00 + n10 n01)_ij -- the weight of the pairs of samples that differ in both spins -- its second moment, which is
    also the sum of tn_pair_moments' second moments of the grouped bits.  Python integers."""
    from tnac4o_amd import ops, overlap
    rng = np.random.default_rng(21)
    M, n, G = 300, 150, 7
    group = rng.permutation(np.repeat(np.arange(G), [5, 0, 70, 1, 34, 9, 31]))
    X = rng.integers(0, 2, (M, n))
    X[1] = X[0]
    grows, wpg = overlap.pack_groups(X, group, G, False)
    dense = overlap.pack_bits(X)
    wmax = cref.wmax_of(wpg, False)
    for name, w in cref.weight_sets(M, wmax, seed=4).items():
        d_w = None if w is None else torch.as_tensor(w.astype(np.uint32).view(np.int32)).cuda()
        d_dense = torch.as_tensor(dense.view(np.int64)).cuda()
        hist = overlap.limbs_to_int(ops.pair_hist(d_dense, n, d_w, False).cpu().numpy())
        pm = overlap.limbs_to_int(ops.pair_moments(torch.as_tensor(grows.view(np.int64)).cuda(), G, wpg, d_w, wmax, False).cpu().numpy().reshape(-1, 2))
        pm = [pm[i * (G + 1):(i + 1) * (G + 1)] for i in range(G + 1)]
        out = run(dense, n, w, wmax if w is not None else 1)
        W = out[n, n + 1]
        n1 = out[:n, n]
        assert sum(n1[i] * out[i, n + 1] for i in range(n)) == sum(d * h for d, h in enumerate(hist)), name
        twice = n1[:, None] + n1[None, :] - out[:n, :n]
        assert not (twice % 2).any(), name
        n11 = twice // 2
        n10, n01 = n1[:, None] - n11, n1[None, :] - n11
        n00 = W - n11 - n10 - n01
        both = int((n11 * n00 + n10 * n01).sum())
        assert both == sum(d * d * h for d, h in enumerate(hist)), name
        assert both == sum(pm[g][k] for g in range(G) for k in range(G)), name
        assert W * W - sum(min(int(v), wmax) ** 2 for v in (w if w is not None else [1] * M)) == 2 * sum(hist) == 2 * pm[G][G], name
        assert W > 0


# ---------------------------------------------------------------------------------------------- 3. independence of the grid
def test_result_does_not_depend_on_the_grid(monkeypatch):
    """TN_SPIN_MOMENTS_WGS = 1, 2, 3, 4, 7 and unset.  M = 2565, n = 70 has 3 tiles of 3 chunks of 16 words, 9 units: one workgroup and
    three hold whole tiles only; two cut the middle tile (the last piece of one share, the first of the next); four and seven cut
    tiles into two and three pieces, with shares that lie inside one tile; unset gives every unit its own workgroup."""
    cases = [(sref.make_rows(M, nbits, seed=7 * M + nbits), nbits) for M in MS for nbits in NBITS]
    cases.append((sref.make_rows(2565, 70, seed=5), 70))
    same = sref.make_rows(300, 130, seed=9)
    same[:] = same[0]
    cases.append((same, 130))                                          # 300 identical rows
    for rows, nbits in cases:
        M = rows.shape[0]
        sets = sref.weight_sets(M, seed=nbits)
        names = ('none', 'random', 'clamp5', 'max') if M < 2000 else tuple(sets)
        for name in names:
            w, wmax = sets[name]
            out = {}
            for wgs in WGS:
                if wgs is None:
                    monkeypatch.delenv('TN_SPIN_MOMENTS_WGS', raising=False)
                else:
                    monkeypatch.setenv('TN_SPIN_MOMENTS_WGS', wgs)
                out[wgs] = run(rows, nbits, w, wmax)
            assert all(np.array_equal(out[k], out[None]) for k in WGS), (M, nbits, name)
            if M > 2000:
                assert np.array_equal(out[None], sref.spin_moments_ref(rows, nbits, w, wmax)), name
            if rows is same and name == 'max':
                X = sref.bits_with_pseudo(rows[:1], nbits)[0]
                assert np.array_equal(out[None], (X[:, None] != X[None, :]).astype(object) * (300 * WMAX))
    monkeypatch.delenv('TN_SPIN_MOMENTS_WGS', raising=False)


# ---------------------------------------------------------------------------------------------- 4. workspace and output contract
@pytest.mark.parametrize('M,nbits', [(300, 130), (2565, 70)])
def test_workspace_and_output_contract(M, nbits, monkeypatch):
    """Exactly tn_spin_moments_ws_bytes suffices whatever the workspace and the output held before; every entry of out is written and,
    with ldo > n + 2, nothing beyond column n + 1; the guards stay intact; one byte less is -3 and a shape outside the limits -1 with
    the limit in the message, and then nothing is written; M = 0 gives zeros."""
    from tnac4o_amd import _lib, ops
    monkeypatch.delenv('TN_SPIN_MOMENTS_WGS', raising=False)
    L = _lib.lib()
    rows = sref.make_rows(M, nbits, seed=31)
    ld, n2 = rows.shape[1], nbits + 2
    w, wmax = sref.weight_sets(M, seed=3)['random']
    want = sref.spin_moments_ref(rows, nbits, w, wmax)
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    d_w = torch.as_tensor(w.astype(np.uint32).view(np.int32)).cuda()
    need = int(L.tn_spin_moments_ws_bytes(M, nbits, wmax))
    assert need > 0
    if M > 2000:                                                       # 9 units, a workgroup each: slabs behind the transpose
        assert need > 8 * (2 * 64 + 32) * -(-M // 64)
    for fill in (0xFF, 'random'):
        for ldo in (n2, n2 + 5):
            ws = Guarded(need, fill, seed=1)
            out = Guarded.of(torch.int64, (n2, ldo), 0xFF if ldo > n2 else fill, seed=2)
            rc = L.tn_spin_moments(d_rows.data_ptr(), M, nbits, ld, d_w.data_ptr(), wmax, out.ptr, ldo, ws.ptr, need, ops._stream())
            torch.cuda.synchronize()
            assert rc == 0
            assert ws.intact() and out.intact()
            host = out.host()
            assert np.array_equal(sref.to_ints(host[:, :n2]), want)   # every entry holds its value
            assert np.all(host[:, n2:] == -1)                          # the columns beyond are untouched
    ws = Guarded(need - 1, 0xFF, seed=3)
    out = Guarded.of(torch.int64, (n2, n2), 0xFF, seed=4)
    rc = L.tn_spin_moments(d_rows.data_ptr(), M, nbits, ld, d_w.data_ptr(), wmax, out.ptr, n2, ws.ptr, need - 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == -3
    assert ws.untouched(0xFF) and out.untouched(0xFF) and ws.intact() and out.intact()
    # outside the limits: -1, the limit in the message, nothing written
    big = Guarded(1 << 20, 0xFF, seed=7)
    for (m, n, wm, ldr, ldo), word in (((2 ** 32, nbits, wmax, ld, n2), '4294967296'), ((-1, nbits, wmax, ld, n2), '4294967296'),
                                       ((M, 0, wmax, ld, n2), '65534'), ((M, 65535, wmax, 1024, 65537), '65534'), ((M, nbits, 0, ld, n2), 'wmax'),
                                       ((M, nbits, wmax, -(-nbits // 64) - 1, n2), 'ldr'), ((M, nbits, wmax, ld, n2 - 1), 'ldo')):
        out = Guarded.of(torch.int64, (n2, n2), 0xFF, seed=8)
        rc = L.tn_spin_moments(d_rows.data_ptr(), m, n, ldr, d_w.data_ptr(), wm, out.ptr, ldo, big.ptr, big.nbytes, ops._stream())
        torch.cuda.synchronize()
        assert rc == -1 and word in last_error(L), (m, n, wm, ldr, ldo, last_error(L))
        assert out.untouched(0xFF) and big.untouched(0xFF) and out.intact() and big.intact()
    # M = 0: zeros in every entry
    out = Guarded.of(torch.int64, (n2, n2), 0xFF, seed=5)
    ws = Guarded(int(L.tn_spin_moments_ws_bytes(0, nbits, wmax)), 0xFF, seed=6)
    assert L.tn_spin_moments(d_rows.data_ptr(), 0, nbits, ld, None, wmax, out.ptr, n2, ws.ptr, ws.nbytes, ops._stream()) == 0
    torch.cuda.synchronize()
    assert not out.host().any() and out.intact() and ws.intact()


# ---------------------------------------------------------------------------------------------- 5. pipeline, uniform weights
STORED = ('sample_spins', 'sample_magnetization', 'sample_correlations', 'sample_overlap_correlations', 'sample_chi_sg', 'overlap_ess')


def test_pipeline_uniform_weights():
    """Uniform weights on 2048 states with 60 distinct rows: the device part is an exact count and both sides are ratios of integers
    below 2^53, so m, C and <q_i q_j> agree with the loops to the rounding of a division; and the sums of <q_i q_j> over lattice lines,
    its mean and its transform are what calculate_overlap_correlations and calculate_overlap_distribution give on the same states."""
    from tnac4o_amd import overlap
    M = 2048
    rng = np.random.default_rng(11)
    s = droplet()
    s.states = states_with_duplicates(M, rng, 60).astype(np.uint8).astype(s.indtype)
    s.calculate_overlap_distribution('spin')
    s.calculate_overlap_correlations('both', 'spin')
    C = s.calculate_sample_correlations()
    bits = overlap.spin_bits(s)
    assert np.unique(bits, axis=0).shape[0] <= 60 and bits.shape == (M, 128)
    assert C is s.sample_correlations and C.shape == (128, 128) and s.sample_magnetization.shape == (128,)
    assert np.array_equal(s.sample_spins, np.arange(128)) and s.overlap_ess == pytest.approx(2048.0, rel=1e-12)
    ref = sref.sample_ref(bits, np.ones(M), pairs=False)
    for name, got, want in (('m', s.sample_magnetization, ref['m']), ('C', C, ref['C'])):
        err = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
        print('uniform, %s: largest relative deviation %.2e' % (name, err))
        assert np.allclose(got, want, rtol=1e-13, atol=0.0), name
    assert np.all(np.diag(C) == 1.0) and np.array_equal(C, C.T)
    # <q_i q_j> against all pairs of a subset of 256 samples
    t = droplet()
    t.states = s.states[:256]
    t.calculate_sample_correlations()
    want = sref.sample_ref(bits[:256], np.ones(256))['QQ']
    print('uniform, <q_i q_j> (M = 256): largest deviation %.2e' % np.max(np.abs(t.sample_overlap_correlations - want)))
    assert np.allclose(t.sample_overlap_correlations, want, rtol=1e-13, atol=0.0)
    # against the existing public calls on the same states
    QQ = s.sample_overlap_correlations
    assert QQ.shape == (128, 128) and np.array_equal(QQ, QQ.T) and np.all(np.diag(QQ) == 1.0)
    for ax in ('x', 'y'):
        group, sizes = overlap.line_groups(s, ax, 'spin')
        line = np.array([[math.fsum(QQ[np.ix_(group == g, group == h)].ravel()) for h in range(4)] for g in range(4)])
        want = s.overlap_line_correlations[ax] * np.outer(sizes, sizes)
        print('axis %s: line sums of <q_i q_j>, largest relative deviation %.2e' % (ax, np.max(np.abs(line - want) / np.abs(want))))
        assert np.allclose(line, want, rtol=1e-12, atol=0.0)
    q2 = math.fsum(QQ.ravel()) / 128.0 ** 2
    print('mean <q_i q_j> %.15f, <q^2> %.15f' % (q2, s.overlap_moments['q2']))
    assert q2 == pytest.approx(s.overlap_moments['q2'], rel=1e-12)
    chi = s.sample_chi_sg
    assert chi.shape == (4, 4) and chi[0, 0] == pytest.approx(s.overlap_moments['chi_sg'], rel=1e-12)
    print('chi_SG(kx, ky):\n%s' % chi)
    assert np.allclose(chi[:3, 0], s.overlap_chi['x'], rtol=0.0, atol=1e-12 * chi[0, 0])
    assert np.allclose(chi[0, :3], s.overlap_chi['y'], rtol=0.0, atol=1e-12 * chi[0, 0])
    gx, gy = overlap.line_groups(s, 'x', 'spin')[0], overlap.line_groups(s, 'y', 'spin')[0]
    assert np.allclose(chi, sref.chi2d_ref(QQ, gx, gy, 4, 4), rtol=0.0, atol=1e-12 * chi[0, 0])
    # a refusal leaves what is stored as it is
    before = {a: getattr(s, a) for a in STORED}
    with pytest.raises(ValueError):
        s.calculate_sample_correlations(weights=np.ones(3))
    assert all(getattr(s, a) is before[a] for a in STORED)


# ---------------------------------------------------------------------------------------------- 6. float weights over 12 decades
def test_pipeline_float_weights():
    """Weights over 12 orders of magnitude on more than 300 distinct rows.  Each of the K quantised weights is off by at most half a
    unit and sum w_q >= wmax / 2, wmax = 2^32 - 1, so a weighted mean of values in [-1, 1] moves by at most 2 K / wmax: |dm|, |dC|.
    <q_i q_j> = (C^2 - s) / (1 - s) with s = sum w^2 / (sum w)^2, whose relative error is at most 2 K / wmax:
    |d<q_i q_j>| <= (K / wmax) (4 / (1 - s) + 2 s / (1 - s)^2) (4 K / wmax as s -> 0)."""
    from tnac4o_amd import overlap
    M = 1024
    rng = np.random.default_rng(12)
    s = droplet()
    s.states = states_with_duplicates(M, rng, 700).astype(np.uint8).astype(s.indtype)
    w = 10.0 ** rng.uniform(-12.0, 0.0, M)
    C = s.calculate_sample_correlations(weights=w)
    bits = overlap.spin_bits(s)
    K = np.unique(bits, axis=0).shape[0]
    assert K > 300
    ref = sref.sample_ref(bits, w)
    ss = float(np.sum(w * w) / w.sum() ** 2)
    d = K / float(WMAX)
    bound_q = d * (4.0 / (1.0 - ss) + 2.0 * ss / (1.0 - ss) ** 2)
    em, ec = float(np.max(np.abs(s.sample_magnetization - ref['m']))), float(np.max(np.abs(C - ref['C'])))
    eq = float(np.max(np.abs(s.sample_overlap_correlations - ref['QQ'])))
    print('float weights: %d distinct rows, s = %.3e; largest deviation of m %.2e, of C %.2e (bound %.2e), of <q_i q_j> %.2e (bound %.2e)'
          % (K, ss, em, ec, 2 * d, eq, bound_q))
    assert em <= 2 * d and ec <= 2 * d
    assert eq <= bound_q
    assert s.overlap_ess == pytest.approx(1.0 / ss, rel=1e-12)


# ---------------------------------------------------------------------------------------------- 7. end to end, exact law
def test_correlations_of_boltzmann_samples():
    """ising_3x3_nc2 at beta = 1, 2^14 samples of an exact contraction (q = p): every <s_i s_j> (136 pairs) and every m_i within 5 sigma
    of the enumerated law, sigma^2 = (1 - exact^2) / M, the variance of the mean of M independent +-1; the same against
    calculate_marginals and, on the couplings, calculate_correlations (which fixes the sign convention)."""
    import marginals_ref as mr
    import tnac4o_amd
    M, beta = 2 ** 14, 1.0
    J = mr.ising_3x3_nc2()
    act = [i for i in range(18) if i != 9]                            # spin 9 has no term: it is not part of the law
    m_ex, C_ex, _ = sref.exact_spin_law(J, beta, 18, act)
    thermal = tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=J, beta=beta)
    thermal.calculate_marginals(Dmax=64)
    thermal.calculate_correlations(Dmax=64)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=J, beta=beta)
    np.random.seed(20241018)
    ins.sample_boltzmann(M=M, Dmax=64)
    C = ins.calculate_sample_correlations()
    m = ins.sample_magnetization
    assert ins.sample_spins.tolist() == act and C.shape == (17, 17) and ins.sample_chi_sg.shape == (3, 3)
    assert ins.overlap_ess == pytest.approx(M, rel=1e-12)
    worst = 0.0
    for i in range(17):
        sig = np.sqrt((1.0 - m_ex[i] ** 2) / M)
        worst = max(worst, abs(m[i] - m_ex[i]) / sig)
        assert abs(m[i] - m_ex[i]) <= 5.0 * sig, (i, m[i], m_ex[i])
        assert abs(m[i] - thermal.magnetization[act[i]]) <= 5.0 * sig, (i, m[i], thermal.magnetization[act[i]])
        for j in range(i + 1, 17):
            sig = np.sqrt((1.0 - C_ex[i, j] ** 2) / M)
            worst = max(worst, abs(C[i, j] - C_ex[i, j]) / sig)
            assert abs(C[i, j] - C_ex[i, j]) <= 5.0 * sig, (i, j, C[i, j], C_ex[i, j])
    print('136 pairs and 17 magnetisations: the largest deviation from the enumerated law is %.2f sigma' % worst)
    pos = {spin: k for k, spin in enumerate(act)}
    assert len(thermal.bond_pairs) > 0
    for (i, j), c in zip(thermal.bond_pairs, thermal.correlations):
        sig = np.sqrt((1.0 - c * c) / M)
        assert abs(C[pos[int(i)], pos[int(j)]] - c) <= 5.0 * sig, (i, j, C[pos[int(i)], pos[int(j)]], c)
    # <q_i q_j> estimates <s_i s_j>^2 without bias; its mean over i, j is <q^2> of the overlap distribution of the same samples
    ins.calculate_overlap_distribution('spin')
    assert math.fsum(ins.sample_overlap_correlations.ravel()) / 17.0 ** 2 == pytest.approx(ins.overlap_moments['q2'], rel=1e-12)
    # the contraction is exact: the importance weights are equal up to rounding
    QQ = ins.sample_overlap_correlations
    Ci = ins.calculate_sample_correlations(weights='importance')
    assert float(np.max(np.abs(Ci - C))) <= 1e-9 and float(np.max(np.abs(ins.sample_magnetization - m))) <= 1e-9
    assert float(np.max(np.abs(ins.sample_overlap_correlations - QQ))) <= 1e-9


# ---------------------------------------------------------------------------------------------- 8. RMF
def test_rmf_is_refused():
    import tnac4o_amd
    from tnac4o_amd import auxx
    ins = tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=3, J=auxx.synthetic_rmf(3, 3, 3, 17), beta=1.0)
    np.random.seed(5)
    ins.sample_boltzmann(M=64, Dmax=64)
    ins.sample_correlations = marker = object()
    with pytest.raises(ValueError, match='Ising'):
        ins.calculate_sample_correlations()
    assert ins.sample_correlations is marker
    assert not any(hasattr(ins, a) for a in STORED if a != 'sample_correlations')
