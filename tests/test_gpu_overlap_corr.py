"""tn_pair_moments and tnac4o.calculate_overlap_correlations on the GPU: the kernel against brute force in Python integers (both limbs
of every entry, exactly), its ties to tn_pair_hist, independence of the grid, the workspace and output contract, the host pipeline
against all M^2 pairs in float64, and the line overlaps of sample_boltzmann's samples against the exact two-replica law."""
import numpy as np
import pytest

import overlap_corr_ref as cref
from guarded import Guarded
from overlap_ref import droplet, first_diffs, last_error, source, states_with_duplicates

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

MS = (1, 2, 31, 32, 33, 65, 300)
SHAPES = ((1, 1), (2, 1), (3, 2), (16, 2), (17, 1), (64, 1), (5, 32))          # (G, wpg)
# the kernel deals 3 of its (element, slice of the pairs) units to a thread while (G+1)(G+2)/2 <= 384, that is G <= 26, and 9 above:
# both sides of that step, and of the steps in the number of slices 3 -> 2 (G = 21 -> 22) and 2 -> 1 (G = 46 -> 47)
CLASS_SHAPES = ((21, 1), (22, 1), (26, 1), (27, 1), (32, 2), (46, 1), (47, 1))

def to_ints(out):
    from tnac4o_amd import overlap
    n = out.shape[0]
    flat = overlap.limbs_to_int(out.cpu().numpy().reshape(-1, 2))
    return [flat[i * n:(i + 1) * n] for i in range(n)]


def run(rows, G, wpg, w, wmax, lanes16):
    """ops.pair_moments on host arrays (rows as a strided view of the padded array) -> nested Python integers."""
    from tnac4o_amd import ops
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    d_w = None if w is None else torch.as_tensor(np.asarray(w, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    out = ops.pair_moments(d_rows[:, :G * wpg], G, wpg, d_w, wmax, lanes16)
    assert out.shape == (G + 1, G + 1, 2) and out.dtype == torch.int64
    return to_ints(out)


def check_exact(M, G, wpg, lanes16):
    rows = cref.make_group_rows(M, G, wpg, lanes16, seed=1000 * M + 10 * G + wpg)
    assert rows.shape[1] == G * wpg + 3
    D = cref.group_dists(rows, G, wpg, lanes16)
    wmax = cref.wmax_of(wpg, lanes16)
    if M >= 3:
        assert np.all(D[:, 0, M - 1] == cref.dmax_of(wpg, lanes16)) and not D[:, 0, 1].any()
    want = None
    for name, w in cref.weight_sets(M, wmax, seed=M + G).items():
        want = cref.pair_moments_ref(rows, G, wpg, w, wmax, lanes16, dist=D)
        got = run(rows, G, wpg, w, wmax, lanes16)
        assert got == want, (name, first_diffs(got, want))
        assert all(got[i][j] == got[j][i] for i in range(G + 1) for j in range(i))
        if name == 'max' and M == 300:                                 # the carry: some entry needs the high limb
            assert max(max(r) for r in want) > 2 ** 64
    if M < 2:
        assert not any(any(r) for r in want)
    # a weight above wmax is read as wmax
    w = cref.weight_sets(M, wmax, seed=M + G)['random']
    over = w.copy()
    over[::3] = np.minimum(wmax + 1 + np.arange(over[::3].size, dtype=np.uint64) * np.uint64(977), np.uint64(2 ** 32 - 1))
    clipped = np.minimum(over, np.uint64(wmax))
    got = run(rows, G, wpg, over, wmax, lanes16)
    assert got == run(rows, G, wpg, clipped, wmax, lanes16)
    assert got == cref.pair_moments_ref(rows, G, wpg, clipped, wmax, lanes16, dist=D)


# ---------------------------------------------------------------------------------------------- 1. kernel against brute force
@pytest.mark.parametrize('lanes16', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('M', MS)
def test_pair_moments_is_exact(M, shape, lanes16):
    check_exact(M, shape[0], shape[1], lanes16)


@pytest.mark.parametrize('lanes16', [False, True])
@pytest.mark.parametrize('shape', CLASS_SHAPES)
def test_pair_moments_is_exact_in_every_element_class(shape, lanes16):
    check_exact(65, shape[0], shape[1], lanes16)


# ---------------------------------------------------------------------------------------------- 2. ties to tn_pair_hist
@pytest.mark.parametrize('lanes16', [False, True])
def test_moments_of_the_total_distance_match_pair_hist(lanes16):
    """The total distance is the sum of the group distances: the zeroth, first and second moment of tn_pair_hist's histogram of the
    same bits, packed densely, are out[G][G], sum_g out[g][G] and sum_{g,g'} out[g][g'].  Integers."""
    from tnac4o_amd import ops, overlap
    rng = np.random.default_rng(21)
    M, G = 300, 7
    group = rng.permutation(np.repeat(np.arange(G), [5, 0, 70, 1, 64, 9, 30] if not lanes16 else [5, 0, 7, 1, 4, 9, 3]))
    n = group.size
    X = rng.integers(0, 2 if not lanes16 else 5, (M, n))
    X[1] = X[0]
    grows, wpg = overlap.pack_groups(X, group, G, lanes16)
    dense = overlap.pack_lanes16(X) if lanes16 else overlap.pack_bits(X)
    wmax = cref.wmax_of(wpg, lanes16)
    for name, w in cref.weight_sets(M, wmax, seed=4).items():
        d_w = None if w is None else torch.as_tensor(w.astype(np.uint32).view(np.int32)).cuda()
        hist = overlap.limbs_to_int(ops.pair_hist(torch.as_tensor(dense.view(np.int64)).cuda(), n, d_w, lanes16).cpu().numpy())
        out = to_ints(ops.pair_moments(torch.as_tensor(grows.view(np.int64)).cuda(), G, wpg, d_w, wmax, lanes16))
        assert sum(hist) == out[G][G], name
        assert sum(d * h for d, h in enumerate(hist)) == sum(out[g][G] for g in range(G)), name
        assert sum(d * d * h for d, h in enumerate(hist)) == sum(out[g][k] for g in range(G) for k in range(G)), name
        assert out[G][G] > 0


# ---------------------------------------------------------------------------------------------- 3. independence of the grid
@pytest.mark.parametrize('lanes16', [False, True])
def test_result_does_not_depend_on_the_grid(lanes16, monkeypatch):
    M = 300
    cases = [(cref.make_group_rows(M, G, wpg, lanes16, seed=G), G, wpg) for G, wpg in SHAPES + ((26, 1), (27, 1))]
    same = cref.make_group_rows(M, 16, 2, lanes16, seed=9)
    same[:] = same[0]
    cases.append((same, 16, 2))                                        # 300 identical rows: every distance is 0
    for rows, G, wpg in cases:
        wmax = cref.wmax_of(wpg, lanes16)
        for name, w in cref.weight_sets(M, wmax, seed=G).items():
            out = {}
            for wgs in ('1', '3', None):
                if wgs is None:
                    monkeypatch.delenv('TN_PAIR_MOMENTS_WGS', raising=False)
                else:
                    monkeypatch.setenv('TN_PAIR_MOMENTS_WGS', wgs)
                out[wgs] = run(rows, G, wpg, w, wmax, lanes16)
            assert out['1'] == out[None] and out['3'] == out[None], (G, wpg, name)
            if rows is same and name == 'max':
                assert out[None][G][G] == wmax * wmax * (M * (M - 1) // 2)
                assert not any(out[None][i][j] for i in range(G + 1) for j in range(G + 1) if (i, j) != (G, G))
    monkeypatch.delenv('TN_PAIR_MOMENTS_WGS', raising=False)
    assert run(same, 16, 2, None, cref.wmax_of(2, lanes16), lanes16)[16][16] == M * (M - 1) // 2


# ---------------------------------------------------------------------------------------------- 4. workspace and output contract
@pytest.mark.parametrize('lanes16', [0, 1])
def test_workspace_and_output_contract(lanes16):
    """Exactly tn_pair_moments_ws_bytes suffices whatever the workspace and the output held before; every entry of out is written;
    the guards stay intact; one byte less is -3 and a shape outside the limits -1 with the limit in the message, and then nothing
    is written."""
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    M, G, wpg = 300, 16, 2
    rows = cref.make_group_rows(M, G, wpg, bool(lanes16), seed=31)
    ld = rows.shape[1]
    wmax = cref.wmax_of(wpg, bool(lanes16))
    w = cref.weight_sets(M, wmax, seed=3)['random']
    want = cref.limbs3(cref.pair_moments_ref(rows, G, wpg, w, wmax, bool(lanes16)))
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    d_w = torch.as_tensor(w.astype(np.uint32).view(np.int32)).cuda()
    need = int(L.tn_pair_moments_ws_bytes(M, G, wpg, lanes16))
    assert need > 0
    shape = (G + 1, G + 1, 2)
    for fill in (0xFF, 'random'):
        ws = Guarded(need, fill, seed=1)
        out = Guarded.of(torch.int64, shape, fill, seed=2)
        rc = L.tn_pair_moments(d_rows.data_ptr(), M, G, wpg, ld, d_w.data_ptr(), wmax, lanes16, out.ptr, ws.ptr, need, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert ws.intact() and out.intact()
        assert np.array_equal(out.host().view(np.uint64), want)       # every entry holds its value
    ws = Guarded(need - 1, 0xFF, seed=3)
    out = Guarded.of(torch.int64, shape, 0xFF, seed=4)
    rc = L.tn_pair_moments(d_rows.data_ptr(), M, G, wpg, ld, d_w.data_ptr(), wmax, lanes16, out.ptr, ws.ptr, need - 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == -3
    assert ws.untouched(0xFF) and out.untouched(0xFF) and ws.intact() and out.intact()
    # outside the limits: -1, the limit in the message, nothing written
    dmax = cref.dmax_of(wpg, bool(lanes16))
    big = Guarded(1 << 20, 0xFF, seed=7)
    wide = torch.zeros((M, 65 * 33), dtype=torch.int64, device='cuda')
    for (g, k, wm), word in (((0, wpg, wmax), '64'), ((65, wpg, wmax), '64'), ((G, 33, 1), '32'), ((G, wpg, 0), 'wmax'),
                             ((G, wpg, 2 ** 32 // dmax), '4294967295')):
        out = Guarded.of(torch.int64, (66, 66, 2), 0xFF, seed=8)
        rc = L.tn_pair_moments(wide.data_ptr(), M, g, k, 65 * 33, d_w.data_ptr(), wm, lanes16, out.ptr, big.ptr, big.nbytes, ops._stream())
        torch.cuda.synchronize()
        assert rc == -1 and word in last_error(L), (g, k, wm, last_error(L))
        assert out.untouched(0xFF) and big.untouched(0xFF) and out.intact() and big.intact()
    # M < 2: zeros in every entry
    out = Guarded.of(torch.int64, shape, 0xFF, seed=5)
    ws = Guarded(int(L.tn_pair_moments_ws_bytes(1, G, wpg, lanes16)), 0xFF, seed=6)
    assert L.tn_pair_moments(d_rows.data_ptr(), 1, G, wpg, ld, None, wmax, lanes16, out.ptr, ws.ptr, ws.nbytes, ops._stream()) == 0
    torch.cuda.synchronize()
    assert not out.host().any() and out.intact() and ws.intact()


# ---------------------------------------------------------------------------------------------- 5. pipeline against all M^2 pairs
STORED = ('overlap_line_correlations', 'overlap_line_mean', 'overlap_line_sizes', 'overlap_chi', 'overlap_xi', 'overlap_xi_over_L')


@pytest.fixture(scope='module')
def pipeline_cases():
    """kind -> weights -> (returned, stored attributes, {axis: reference}, more): M = 2048 on the droplet lattice, both axes."""
    from tnac4o_amd import overlap
    M = 2048
    out = {}
    for kind in ('spin', 'cell'):
        rng = np.random.default_rng(11)
        s = droplet()
        out[kind] = {}
        for name in ('uniform', 'float'):
            s.states = states_with_duplicates(M, rng, 60 if name == 'uniform' else 700).astype(np.uint8).astype(s.indtype)
            w = np.ones(M) if name == 'uniform' else 10.0 ** rng.uniform(-12.0, 0.0, M)
            more = {}
            if kind == 'spin' and name == 'uniform':
                s.calculate_overlap_distribution('spin')
                more = dict(chi_sg=s.overlap_moments['chi_sg'], P=s.overlap_distribution.copy(), pairs=s.overlap_pairs)
            C = s.calculate_overlap_correlations('both', kind, 'uniform' if name == 'uniform' else w)
            if more:
                more['P_after'], more['pairs_after'], more['chi_sg_after'] = s.overlap_distribution, s.overlap_pairs, s.overlap_moments['chi_sg']
            src = source(s, kind, unsigned=True)
            ref = {ax: cref.correlations_ref(src, overlap.line_groups(s, ax, kind)[0], 4, w, kind) for ax in ('x', 'y')}
            more.update(K=np.unique(src, axis=0).shape[0], w=w, ess=s.overlap_ess, kind=s.overlap_line_kind)
            out[kind][name] = (C, {a: getattr(s, a) for a in STORED}, ref, more)
    return out


@pytest.mark.parametrize('kind', ['spin', 'cell'])
def test_pipeline_uniform_weights(pipeline_cases, kind):
    """Uniform weights: the device part is the exact pair count, and every sum of the reference is a sum of integers below 2^53, so
    both sides are exact up to their final divisions."""
    C, got, ref, more = pipeline_cases[kind]['uniform']
    assert more['K'] <= 60 and C is got['overlap_line_correlations'] and sorted(C) == ['x', 'y'] and more['kind'] == kind
    assert more['ess'] == pytest.approx(2048.0, rel=1e-12)
    for ax in ('x', 'y'):
        assert C[ax].shape == (4, 4) and np.array_equal(C[ax], C[ax].T)
        assert np.array_equal(got['overlap_line_sizes'][ax], ref[ax]['sizes']) and ref[ax]['sizes'].sum() == (128 if kind == 'spin' else 16)
        err = np.max(np.abs(C[ax] - ref[ax]['C']) / np.maximum(np.abs(ref[ax]['C']), 1e-300))
        print('%s, axis %s, uniform: %d distinct rows, largest relative deviation of C %.2e' % (kind, ax, more['K'], err))
        assert np.allclose(C[ax], ref[ax]['C'], rtol=1e-13, atol=0.0)
        assert np.allclose(got['overlap_line_mean'][ax], ref[ax]['mean'], rtol=1e-13, atol=0.0)
        assert got['overlap_chi'][ax].shape == (3,)
        assert np.allclose(got['overlap_chi'][ax], ref[ax]['chi'], rtol=1e-13, atol=0.0)
        chi = ref[ax]['chi']
        want_xi = np.sqrt(chi[0] / chi[1] - 1.0) / (2.0 * np.sin(np.pi / 4)) if chi[1] > 0 and chi[0] >= chi[1] else np.nan
        assert got['overlap_xi'][ax] == pytest.approx(want_xi, rel=1e-9, nan_ok=True)
        assert got['overlap_xi_over_L'][ax] == pytest.approx(want_xi / 4, rel=1e-9, nan_ok=True)
        if kind == 'spin':                                             # chi at k = 0 is chi_SG of the overlap distribution
            assert got['overlap_chi'][ax][0] == pytest.approx(more['chi_sg'], rel=1e-12)
    if kind == 'spin':                                                 # what calculate_overlap_distribution stored is still there
        assert np.array_equal(more['P'], more['P_after']) and more['pairs'] == more['pairs_after'] and more['chi_sg'] == more['chi_sg_after']


@pytest.mark.parametrize('kind', ['spin', 'cell'])
def test_pipeline_float_weights(pipeline_cases, kind):
    """Weights over 12 orders of magnitude.  Each quantised weight is off by at most max W / (2 wmax) and C is a ratio of sums of pair
    products with |q_g q_g'| <= 1 over K distinct rows: |C - C_ref| <= 2 K / wmax, wmax = (2^32 - 1) / dmax."""
    C, got, ref, more = pipeline_cases[kind]['float']
    wmax = (2 ** 32 - 1) // (64 if kind == 'spin' else 4)
    assert more['K'] > 300
    for ax in ('x', 'y'):
        err = float(np.max(np.abs(C[ax] - ref[ax]['C'])))
        print('%s, axis %s, float weights: %d distinct rows, largest deviation %.2e, bound %.2e' % (kind, ax, more['K'], err, 2.0 * more['K'] / wmax))
        assert err <= 2.0 * more['K'] / wmax
    w = more['w']
    assert more['ess'] == pytest.approx(w.sum() ** 2 / np.sum(w * w), rel=1e-12)


# ---------------------------------------------------------------------------------------------- 6. end to end, exact law
def test_line_overlaps_of_boltzmann_samples():
    """ising_3x3_nc2 at beta = 1, 2^14 samples of an exact contraction (q = p), axis 'x': each of the 6 distinct <Q_g Q_g'> within
    5 sigma of its exact value for two independent replicas, sigma^2 = 2 Var(Q_g Q_g') / M from the exact law (the bound on the
    variance of a pair U-statistic of M independent draws)."""
    import marginals_ref as mr
    import tnac4o_amd
    from tnac4o_amd import auxx, overlap
    M, beta = 2 ** 14, 1.0
    act = [i for i in range(18) if i != 9]                            # spin 9 has no term: it is not part of the law
    binary = np.zeros((2 ** 17, 18), dtype=np.int8)
    binary[:, act] = (np.arange(2 ** 17)[:, None] >> np.arange(17)[None, :]) & 1
    E = auxx.energy_Jij(mr.ising_3x3_nc2(), binary)
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=beta)
    group, sizes = overlap.line_groups(ins, 'x', 'spin')
    Eq, Vq = cref.exact_line_moments(p, group, 3)
    np.random.seed(20241018)
    ins.sample_boltzmann(M=M, Dmax=64)
    C = ins.calculate_overlap_correlations(axis='x')
    assert sorted(C) == ['x'] and sorted(ins.overlap_chi) == ['x'] and ins.overlap_line_kind == 'spin'
    assert np.array_equal(ins.overlap_line_sizes['x'], sizes) and sizes.tolist() == [6, 5, 6]
    QQ = C['x'] * np.outer(sizes, sizes)
    sigma = np.sqrt(2.0 * Vq / M)
    for g in range(3):
        for h in range(g, 3):
            print('<Q_%d Q_%d> = %.5f, exact %.5f, sigma %.2e: %.2f sigma' % (g, h, QQ[g, h], Eq[g, h], sigma[g, h], abs(QQ[g, h] - Eq[g, h]) / sigma[g, h]))
            assert abs(QQ[g, h] - Eq[g, h]) <= 5.0 * sigma[g, h]
    assert ins.overlap_ess == pytest.approx(M, rel=1e-12)
    # the contraction is exact: the importance weights are equal up to rounding
    Ci = ins.calculate_overlap_correlations(axis='x', weights='importance')
    assert float(np.max(np.abs(Ci['x'] - C['x']))) <= 1e-9


# ---------------------------------------------------------------------------------------------- 7. RMF
def test_cell_line_overlaps_on_rmf():
    import tnac4o_amd
    from tnac4o_amd import auxx, overlap
    ins = tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=3, J=auxx.synthetic_rmf(3, 3, 3, 17), beta=1.0)
    np.random.seed(5)
    ins.sample_boltzmann(M=1024, Dmax=64)
    C = ins.calculate_overlap_correlations()
    assert ins.overlap_line_kind == 'cell' and sorted(C) == ['x', 'y']
    X = np.asarray(ins.states).astype(np.int64)
    for ax in ('x', 'y'):
        ref = cref.correlations_ref(X, overlap.line_groups(ins, ax, 'cell')[0], 3, np.ones(1024), 'cell')
        assert ins.overlap_line_sizes[ax].tolist() == [3, 3, 3]
        assert np.allclose(C[ax], ref['C'], rtol=1e-13, atol=0.0)
        assert np.allclose(ins.overlap_line_mean[ax], ref['mean'], rtol=1e-13, atol=0.0)
        assert np.allclose(ins.overlap_chi[ax], ref['chi'], rtol=1e-13, atol=0.0)
    with pytest.raises(ValueError):
        ins.calculate_overlap_correlations(kind='link')
    before = {a: getattr(ins, a) for a in STORED}
    ins.Nx_model = 65                                                  # a lattice mocked to 65 columns: refused before any device work
    with pytest.raises(NotImplementedError, match='64'):
        ins.calculate_overlap_correlations()
    assert all(getattr(ins, a) is before[a] for a in STORED)
