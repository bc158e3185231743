"""tn_pair_hist and tnac4o.calculate_overlap_distribution on the GPU: the kernel against brute force in Python integers (both limbs,
exactly), independence of the grid, the workspace and output contract, the host pipeline against all M^2 pairs in float64, and the
overlap law of sample_boltzmann's samples against the exact one of two independent replicas."""
import numpy as np
import pytest

import overlap_ref as oref
from guarded import Guarded
from overlap_ref import WMAX, droplet, make_rows

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

MS = (1, 2, 63, 64, 65, 129, 300)
NBITS = (1, 63, 64, 65, 130, 2048)


def run(rows, nbits, w, lanes16):
    """ops.pair_hist on host arrays -> Python integers."""
    from tnac4o_amd import ops, overlap
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    nwords = -(-nbits // (4 if lanes16 else 64))
    d_w = None if w is None else torch.as_tensor(np.asarray(w, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    out = ops.pair_hist(d_rows[:, :nwords], nbits, d_w, lanes16)          # a view: the stride stays nwords + 3
    assert out.shape == (nbits + 1, 2) and out.dtype == torch.int64
    return overlap.limbs_to_int(out.cpu().numpy())


# ---------------------------------------------------------------------------------------------- 1. kernel against brute force
@pytest.mark.parametrize('lanes16', [False, True])
@pytest.mark.parametrize('nbits', NBITS)
@pytest.mark.parametrize('M', MS)
def test_pair_hist_is_exact(M, nbits, lanes16):
    rows = make_rows(M, nbits, lanes16, seed=1000 * M + nbits)
    D = oref.pair_dist_ref(rows, nbits, lanes16)
    if M >= 2:
        assert D[0, M - 1] == nbits and (M < 3 or D[0, 1] == 0)
    for name, w in oref.weight_sets(M, WMAX, seed=M + nbits).items():
        want = oref.pair_hist_ref(rows, nbits, w, lanes16, dist=D)
        got = run(rows, nbits, w, lanes16)
        assert got == want, (name, [(d, g, x) for d, (g, x) in enumerate(zip(got, want)) if g != x][:4])
    if M < 2:
        assert not any(want)
    if M == 300 and nbits == 1:                                        # the carry case: all-maximum weights reach 2^78
        assert max(oref.pair_hist_ref(rows, nbits, np.full(M, WMAX, dtype=np.uint64), lanes16, dist=D)) > 2 ** 78


@pytest.mark.parametrize('lanes16', [False, True])
def test_pair_hist_at_the_largest_nbits(lanes16):
    from tnac4o_amd import _lib, ops, overlap
    M, nbits = 65, overlap.MAX_NBITS
    rows = make_rows(M, nbits, lanes16, seed=77)
    D = oref.pair_dist_ref(rows, nbits, lanes16)
    for name, w in oref.weight_sets(M, WMAX, seed=5).items():
        assert run(rows, nbits, w, lanes16) == oref.pair_hist_ref(rows, nbits, w, lanes16, dist=D), name
    with pytest.raises(_lib.TnError, match=str(nbits)):               # one more does not fit: refused by name, nothing launched
        ops.pair_hist(torch.zeros((2, 4096), dtype=torch.int64, device='cuda'), nbits + 1, None, lanes16)


# ---------------------------------------------------------------------------------------------- 2. independence of the grid
@pytest.mark.parametrize('lanes16', [False, True])
def test_result_does_not_depend_on_the_grid(lanes16, monkeypatch):
    M = 300
    cases = [(make_rows(M, nbits, lanes16, seed=nbits), nbits) for nbits in (1, 65, 130, 2048)]
    same = make_rows(M, 130, lanes16, seed=9)
    same[:] = same[0]
    cases.append((same, 130))                                          # 300 identical rows: every pair in bin 0
    for rows, nbits in cases:
        for name, w in oref.weight_sets(M, WMAX, seed=nbits).items():
            out = {}
            for wgs in ('1', '3', None):
                if wgs is None:
                    monkeypatch.delenv('TN_PAIR_HIST_WGS', raising=False)
                else:
                    monkeypatch.setenv('TN_PAIR_HIST_WGS', wgs)
                out[wgs] = run(rows, nbits, w, lanes16)
            assert out['1'] == out[None] and out['3'] == out[None], (nbits, name)
            if rows is same and name == 'max':
                assert out[None][0] == WMAX * WMAX * (M * (M - 1) // 2) and not any(out[None][1:])
    monkeypatch.delenv('TN_PAIR_HIST_WGS', raising=False)
    assert run(same, 130, None, lanes16)[0] == M * (M - 1) // 2


# ---------------------------------------------------------------------------------------------- 3. workspace and output contract
@pytest.mark.parametrize('lanes16', [0, 1])
def test_workspace_and_output_contract(lanes16):
    """Exactly tn_pair_hist_ws_bytes suffices whatever the workspace and the output held before; the whole of hist_out is written;
    the guards stay intact; one byte less is -3 and nothing is written."""
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    M, nbits = 300, 130
    rows = make_rows(M, nbits, bool(lanes16), seed=31)
    ld = rows.shape[1]
    w = oref.weight_sets(M, WMAX, seed=3)['random']
    want = oref.limbs(oref.pair_hist_ref(rows, nbits, w, bool(lanes16)))
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    d_w = torch.as_tensor(w.astype(np.uint32).view(np.int32)).cuda()
    need = int(L.tn_pair_hist_ws_bytes(M, nbits, lanes16))
    assert need > 0
    for fill in (0xFF, 'random'):
        ws = Guarded(need, fill, seed=1)
        out = Guarded.of(torch.int64, (nbits + 1, 2), fill, seed=2)
        rc = L.tn_pair_hist(d_rows.data_ptr(), M, nbits, ld, d_w.data_ptr(), lanes16, out.ptr, ws.ptr, need, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert ws.intact() and out.intact()
        assert np.array_equal(out.host().view(np.uint64), want)       # every bin, the empty ones included, holds its value
    ws = Guarded(need - 1, 0xFF, seed=3)
    out = Guarded.of(torch.int64, (nbits + 1, 2), 0xFF, seed=4)
    rc = L.tn_pair_hist(d_rows.data_ptr(), M, nbits, ld, d_w.data_ptr(), lanes16, out.ptr, ws.ptr, need - 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == -3
    assert ws.untouched(0xFF) and out.untouched(0xFF) and ws.intact() and out.intact()
    # M < 2: zeros in every bin
    out = Guarded.of(torch.int64, (nbits + 1, 2), 0xFF, seed=5)
    ws = Guarded(int(L.tn_pair_hist_ws_bytes(1, nbits, lanes16)), 0xFF, seed=6)
    assert L.tn_pair_hist(d_rows.data_ptr(), 1, nbits, ld, None, lanes16, out.ptr, ws.ptr, ws.nbytes, ops._stream()) == 0
    torch.cuda.synchronize()
    assert not out.host().any() and out.intact() and ws.intact()


# ---------------------------------------------------------------------------------------------- 4. pipeline against all M^2 pairs
@pytest.fixture(scope='module')
def pipeline_cases():
    """kind -> weights -> (solver attributes after the call, reference): M = 2048 on the droplet lattice."""
    from tnac4o_amd import overlap
    M = 2048
    out = {}
    for kind in ('spin', 'link', 'cell'):
        rng = np.random.default_rng(11)
        s = droplet()
        out[kind] = {}
        for name in ('uniform', 'float'):
            s.states = oref.states_with_duplicates(M, rng, 60 if name == 'uniform' else 700).astype(np.uint8).astype(s.indtype)
            w = np.ones(M) if name == 'uniform' else 10.0 ** rng.uniform(-12.0, 0.0, M)
            P = s.calculate_overlap_distribution(kind, 'uniform' if name == 'uniform' else w)
            src = oref.source(s, kind)
            K = np.unique(src, axis=0).shape[0]
            out[kind][name] = (P, dict(values=s.overlap_values, moments=dict(s.overlap_moments), ess=s.overlap_ess, pairs=s.overlap_pairs,
                                       kind=s.overlap_kind, stored=s.overlap_distribution, n=src.shape[1], K=K, w=w),
                               oref.distribution_ref(src, w, kind))
    return out


@pytest.mark.parametrize('kind', ['spin', 'link', 'cell'])
def test_pipeline_uniform_weights(pipeline_cases, kind):
    P, got, (values, Pref) = pipeline_cases[kind]['uniform']
    assert got['K'] <= 60 and P is got['stored'] and got['kind'] == kind and got['pairs'] == 2048 * 2047 // 2
    assert np.array_equal(got['values'], values) and P.shape == values.shape
    err = np.max(np.abs(P - Pref) / np.where(Pref > 0, Pref, 1.0))
    print('%s, uniform: %d distinct rows, largest relative deviation %.2e' % (kind, got['K'], err))
    assert np.allclose(P, Pref, rtol=1e-14, atol=0.0)                 # the device part is exact
    assert got['ess'] == pytest.approx(2048.0, rel=1e-12)
    q2 = float(Pref @ values ** 2)
    assert got['moments']['q2'] == pytest.approx(q2, rel=1e-12)
    assert ('chi_sg' in got['moments']) == (kind == 'spin')
    if kind == 'spin':
        assert got['n'] == 128 and got['moments']['chi_sg'] == pytest.approx(128 * q2, rel=1e-12)


@pytest.mark.parametrize('kind', ['spin', 'link', 'cell'])
def test_pipeline_float_weights(pipeline_cases, kind):
    """Weights over 12 orders of magnitude.  Each quantised weight is off by at most 2^-33 of the largest and P is a ratio of sums of
    pair products over K distinct rows: |P - P_ref| <= K 2^-31."""
    P, got, (values, Pref) = pipeline_cases[kind]['float']
    err = float(np.max(np.abs(P - Pref)))
    print('%s, float weights: %d distinct rows, largest deviation %.2e, bound %.2e' % (kind, got['K'], err, got['K'] * 2.0 ** -31))
    assert got['K'] > 300
    assert err <= got['K'] * 2.0 ** -31
    assert abs(P.sum() - 1.0) < 1e-12
    w = got['w']
    assert got['ess'] == pytest.approx(w.sum() ** 2 / np.sum(w * w), rel=1e-12)


# ---------------------------------------------------------------------------------------------- 5. end to end
def _small(case, beta=1.0):
    import tnac4o_amd
    from tnac4o_amd import auxx
    if case == 'ising3x3':
        return oref.ising3x3(beta)
    if case == 'rmf3x3':
        return oref.rmf(beta)
    return tnac4o_amd.tnac4o(mode='Ising', Nx=2, Ny=2, Nc=8, J=auxx.synthetic_chimera(2, 2, 29), beta=beta)


def test_overlap_law_of_boltzmann_samples():
    """ising_3x3_nc2 at beta = 1, 2^14 samples of an exact contraction (q = p): <q^2> of the pair estimate within 5 sigma of the exact
    value of two independent replicas, sigma^2 = 2 Var(q^2) / M from the exact law (the bound on the variance of a pair
    U-statistic of M independent draws)."""
    import marginals_ref as mr
    from tnac4o_amd import auxx
    M, beta = 2 ** 14, 1.0
    act = [i for i in range(18) if i != 9]                            # spin 9 has no term: it is not part of the law
    binary = np.zeros((2 ** 17, 18), dtype=np.int8)
    binary[:, act] = (np.arange(2 ** 17)[:, None] >> np.arange(17)[None, :]) & 1
    E = auxx.energy_Jij(mr.ising_3x3_nc2(), binary)
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    Pd = oref.exact_spin_overlap_law(p)
    q = 1.0 - 2.0 * np.arange(18) / 17.0
    q2, q4 = float(Pd @ q ** 2), float(Pd @ q ** 4)
    sigma = np.sqrt(2.0 * (q4 - q2 * q2) / M)
    ins = _small('ising3x3', beta)
    np.random.seed(20241017)
    ins.sample_boltzmann(M=M, Dmax=64)
    P = ins.calculate_overlap_distribution('spin').copy()
    assert ins.overlap_kind == 'spin' and P.shape == (18,) and np.array_equal(ins.overlap_values, q)
    got = ins.overlap_moments['q2']
    print('<q^2> = %.6f, exact %.6f, sigma %.2e: %.2f sigma' % (got, q2, sigma, abs(got - q2) / sigma))
    assert abs(got - q2) <= 5.0 * sigma
    assert ins.overlap_moments['chi_sg'] == pytest.approx(17 * got, rel=1e-14)
    assert ins.overlap_pairs == M * (M - 1) // 2 and ins.overlap_ess == pytest.approx(M, rel=1e-12)
    # the same from all pairs on the host
    from tnac4o_amd import overlap
    assert np.allclose(P, oref.distribution_ref(overlap.spin_bits(ins), np.ones(M), 'spin')[1], rtol=1e-14, atol=0.0)
    # the contraction is exact: the importance weights are equal up to rounding
    Pi = ins.calculate_overlap_distribution('spin', 'importance')
    assert float(np.max(np.abs(Pi - P))) <= 1e-9
    assert ins.overlap_ess == pytest.approx(M, rel=1e-9)
    # the default kind, and states from another source
    assert np.array_equal(ins.calculate_overlap_distribution(), P)


def test_cell_overlap_on_rmf():
    ins = _small('rmf3x3')
    np.random.seed(5)
    ins.sample_boltzmann(M=1024, Dmax=64)
    P = ins.calculate_overlap_distribution()
    assert ins.overlap_kind == 'cell' and 'chi_sg' not in ins.overlap_moments
    values, Pref = oref.distribution_ref(np.asarray(ins.states).astype(np.int64), np.ones(1024), 'cell')
    assert np.array_equal(ins.overlap_values, values)
    assert np.allclose(P, Pref, rtol=1e-14, atol=0.0)


def test_link_overlap_on_chimera_2x2():
    from tnac4o_amd import overlap
    ins = _small('chimera2x2')
    np.random.seed(6)
    ins.sample_boltzmann(M=1024, Dmax=64)
    P = ins.calculate_overlap_distribution('link')
    lb = overlap.link_bits(ins)
    values, Pref = oref.distribution_ref(lb, np.ones(1024), 'link')
    assert lb.shape[1] == overlap.link_pairs(ins.J0).shape[0] and np.array_equal(ins.overlap_values, values)
    assert np.allclose(P, Pref, rtol=1e-14, atol=0.0)
    # a search writes states too
    ins.search_ground_state(M=64, Dmax=64)
    if ins.states.shape[0] >= 2:
        Ps = ins.calculate_overlap_distribution('spin')
        assert np.allclose(Ps, oref.distribution_ref(overlap.spin_bits(ins), np.ones(ins.states.shape[0]), 'spin')[1], rtol=1e-14, atol=0.0)
