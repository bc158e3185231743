"""tn_pair_rowsums and tnac4o.calculate_overlap_errors on the GPU: the kernel against brute force in Python integers (both limbs, every
row and entry), against tn_pair_hist, independence of the grid, the workspace and output contract, the host pipeline against the
jackknife of the reference integers, and the errors of sample_boltzmann's samples against the exact variance of the projections."""
import numpy as np
import pytest

import overlap_ref as oref
import rowsums_ref as rref
from guarded import Guarded
from overlap_ref import WMAX, droplet, make_rows

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

MS = (1, 2, 63, 64, 65, 129, 300)
NBITS = (1, 63, 64, 65, 130, 2048)
MAX_NBITS = 65535


def device(rows, nbits, w, lanes16):
    """(rows view with the stride of make_rows' padding, weights) on the device."""
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    nwords = -(-nbits // (4 if lanes16 else 64))
    d_w = None if w is None else torch.as_tensor(np.asarray(w, dtype=np.uint64).astype(np.uint32).view(np.int32)).cuda()
    return d_rows[:, :nwords], d_w


def run(rows, nbits, w, lanes16):
    """ops.pair_rowsums on host arrays -> M lists of six Python integers."""
    from tnac4o_amd import ops, overlap
    d_rows, d_w = device(rows, nbits, w, lanes16)
    out = ops.pair_rowsums(d_rows, nbits, d_w, lanes16)
    assert out.shape == (rows.shape[0], 6, 2) and out.dtype == torch.int64
    return overlap.rowsums_to_int(out.cpu().numpy())


def diffs(got, want):
    return [(a, k, got[a][k], want[a][k]) for a in range(len(want)) for k in range(6) if got[a][k] != want[a][k]][:4]


def bit_dist(rows, nbits):
    """pair_dist_ref for long rows of bits: the distances from a float32 product of the spins, exact below 2^24."""
    S = 2.0 * oref.unpack_rows(rows, nbits, False).astype(np.float32) - 1.0
    return np.rint((nbits - S @ S.T) / 2.0).astype(np.int64)


# ---------------------------------------------------------------------------------------------- 5. kernel against brute force
@pytest.mark.parametrize('lanes16', [False, True])
@pytest.mark.parametrize('nbits', NBITS)
@pytest.mark.parametrize('M', MS)
def test_pair_rowsums_is_exact(M, nbits, lanes16):
    rows = make_rows(M, nbits, lanes16, seed=1000 * M + nbits)
    D = oref.pair_dist_ref(rows, nbits, lanes16)
    if M >= 2:
        assert D[0, M - 1] == nbits and (M < 3 or D[0, 1] == 0)
    for name, w in oref.weight_sets(M, WMAX, seed=M + nbits).items():
        want = rref.pair_rowsums_ref(rows, nbits, w, lanes16, dist=D)
        got = run(rows, nbits, w, lanes16)
        assert got == want, (name, diffs(got, want))
    if M == 1:
        assert want == [[0] * 6]


@pytest.mark.parametrize('lanes16', [False, True])
def test_pair_rowsums_at_the_largest_nbits(lanes16):
    from tnac4o_amd import _lib, ops
    M, nbits = 65, MAX_NBITS
    rows = make_rows(M, nbits, lanes16, seed=77)
    D = oref.pair_dist_ref(rows, nbits, lanes16)
    assert D[0, M - 1] == nbits
    for name, w in oref.weight_sets(M, WMAX, seed=5).items():
        want = rref.pair_rowsums_ref(rows, nbits, w, lanes16, dist=D)
        got = run(rows, nbits, w, lanes16)
        assert got == want, (name, diffs(got, want))
    with pytest.raises(_lib.TnError, match=str(nbits)):               # one more is refused by name, nothing launched
        ops.pair_rowsums(torch.zeros((2, 1 << 14), dtype=torch.int64, device='cuda'), nbits + 1, None, lanes16)


def test_carry_into_the_high_limb():
    """M = 300 rows of 65535 bits with all-maximum weights: sums of w d^4 beyond 2^100."""
    M, nbits = 300, MAX_NBITS
    rows = make_rows(M, nbits, False, seed=78)
    D = bit_dist(rows, nbits)
    assert D[0, M - 1] == nbits and D[0, 1] == 0 and np.array_equal(D[:8, :8], oref.pair_dist_ref(rows[:8], nbits, False))
    w = np.full(M, WMAX, dtype=np.uint64)
    want = rref.pair_rowsums_ref(rows, nbits, w, False, dist=D)
    assert max(r[4] for r in want) > 2 ** 100 and min(r[3] for r in want) > 2 ** 64
    got = run(rows, nbits, w, False)
    assert got == want, diffs(got, want)


# ---------------------------------------------------------------------------------------------- 6. against tn_pair_hist
@pytest.mark.parametrize('lanes16', [False, True])
@pytest.mark.parametrize('nbits', (1, 65, 130, 2048))
def test_weighted_row_sums_are_twice_the_histogram_moments(nbits, lanes16):
    """sum_a w_a out[a][k] = 2 sum_d hist[d] d^k for k = 0 .. 4, and sum_a w_a out[a][5] = 2 sum_d hist[d] |nbits - 2 d|: two kernels,
    the same integers."""
    from tnac4o_amd import ops, overlap
    for M in (65, 300):
        rows = make_rows(M, nbits, lanes16, seed=M + 7 * nbits)
        for name, w in oref.weight_sets(M, WMAX, seed=nbits).items():
            d_rows, d_w = device(rows, nbits, w, lanes16)
            hist = overlap.limbs_to_int(ops.pair_hist(d_rows, nbits, d_w, lanes16).cpu().numpy())
            R = run(rows, nbits, w, lanes16)
            wi = [1] * M if w is None else [int(x) for x in w]
            for k in range(5):
                assert sum(wi[a] * R[a][k] for a in range(M)) == 2 * sum(h * d ** k for d, h in enumerate(hist)), (M, name, k)
            assert sum(wi[a] * R[a][5] for a in range(M)) == 2 * sum(h * abs(nbits - 2 * d) for d, h in enumerate(hist)), (M, name)


# ---------------------------------------------------------------------------------------------- 7. independence of the grid
@pytest.mark.parametrize('lanes16', [False, True])
def test_result_does_not_depend_on_the_grid(lanes16, monkeypatch):
    M = 300
    cases = [(make_rows(M, nbits, lanes16, seed=nbits), nbits) for nbits in (1, 65, 130, 2048)]
    same = make_rows(M, 130, lanes16, seed=9)
    same[:] = same[0]
    cases.append((same, 130))                                          # 300 identical rows: every distance is 0
    for rows, nbits in cases:
        for name, w in oref.weight_sets(M, WMAX, seed=nbits).items():
            out = {}
            for wgs in ('1', '3', None):
                if wgs is None:
                    monkeypatch.delenv('TN_PAIR_ROWSUMS_WGS', raising=False)
                else:
                    monkeypatch.setenv('TN_PAIR_ROWSUMS_WGS', wgs)
                out[wgs] = run(rows, nbits, w, lanes16)
            assert out['1'] == out[None] and out['3'] == out[None], (nbits, name)
            if rows is same and name == 'max':
                assert out[None] == [[WMAX * (M - 1), 0, 0, 0, 0, WMAX * (M - 1) * nbits]] * M
    monkeypatch.delenv('TN_PAIR_ROWSUMS_WGS', raising=False)
    assert run(same, 130, None, lanes16) == [[M - 1, 0, 0, 0, 0, (M - 1) * 130]] * M


# ---------------------------------------------------------------------------------------------- 8. workspace and output contract
@pytest.mark.parametrize('lanes16', [0, 1])
def test_workspace_and_output_contract(lanes16, monkeypatch):
    """Exactly tn_pair_rowsums_ws_bytes suffices whatever the workspace and the output held before; the whole of out is written; the
    guards stay intact; one byte less is -3 and nothing is written; M = 1 writes six zeros."""
    from tnac4o_amd import _lib, ops
    monkeypatch.delenv('TN_PAIR_ROWSUMS_WGS', raising=False)
    L = _lib.lib()
    M, nbits = 300, 130
    rows = make_rows(M, nbits, bool(lanes16), seed=31)
    ld = rows.shape[1]
    w = oref.weight_sets(M, WMAX, seed=3)['random']
    want = rref.limbs(rref.pair_rowsums_ref(rows, nbits, w, bool(lanes16)))
    d_rows = torch.as_tensor(rows.view(np.int64)).cuda()
    d_w = torch.as_tensor(w.astype(np.uint32).view(np.int32)).cuda()
    need = int(L.tn_pair_rowsums_ws_bytes(M, nbits, lanes16))
    assert need > M * 6 * 16                                           # more than one slab: the default grid splits the columns
    for fill in (0xFF, 'random'):
        ws = Guarded(need, fill, seed=1)
        out = Guarded.of(torch.int64, (M, 6, 2), fill, seed=2)
        rc = L.tn_pair_rowsums(d_rows.data_ptr(), M, nbits, ld, d_w.data_ptr(), lanes16, out.ptr, ws.ptr, need, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert ws.intact() and out.intact()
        assert np.array_equal(out.host().view(np.uint64).reshape(M, 6, 2), want)
    ws = Guarded(need - 1, 0xFF, seed=3)
    out = Guarded.of(torch.int64, (M, 6, 2), 0xFF, seed=4)
    rc = L.tn_pair_rowsums(d_rows.data_ptr(), M, nbits, ld, d_w.data_ptr(), lanes16, out.ptr, ws.ptr, need - 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == -3
    assert ws.untouched(0xFF) and out.untouched(0xFF) and ws.intact() and out.intact()
    # M = 1: six zeros, whatever the weight of the row
    out = Guarded.of(torch.int64, (1, 6, 2), 0xFF, seed=5)
    ws = Guarded(int(L.tn_pair_rowsums_ws_bytes(1, nbits, lanes16)), 0xFF, seed=6)
    assert L.tn_pair_rowsums(d_rows.data_ptr(), 1, nbits, ld, d_w.data_ptr(), lanes16, out.ptr, ws.ptr, ws.nbytes, ops._stream()) == 0
    torch.cuda.synchronize()
    assert not out.host().any() and out.intact() and ws.intact()
    # M = 0: nothing is written
    out = Guarded.of(torch.int64, (1, 6, 2), 0xFF, seed=7)
    ws = Guarded(int(L.tn_pair_rowsums_ws_bytes(0, nbits, lanes16)), 0xFF, seed=8)
    assert L.tn_pair_rowsums(d_rows.data_ptr(), 0, nbits, ld, None, lanes16, out.ptr, ws.ptr, ws.nbytes, ops._stream()) == 0
    torch.cuda.synchronize()
    assert out.untouched(0xFF) and ws.untouched(0xFF) and out.intact() and ws.intact()
    assert ops.pair_rowsums(d_rows[:0], nbits, None, bool(lanes16)).shape == (0, 6, 2)


# ---------------------------------------------------------------------------------------------- 9. pipeline
STORED = ('overlap_errors', 'overlap_error_estimates', 'overlap_bias_corrected')


@pytest.fixture(scope='module')
def pipeline_cases():
    """kind -> weights -> (what the call stored, the jackknife of the reference integers, overlap_moments of the distribution, n):
    M = 2048 states with duplicates on the droplet lattice."""
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
            s.calculate_overlap_distribution(kind, 'uniform' if name == 'uniform' else w)
            before = {a: getattr(s, a) for a in ('overlap_distribution', 'overlap_values', 'overlap_moments', 'overlap_kind', 'overlap_pairs')}
            ret = s.calculate_overlap_errors(kind, 'uniform' if name == 'uniform' else w)
            assert ret is s.overlap_errors and s.overlap_error_kind == kind
            assert all(getattr(s, a) is v for a, v in before.items())          # nothing of calculate_overlap_distribution is rewritten
            R, wq, scale, inv, n = rref.class_rowsums(oref.source(s, kind, unsigned=True), w, kind)
            got = {a: getattr(s, a) for a in STORED + ('overlap_state_q', 'overlap_state_q2', 'overlap_ess')}
            out[kind][name] = (got, overlap.jackknife(R, wq, scale, inv, w, n, kind), dict(s.overlap_moments), n, w)
    return out


@pytest.mark.parametrize('kind', ['spin', 'link', 'cell'])
def test_pipeline_uniform_weights(pipeline_cases, kind):
    got, jk, moments, n, w = pipeline_cases[kind]['uniform']
    assert got['overlap_errors'] == jk['error'] and got['overlap_error_estimates'] == jk['estimate']
    assert got['overlap_bias_corrected'] == jk['bias_corrected']
    assert np.array_equal(got['overlap_state_q'], jk['state_q']) and np.array_equal(got['overlap_state_q2'], jk['state_q2'])
    assert got['overlap_state_q'].shape == (2048,) and not np.isnan(got['overlap_state_q']).any()
    assert set(got['overlap_errors']) == set(moments) and ('chi_sg' in moments) == (kind == 'spin')
    assert all(v > 0 for v in got['overlap_errors'].values())
    assert got['overlap_ess'] == pytest.approx(2048.0, rel=1e-12)
    for k in ('q', 'abs_q', 'q2', 'q4'):
        dev = abs(got['overlap_error_estimates'][k] - moments[k])
        print('%s, uniform, %s = %.12f +- %.2e: off overlap_moments by %.1e, bound %.1e' % (kind, k, moments[k], got['overlap_errors'][k], dev,
                                                                                           8 * (n + 1) * 2.0 ** -52))
        assert dev <= 8 * (n + 1) * 2.0 ** -52


@pytest.mark.parametrize('kind', ['spin', 'link', 'cell'])
def test_pipeline_float_weights(pipeline_cases, kind):
    got, jk, moments, n, w = pipeline_cases[kind]['float']
    for a, part in zip(STORED, ('error', 'estimate', 'bias_corrected')):
        for k, v in jk[part].items():
            assert got[a][k] == pytest.approx(v, rel=1e-12), (a, k)
    assert np.allclose(got['overlap_state_q'], jk['state_q'], rtol=1e-12, atol=0.0, equal_nan=True)
    assert np.allclose(got['overlap_state_q2'], jk['state_q2'], rtol=1e-12, atol=0.0, equal_nan=True)
    assert got['overlap_ess'] == pytest.approx(w.sum() ** 2 / np.sum(w * w), rel=1e-12)
    for k in ('q', 'abs_q', 'q2', 'q4'):
        dev = abs(got['overlap_error_estimates'][k] - moments[k])
        print('%s, float weights, %s = %.12f +- %.2e: off overlap_moments by %.1e, bound %.1e' % (kind, k, moments[k], got['overlap_errors'][k], dev,
                                                                                                 8 * (n + 1) * 2.0 ** -52))
        assert dev <= 8 * (n + 1) * 2.0 ** -52


# ---------------------------------------------------------------------------------------------- 10. end to end
def test_errors_of_boltzmann_samples():
    """ising_3x3_nc2 at beta = 1, 2^12 samples of an exact contraction (q = p).  With m = <s>, C = <s s^T> of the enumerated law p:
    q_exact = m.m / N, q2_exact = sum C_ij^2 / N^2; the pair statistics have the projections h_q(x) = x.m / N and
    h_q2(x) = x^T C x / N^2, so their variance over M independent draws is sigma^2 = 4 Var_p(h) / M to leading order.  The
    estimate lies within 5 errors of the exact value and the error within 10 % of sigma, for q and q2."""
    import marginals_ref as mr
    from tnac4o_amd import auxx
    M, beta, N = 2 ** 12, 1.0, 17
    act = [i for i in range(18) if i != 9]                            # spin 9 has no term: it is not part of the law
    binary = np.zeros((2 ** 17, 18), dtype=np.int8)
    binary[:, act] = (np.arange(2 ** 17)[:, None] >> np.arange(17)[None, :]) & 1
    E = auxx.energy_Jij(mr.ising_3x3_nc2(), binary)
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    S = 2.0 * binary[:, act] - 1.0
    m = p @ S
    C = S.T @ (S * p[:, None])
    exact = {'q': float(m @ m) / N, 'q2': float(np.sum(C * C)) / N ** 2}
    h = {'q': S @ m / N, 'q2': np.sum((S @ C) * S, axis=1) / N ** 2}
    ins = oref.ising3x3(beta)
    ins.sample_boltzmann(M=M, Dmax=64, seed=20261021)
    err = ins.calculate_overlap_errors('spin')
    assert ins.overlap_error_kind == 'spin' and ins.overlap_state_q.shape == (M,) and ins.overlap_ess == pytest.approx(M, rel=1e-12)
    for k in ('q', 'q2'):
        sigma = float(np.sqrt(4.0 * (p @ h[k] ** 2 - (p @ h[k]) ** 2) / M))
        got = ins.overlap_error_estimates[k]
        print('%s = %.6f +- %.2e, exact %.6f (%.2f errors), sigma %.2e, error / sigma = %.3f' % (k, got, err[k], exact[k], abs(got - exact[k]) / err[k],
                                                                                                 sigma, err[k] / sigma))
        assert abs(got - exact[k]) <= 5.0 * err[k]
        assert 0.9 <= err[k] / sigma <= 1.1
    assert ins.overlap_error_estimates['chi_sg'] == pytest.approx(N * ins.overlap_error_estimates['q2'], rel=1e-14)
