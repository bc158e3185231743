"""Host side of tnac4o.calculate_overlap_errors (tnac4o_amd/overlap.py: jackknife, overlap_errors) without a GPU: the jackknife against
a recomputation from scratch without each sample, its estimates against the trusted moments, its calibration on independent draws,
and what the driver and the export refuse before any device work."""
import numpy as np
import pytest

import overlap_ref as oref
import rowsums_ref as rref
from overlap_ref import droplet, last_error, rmf
from tnac4o_amd import overlap as ov

KINDS = ('spin', 'link', 'cell')
FOUR = ('q', 'abs_q', 'q2', 'q4')


def weights_of(name, M, rng):
    if name == 'uniform':
        return np.ones(M)
    if name == 'integer':                                              # exact arithmetic, some samples without weight
        w = rng.integers(0, 4, M).astype(np.float64)
        w[:3] = (0.0, 2.0, 1.0)
        return w
    w = 10.0 ** rng.uniform(-12.0, 0.0, M)                             # 12 decades, some samples without weight
    w[rng.random(M) < 0.15] = 0.0
    w[:2] = (0.0, 1.0)
    return w


@pytest.fixture(scope='module')
def cases():
    """(kind, weights) -> (X, w, jackknife of rowsums_ref's integers, jackknife_ref, K): 40 states of the droplet lattice from 12."""
    out = {}
    for kind in KINDS:
        for name in ('uniform', 'integer', 'float'):
            rng = np.random.default_rng(7)
            s = droplet()
            s.states = oref.states_with_duplicates(40, rng, 12).astype(np.uint8).astype(s.indtype)
            X = oref.source(s, kind, unsigned=True)
            w = weights_of(name, 40, rng)
            R, wq, scale, inv, n = rref.class_rowsums(X, w, kind)
            assert (scale == 1.0) == (name != 'float') and len(R) == wq.size < 40 and n == X.shape[1]
            out[kind, name] = (X, w, ov.jackknife(R, wq, scale, inv, w, n, kind), rref.jackknife_ref(X, w, kind), wq.size)
    return out


# ---------------------------------------------------------------------------------------------- 1. against the recomputation from scratch
@pytest.mark.parametrize('name', ['uniform', 'integer'])
@pytest.mark.parametrize('kind', KINDS)
def test_jackknife_equals_brute_force(cases, kind, name):
    X, w, jk, (est, loo, err, corr), K = cases[kind, name]
    keys = set(est)
    assert keys == {'q', 'abs_q', 'q2', 'q4', 'binder'} | ({'chi_sg'} if kind == 'spin' else set())
    for part in ('estimate', 'error', 'bias_corrected', 'leave_one_out'):
        assert set(jk[part]) == keys
    for k in sorted(keys):
        got, want = jk['leave_one_out'][k], loo[k]
        assert got.shape == (40,) and np.array_equal(np.isnan(got), w == 0)
        dev = np.nanmax(np.abs(got - want) / np.abs(want))
        print('%s %s %s: leave-one-out %.1e, error %.6e against %.6e, corrected %.6e against %.6e' % (kind, name, k, dev, jk['error'][k], err[k],
                                                                                                      jk['bias_corrected'][k], corr[k]))
        assert np.allclose(got[w > 0], want[w > 0], rtol=1e-12, atol=0.0)
        assert jk['estimate'][k] == pytest.approx(est[k], rel=1e-12)
        assert jk['error'][k] == pytest.approx(err[k], rel=1e-12)
        assert jk['bias_corrected'][k] == pytest.approx(corr[k], rel=1e-12)
        assert jk['error'][k] > 0


@pytest.mark.parametrize('kind', KINDS)
def test_jackknife_float_weights(cases, kind):
    """Weights over 12 decades: a quantised weight is off by at most 2^-33 of the largest, P by at most K 2^-31 per bin (the bound of the
    overlap pipeline), a moment with |q| <= 1 by at most that summed over the n + 1 bins."""
    X, w, jk, (est, loo, _, _), K = cases[kind, 'float']
    bound = (X.shape[1] + 1) * K * 2.0 ** -31
    assert np.count_nonzero(w == 0) >= 2 and w[w > 0].max() / w[w > 0].min() > 1e9
    for k in FOUR:
        got, want = jk['leave_one_out'][k], loo[k]
        assert np.array_equal(np.isnan(got), w == 0)
        dev = max(float(np.nanmax(np.abs(got - want))), abs(jk['estimate'][k] - est[k]))
        print('%s float %s: largest deviation %.2e, bound %.2e' % (kind, k, dev, bound))
        assert dev <= bound


# ---------------------------------------------------------------------------------------------- 2. the estimate is the trusted one
@pytest.mark.parametrize('kind', KINDS)
def test_estimate_is_moments_of_the_distribution(cases, kind):
    for name in ('uniform', 'integer', 'float'):
        X, w, jk, _, K = cases[kind, name]
        want = rref.moments_ref(X, w, kind)
        for k in want:
            if name == 'float':
                if k in FOUR:
                    assert abs(jk['estimate'][k] - want[k]) <= (X.shape[1] + 1) * K * 2.0 ** -31
            else:
                assert jk['estimate'][k] == pytest.approx(want[k], rel=1e-12)


def test_state_means_and_dropped_rows():
    """state_q of sample s is the mean overlap with all other samples; a sample whose row was dropped leaves the estimate unchanged."""
    rng = np.random.default_rng(3)
    X = (rng.random((12, 30)) < 0.6).astype(np.uint8)
    X[5] = X[2]
    w = rng.integers(1, 4, 12).astype(np.float64)
    R, wq, scale, inv, n = rref.class_rowsums(X, w, 'spin')
    jk = ov.jackknife(R, wq, scale, inv, w, n, 'spin')
    S = 2.0 * X - 1.0
    Qm = S @ S.T / n
    for s in range(12):
        o = np.arange(12) != s
        assert jk['state_q'][s] == pytest.approx(np.sum(w[o] * Qm[s, o]) / w[o].sum(), rel=1e-12)
        assert jk['state_q2'][s] == pytest.approx(np.sum(w[o] * Qm[s, o] ** 2) / w[o].sum(), rel=1e-12)
    # drop the class of sample 7 by hand: its sample still counts, with theta^(-s) = theta
    keep = np.arange(len(R)) != inv[7]
    assert np.count_nonzero(inv == inv[7]) == 1
    X2, w2 = X[np.arange(12) != 7], w[np.arange(12) != 7]
    R2, wq2, _, inv2, _ = rref.class_rowsums(X2, w2, 'spin')
    assert len(R2) == int(keep.sum())
    inv_d = np.insert(inv2, 7, -1)
    jd = ov.jackknife(R2, wq2, 1.0, inv_d, w, n, 'spin')
    base = ov.jackknife(R2, wq2, 1.0, inv2, w2, n, 'spin')
    assert jd['estimate'] == base['estimate'] and np.isnan(jd['state_q'][7])
    assert jd['leave_one_out']['q2'][7] == jd['estimate']['q2']
    assert np.array_equal(np.delete(jd['leave_one_out']['q2'], 7), base['leave_one_out']['q2'])


# ---------------------------------------------------------------------------------------------- 3. calibration on independent draws
def rowsums_int64(bits):
    """The six sums of every row of (M, n) bits under unit weights in int64 (M n^4 < 2^63): the diagonal has d = 0, so it enters the
    entries 0 and 5 only, where it is taken out."""
    M, n = bits.shape
    S = 2 * bits.astype(np.int64) - 1
    D = (n - S @ S.T) // 2
    R = np.stack([np.full(M, M - 1)] + [(D ** k).sum(1) for k in (1, 2, 3, 4)] + [np.abs(n - 2 * D).sum(1) - n], axis=1)
    return [[int(v) for v in row] for row in R]


def test_calibration_on_iid_bits():
    """iid bits with P(1) = 0.7, M = 128, n = 64, 300 repetitions: the mean of error^2 over the empirical variance of the estimate lies in
    [0.8, 1.5] (the band leaves about twice the sampling spread of a variance from 300 repetitions)."""
    rng = np.random.default_rng(1)
    M, n, reps = 128, 64, 300
    keys = ('q', 'q2', 'q4', 'binder')
    est, err2 = {k: [] for k in keys}, {k: [] for k in keys}
    for _ in range(reps):
        bits = (rng.random((M, n)) < 0.7).astype(np.uint8)
        assert np.unique(bits, axis=0).shape[0] == M
        jk = ov.jackknife(rowsums_int64(bits), np.ones(M, dtype=np.uint32), 1.0, np.arange(M), np.ones(M), n, 'spin')
        for k in keys:
            est[k].append(jk['estimate'][k])
            err2[k].append(jk['error'][k] ** 2)
    for k in keys:
        ratio = float(np.mean(err2[k]) / np.var(est[k], ddof=1))
        print('%s: mean error^2 / variance of the estimate = %.3f' % (k, ratio))
        assert 0.8 <= ratio <= 1.5, (k, ratio)


def test_rowsums_int64_is_the_reference():
    bits = (np.random.default_rng(2).random((20, 64)) < 0.7).astype(np.uint8)
    R = rref.pair_rowsums_ref(ov.pack_bits(bits), 64)
    assert rowsums_int64(bits) == R
    # limbs and back, both limbs in use and the sign bit of each set
    big = [[(v << 70) + (1 << 127) + (1 << 63) + v for v in row] for row in R]
    assert ov.rowsums_to_int(rref.limbs(R)) == R and ov.rowsums_to_int(rref.limbs(big).view(np.int64)) == big
    with pytest.raises(ValueError):
        ov.rowsums_to_int(np.zeros((3, 5, 2), dtype=np.int64))


# ---------------------------------------------------------------------------------------------- 4. refusals, before any device work
def test_public_call_refusals(monkeypatch):
    from tnac4o_amd import ops
    monkeypatch.setattr(ops, 'pair_rowsums', lambda *a, **k: pytest.fail('device work before a refusal'))
    s = droplet()
    with pytest.raises(ValueError):                                    # no states
        s.calculate_overlap_errors()
    s.states = np.random.default_rng(4).integers(0, 256, (2, 16)).astype(s.indtype)
    with pytest.raises(ValueError, match='three'):                     # two states have one pair and no jackknife
        s.calculate_overlap_errors()
    s.states = np.random.default_rng(4).integers(0, 256, (5, 16)).astype(s.indtype)
    with pytest.raises(ValueError, match='three'):                     # ... as have two states with weight
        s.calculate_overlap_errors(weights=[1, 0, 0, 2, 0])
    with pytest.raises(ValueError):
        s.calculate_overlap_errors(kind='bond')
    with pytest.raises(ValueError):
        s.calculate_overlap_errors(weights='boltzmann')
    with pytest.raises(ValueError):                                    # no sample_log2Z
        s.calculate_overlap_errors(weights='importance')
    for bad in (np.ones(4), [1, 1, -1, 1, 1], [1, 1, np.nan, 1, 1], np.zeros(5)):
        with pytest.raises(ValueError):
            s.calculate_overlap_errors(weights=bad)
    r = rmf()
    r.states = np.zeros((5, 9), dtype=r.indtype)
    for kind in ('spin', 'link'):
        with pytest.raises(ValueError):
            r.calculate_overlap_errors(kind=kind)
    r.states = np.zeros((3, ov.MAX_ROWSUM_NBITS + 1), dtype=np.int8)
    with pytest.raises(NotImplementedError, match=str(ov.MAX_ROWSUM_NBITS)):
        r.calculate_overlap_errors()
    for x in (s, r):
        assert not hasattr(x, 'overlap_errors') and not hasattr(x, 'overlap_error_kind') and not hasattr(x, 'overlap_ess')
    with pytest.raises(ValueError, match='three'):
        ov.jackknife([[0] * 6] * 2, np.ones(2, dtype=np.uint32), 1.0, np.arange(2), np.ones(2), 4, 'spin')


def test_one_distinct_row_needs_no_launch(monkeypatch):
    from tnac4o_amd import ops
    monkeypatch.setattr(ops, 'pair_rowsums', lambda *a, **k: pytest.fail('a launch for one distinct row'))
    s = droplet()
    s.states = np.tile(np.random.default_rng(5).integers(0, 256, (1, 16)), (6, 1)).astype(s.indtype)
    for kind in KINDS:
        err = s.calculate_overlap_errors(kind)
        assert err is s.overlap_errors and s.overlap_error_kind == kind and not any(err.values())
        assert s.overlap_error_estimates['q'] == 1.0 and s.overlap_error_estimates['binder'] == 1.0
        assert s.overlap_bias_corrected['q2'] == 1.0 and np.array_equal(s.overlap_state_q, np.ones(6)) and s.overlap_ess == pytest.approx(6.0)
    assert not hasattr(s, 'overlap_distribution') and not hasattr(s, 'overlap_moments') and not hasattr(s, 'overlap_kind')


# ---------------------------------------------------------------------------------------------- argument errors of the export
def test_pair_rowsums_argument_errors(monkeypatch):
    """rc < 0 with a message and nothing launched: the pointers below are not device memory, they are never followed."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv('TN_PAIR_ROWSUMS_WGS', raising=False)
    p = 4096                                                           # stands for a non-null pointer
    M, nbits = 300, 130
    need = int(L.tn_pair_rowsums_ws_bytes(M, nbits, 0))
    assert need >= M * 6 * 16 and need % 16 == 0
    for args in ((None, M, nbits, 3, None, 0, p, p, need, None), (p, M, nbits, 3, None, 0, None, p, need, None),
                 (p, M, nbits, 3, None, 0, p, None, need, None)):
        assert L.tn_pair_rowsums(*args) == -1
        assert 'null operand' in last_error(L)
    assert L.tn_pair_rowsums(p, M, nbits, 2, None, 0, p, p, need, None) == -1       # three words per row
    assert 'ldr' in last_error(L)
    assert L.tn_pair_rowsums(p, M, 5, 1, None, 1, p, p, need, None) == -1           # five lanes take two words
    assert 'ldr' in last_error(L)
    assert L.tn_pair_rowsums(p, -1, nbits, 3, None, 0, p, p, need, None) == -1
    assert L.tn_pair_rowsums(p, 2 ** 31, nbits, 3, None, 0, p, p, need, None) == -1
    assert '2^31' in last_error(L)
    assert L.tn_pair_rowsums(p, M, 0, 3, None, 0, p, p, need, None) == -1
    assert int(L.tn_pair_rowsums_ws_bytes(65, ov.MAX_ROWSUM_NBITS, 0)) > 0
    assert int(L.tn_pair_rowsums_ws_bytes(65, ov.MAX_ROWSUM_NBITS + 1, 0)) == 0
    for lanes16 in (0, 1):
        assert L.tn_pair_rowsums(p, 65, ov.MAX_ROWSUM_NBITS + 1, 1 << 14, None, lanes16, p, p, 1 << 30, None) == -1
        assert str(ov.MAX_ROWSUM_NBITS) in last_error(L)
    assert L.tn_pair_rowsums(p, M, nbits, 3, None, 0, p, p, need - 1, None) == -3
    assert 'workspace too small' in last_error(L)
    # the size of the workspace follows the switch: one slab per segment of the column blocks
    monkeypatch.setenv('TN_PAIR_ROWSUMS_WGS', '1')
    assert int(L.tn_pair_rowsums_ws_bytes(M, nbits, 0)) == M * 6 * 16
    monkeypatch.setenv('TN_PAIR_ROWSUMS_WGS', '7')
    assert int(L.tn_pair_rowsums_ws_bytes(M, nbits, 0)) == 2 * M * 6 * 16
