"""Host side of tnac4o.calculate_overlap_distribution (tnac4o_amd/overlap.py) and the argument errors of tn_pair_hist.  No GPU."""
import numpy as np
import pytest

import golden_inputs as gi
import overlap_ref as oref
from overlap_ref import droplet, last_error, rmf
from tnac4o_amd import overlap as ov


# ---------------------------------------------------------------------------------------------- packers
def test_pack_bits_layout():
    for n, nwords in ((1, 1), (63, 1), (64, 1), (65, 2), (130, 3)):
        bits = np.zeros((n + 1, n), dtype=np.int8)
        for i in range(n):
            bits[i, i] = 1                                     # row i: bit i alone; the last row: nothing
        rows = ov.pack_bits(bits)
        assert rows.dtype == np.uint64 and rows.shape == (n + 1, nwords)
        for i in (0, 63, 64, n - 1):
            if i < n:
                want = np.zeros(nwords, dtype=np.uint64)
                want[i // 64] = np.uint64(1) << np.uint64(i % 64)
                assert np.array_equal(rows[i], want), (n, i)
        assert not rows[n].any()
    full = ov.pack_bits(np.ones((1, 65), dtype=np.int64))
    assert int(full[0, 0]) == 2 ** 64 - 1 and int(full[0, 1]) == 1       # nothing beyond n is set
    with pytest.raises(ValueError):
        ov.pack_bits(np.array([[0, 2]]))
    rng = np.random.default_rng(0)
    b = rng.integers(0, 2, (7, 200))
    assert np.array_equal(oref.unpack_rows(ov.pack_bits(b), 200, False), b)


def test_pack_lanes16_layout():
    st = np.array([[1, 2, 3, 32767, 5, 6]])
    rows = ov.pack_lanes16(st)
    assert rows.dtype == np.uint64 and rows.shape == (1, 2)
    assert int(rows[0, 0]) == 1 | (2 << 16) | (3 << 32) | (32767 << 48)
    assert int(rows[0, 1]) == 5 | (6 << 16)                              # the last lane; the lanes beyond stay 0
    assert ov.pack_lanes16(np.zeros((3, 4), dtype=np.int8)).shape == (3, 1)
    assert ov.pack_lanes16(np.zeros((3, 5), dtype=np.int16)).shape == (3, 2)
    for bad in ([[32768]], [[-1]]):
        with pytest.raises(ValueError):
            ov.pack_lanes16(np.array(bad))
    rng = np.random.default_rng(1)
    s = rng.integers(0, 32768, (5, 11))
    assert np.array_equal(oref.unpack_rows(ov.pack_lanes16(s), 11, True), s)


# ---------------------------------------------------------------------------------------------- bits of a solver
def test_spin_and_link_bits_on_the_droplet_instance():
    s = droplet()
    rng = np.random.default_rng(2)
    s.states = rng.integers(0, 256, (6, 16)).astype(s.indtype)
    # the couplings: every i < j with a non-zero accumulated J, sorted -- the bond_pairs of model_correlations
    acc = {}
    for i, j, v in gi.droplet_J(128, 1):
        i, j = int(i), int(j)
        if i != j:
            key = (min(i, j), max(i, j))
            acc[key] = acc.get(key, 0.0) + v
    want = sorted(k for k, v in acc.items() if v != 0)
    pairs = ov.link_pairs(s.J0)
    assert pairs.shape == (len(want), 2) and [tuple(p) for p in pairs.tolist()] == want
    b = s.binary_states()
    lb = ov.link_bits(s)
    assert lb.shape == (6, len(want))
    for k in (0, 5):
        assert lb[k].tolist() == [int(b[k, i] == b[k, j]) for i, j in want]
    sb = ov.spin_bits(s)
    assert sb.shape == (6, s.active) and s.active == 128 and np.array_equal(sb, b)
    # the global flip: every spin bit turns, no link bit does
    flipped = droplet()
    flipped.states = (255 - s.states.astype(np.int64)).astype(s.indtype)
    assert np.array_equal(ov.spin_bits(flipped), 1 - sb)
    assert np.array_equal(ov.link_bits(flipped), lb)
    # an inactive spin is left out
    import marginals_ref as mr
    import tnac4o_amd
    t = tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=1.0)
    t.states = rng.integers(0, 2, (4, 9)).astype(t.indtype)
    assert t.active == 17 and ov.spin_bits(t).shape == (4, 17)
    assert np.array_equal(ov.spin_bits(t), np.delete(t.binary_states(), 9, axis=1))
    for f in (ov.spin_bits, ov.link_bits):
        with pytest.raises(ValueError):
            f(rmf())


# ---------------------------------------------------------------------------------------------- condense / quantise
def test_condense_identity_in_exact_integers():
    """Brute-force integer histogram of all rows = histogram of the distinct rows with the aggregated weights + the self term in bin 0."""
    rng = np.random.default_rng(3)
    nbits = 100
    base = ov.pack_bits(rng.integers(0, 2, (260, nbits)))
    rows = np.concatenate([base, base[rng.integers(0, 260, 40)]])            # 300 rows, 40 of them duplicates
    rows = rows[rng.permutation(300)]
    w = rng.integers(1, 2 ** 20, 300)                                          # W_c^2 and every product stay below 2^53: float64 is exact
    full = oref.pair_hist_ref(rows, nbits, w, False)
    urows, W, D0 = ov.condense(rows, w)
    assert urows.shape[0] <= 260 and W.sum() == w.sum()
    assert np.all(W == np.rint(W)) and D0 == int(D0) and D0 > 0
    cond = oref.pair_hist_ref(urows, nbits, [int(x) for x in W], False)
    cond[0] += int(D0)
    assert cond == full
    assert cond[0] == int(D0)                                                   # distinct rows never land in bin 0
    # the self term by its definition
    inv = [tuple(r) for r in rows.tolist()]
    self_pairs = sum(int(w[a]) * int(w[b]) for a in range(300) for b in range(a + 1, 300) if inv[a] == inv[b])
    assert self_pairs == int(D0)


def test_quantise():
    full = 2 ** 32 - 1
    # integers pass through: multiplicities stay exact, zero weights are dropped
    wq, keep, scale = ov.quantise(np.array([3.0, 1.0, 0.0, 2.0 ** 32 - 1]))
    assert wq.dtype == np.uint32 and wq.tolist() == [3, 1, 0, full] and keep.tolist() == [True, True, False, True] and scale == 1.0
    # an integer above 2^32 - 1 is scaled: the power of two, 1 / 2, would lose the small weight, the full scale keeps it
    wq, keep, scale = ov.quantise(np.array([2.0 ** 32, 1.0, 0.0]))
    assert scale == full / 2.0 ** 32 and wq.tolist() == [full, 1, 0] and keep.tolist() == [True, True, False]
    # real weights: one of the two scales, the total rounding error within K half units of the full scale, rows that round to 0 dropped
    W = np.array([0.3, 0.7, 1e-3, 0.7 * 1e-11, 0.7 * 3e-10])
    wq, keep, scale = ov.quantise(W)
    assert scale in (full / 0.7, 2.0 ** 32) and wq.max() <= full
    assert np.all(wq == np.rint(W * scale))
    assert np.sum(np.abs(wq / scale - W)) <= W.size * 0.5 * 0.7 / full
    assert keep.tolist() == [True, True, True, False, True] and wq[3] == 0 and wq[4] == 1
    # multiplicities of nearly equal weights: the power of two keeps them apart by exact factors
    rng = np.random.default_rng(8)
    c = rng.integers(1, 700, 3000).astype(np.float64)
    c[0] = 666.0
    W = c * (1.0 - 1e-12 * rng.random(3000))
    wq, keep, scale = ov.quantise(W)
    assert scale == 2.0 ** 22 and np.array_equal(wq, c * scale) and keep.all()
    wq, keep, scale = ov.quantise(np.zeros(0))
    assert wq.size == 0 and keep.size == 0


def test_prepare_is_condense_quantise_keep():
    """prepare, which the three drivers call, returns exactly what the sequence they wrote out returns: the droplet rows with
    duplicates under uniform weights and under float weights with zeros and with values that quantise to 0, at the full wmax and
    at a smaller one."""
    rng = np.random.default_rng(11)
    s = droplet()
    w = 10.0 ** rng.uniform(-12.0, 0.0, 2048)
    w[::3] = 0.0
    for distinct, weights in ((60, np.ones(2048)), (700, w)):
        s.states = oref.states_with_duplicates(2048, rng, distinct).astype(np.uint8).astype(s.indtype)
        for kind in ('spin', 'cell'):
            rows = ov.rows_of(s, kind)[0]
            for wmax in (ov.WMAX, ov.WMAX // 128, 5):
                urows, W, D0 = ov.condense(rows, weights)
                wq, keep, scale = ov.quantise(W, wmax)
                if weights is w:
                    assert (W == 0).any() and (wq[W > 0] == 0).any() and 2 <= keep.sum() < keep.size
                got = ov.prepare(rows, weights, wmax)
                assert len(got) == 4 and got[2] == scale and got[3] == D0
                assert np.array_equal(got[0], urows[keep]) and got[0].dtype == np.uint64 and got[0].flags['C_CONTIGUOUS']
                assert np.array_equal(got[1], wq[keep]) and got[1].dtype == np.uint32 and got[1].flags['C_CONTIGUOUS']
    got, want = ov.prepare(rows, w), ov.quantise(ov.condense(rows, w)[1])           # wmax defaults to 2^32 - 1
    assert np.array_equal(got[1], want[0][want[1]]) and got[2] == want[2]


# ---------------------------------------------------------------------------------------------- distribution / moments
def test_distribution_and_moments_by_hand():
    """Three rows of 4 bits, 0000 (weight 1), 0011 (weight 2), 1111 (weight 3): distances 2, 4, 2 with products 2, 3, 6."""
    bits = np.array([[0, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1]])
    w = [1, 2, 3]
    hist = oref.pair_hist_ref(ov.pack_bits(bits), 4, w, False)
    assert hist == [0, 0, 8, 0, 3]
    P = ov.distribution(oref.limbs(hist), 1.0, 0.0)
    assert np.array_equal(P, np.array([0, 0, 8, 0, 3]) / 11.0)
    # a scale and a self term: integers of weights 10 x as large, 5.5 in bin 0
    P2 = ov.distribution(oref.limbs([100 * h for h in hist]), 10.0, 5.5)
    assert np.allclose(P2, np.array([5.5, 0, 8, 0, 3]) / 16.5, rtol=1e-15, atol=0)
    # the high limb counts 2^64
    P3 = ov.distribution(np.array([[0, 1], [0, 0], [0, 3]], dtype=np.uint64), 1.0, 0.0)
    assert np.array_equal(P3, [0.25, 0.0, 0.75])
    # limbs as a signed tensor would hand them over
    assert ov.limbs_to_int(np.array([[-1, 1]], dtype=np.int64)) == [(2 ** 64 - 1) + 2 ** 64]
    with pytest.raises(ValueError):
        ov.distribution(np.zeros((3, 2), dtype=np.uint64), 1.0, 0.0)
    values = ov.overlap_values('spin', 4)
    assert values.tolist() == [1.0, 0.5, 0.0, -0.5, -1.0]
    assert ov.overlap_values('cell', 4).tolist() == [1.0, 0.75, 0.5, 0.25, 0.0]
    m = ov.moments(values, P)
    assert m['q'] == pytest.approx(-3 / 11) and m['abs_q'] == pytest.approx(3 / 11)
    assert m['q2'] == pytest.approx(3 / 11) and m['q4'] == pytest.approx(3 / 11)
    assert m['binder'] == pytest.approx(0.5 * (3 - (3 / 11) / (3 / 11) ** 2))
    assert ov.effective_sample_size([1, 2, 3]) == pytest.approx(36 / 14)
    assert ov.effective_sample_size(np.ones(50)) == pytest.approx(50)


# ---------------------------------------------------------------------------------------------- the public call refuses ...
def test_public_call_value_errors():
    s = droplet()
    with pytest.raises(ValueError):                                    # no states
        s.calculate_overlap_distribution()
    s.states = np.zeros((1, 16), dtype=s.indtype)
    with pytest.raises(ValueError):                                    # one state has no pair
        s.calculate_overlap_distribution()
    s.states = np.random.default_rng(4).integers(0, 256, (5, 16)).astype(s.indtype)
    with pytest.raises(ValueError):
        s.calculate_overlap_distribution(kind='bond')
    with pytest.raises(ValueError):
        s.calculate_overlap_distribution(weights='boltzmann')
    with pytest.raises(ValueError):                                    # no sample_log2Z
        s.calculate_overlap_distribution(weights='importance')
    s.sample_log2Z = np.zeros(4)
    with pytest.raises(ValueError):                                    # ... of another length
        s.calculate_overlap_distribution(weights='importance')
    for bad in (np.ones(4), np.ones((5, 1)), [1, 1, -1, 1, 1], [1, 1, np.nan, 1, 1], [1, np.inf, 1, 1, 1], np.zeros(5), ['a'] * 5):
        with pytest.raises(ValueError):
            s.calculate_overlap_distribution(weights=bad)
    r = rmf()
    r.states = np.zeros((5, 9), dtype=r.indtype)
    for kind in ('spin', 'link'):
        with pytest.raises(ValueError):
            r.calculate_overlap_distribution(kind=kind)
    assert not hasattr(s, 'overlap_distribution') and not hasattr(r, 'overlap_kind')


def test_public_call_names_the_lds_limit():
    r = rmf()
    r.states = np.zeros((2, ov.MAX_NBITS + 1), dtype=np.int8)
    with pytest.raises(NotImplementedError, match=str(ov.MAX_NBITS)):
        r.calculate_overlap_distribution()


# ---------------------------------------------------------------------------------------------- argument errors of the export
def test_pair_hist_argument_errors():
    """rc < 0 with a message and nothing launched: the pointers below are not device memory, they are never followed."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    p = 4096                                                           # stands for a non-null pointer
    M, nbits = 300, 130
    need = int(L.tn_pair_hist_ws_bytes(M, nbits, 0))
    assert need >= (nbits + 1) * 16 and need % 16 == 0
    for args in ((None, M, nbits, 3, None, 0, p, p, need, None), (p, M, nbits, 3, None, 0, None, p, need, None),
                 (p, M, nbits, 3, None, 0, p, None, need, None)):
        assert L.tn_pair_hist(*args) == -1
        assert 'null operand' in last_error(L)
    assert L.tn_pair_hist(p, M, nbits, 2, None, 0, p, p, need, None) == -1          # three words per row
    assert 'ldr' in last_error(L)
    assert L.tn_pair_hist(p, M, 5, 1, None, 1, p, p, need, None) == -1              # five lanes take two words
    assert 'ldr' in last_error(L)
    assert L.tn_pair_hist(p, -1, nbits, 3, None, 0, p, p, need, None) == -1
    assert L.tn_pair_hist(p, M, 0, 3, None, 0, p, p, need, None) == -1
    # the LDS limit: the largest nbits has a workspace size, one more is refused by name
    assert int(L.tn_pair_hist_ws_bytes(65, ov.MAX_NBITS, 0)) > 0
    assert int(L.tn_pair_hist_ws_bytes(65, ov.MAX_NBITS + 1, 0)) == 0
    for lanes16 in (0, 1):
        assert L.tn_pair_hist(p, 65, ov.MAX_NBITS + 1, 4096, None, lanes16, p, p, 1 << 30, None) == -1
        msg = last_error(L)
        assert str(ov.MAX_NBITS) in msg and 'LDS' in msg, msg
    assert L.tn_pair_hist(p, M, nbits, 3, None, 0, p, p, need - 1, None) == -3
    assert 'workspace too small' in last_error(L)
    assert L.tn_pair_hist(p, M, nbits, 3, None, 0, p, p, 0, None) == -3
