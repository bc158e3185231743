"""Host side of temper_samples(measure=) (tnac4o_amd/ladder.py) and the numpy reference tests/ladder_ref.py, no GPU: the schedule and
its time bins, every refusal, pairs_in_halves, the reference against brute force on +-1 spins, the moments and the bin jackknife on a
hand-made histogram, and the sum rule of a histogram."""
import numpy as np
import pytest

import ladder_ref as lr
import temper_ref as tr
from overlap_ref import droplet, ising3x3, rmf
from tnac4o_amd import ladder
from tnac4o_amd import overlap
from tnac4o_amd import temper as tp


# ---------------------------------------------------------------------------------------------- schedule
@pytest.mark.parametrize('rounds,every,start,nbins', [(7, 2, 1, 2), (10, 1, 0, 16), (10, 3, 0, 2), (10, 3, 4, 5), (9, 4, 1, 1), (100, 7, 13, 5), (5, 5, 0, 3)])
def test_schedule_and_bins(rounds, every, start, nbins):
    """ladder.schedule against the rule restated round by round: the rounds, n_meas = (rounds - measure_from) // measure, the bins
    i B // n_meas with B = min(measure_bins, n_meas) (B > n_meas included), bins non-decreasing and all used."""
    after, bins, B = ladder.schedule(rounds, every, start, nbins)
    plan, Bref = lr.schedule(rounds, every, start, nbins)
    assert [(int(r), int(b)) for r, b in zip(after, bins)] == plan and B == Bref
    n = (rounds - start) // every
    assert after.size == n and B == min(nbins, n) and after.max() < rounds and after.min() >= start
    assert np.all(np.diff(bins) >= 0) and sorted(set(bins.tolist())) == list(range(B))
    assert ladder.schedule(7, 2, 1, 2)[0].tolist() == [2, 4, 6] and ladder.schedule(7, 2, 1, 2)[1].tolist() == [0, 0, 1]


def test_schedule_refusals():
    for args, word in (((4, 0), 'measure'), ((4, -1), 'measure'), ((4, 1.5), 'measure'), ((4, True), 'measure'), ((4, 1, -1), 'measure_from'),
                       ((4, 1, 5), 'measure_from'), ((4, 1, 0.5), 'measure_from'), ((4, 1, 0, 0), 'measure_bins'), ((4, 5), 'no measurement'),
                       ((4, 2, 3), 'no measurement'), ((4, 1, 4), 'no measurement'), ((0, 1), 'no measurement')):
        with pytest.raises(ValueError, match=word):
            ladder.schedule(*args)


def test_block_ends():
    """The blocks of temper_native: without a measurement the cut of rounds_per_call alone; with one, an end behind every measurement
    round and never a block longer than rounds_per_call."""
    assert ladder.block_ends(0, 3, None) == [0] and ladder.block_ends(7, 3, None) == [3, 6, 7] and ladder.block_ends(6, 3, None) == [3, 6]
    after = ladder.schedule(7, 2, 1, 2)[0]
    assert ladder.block_ends(7, 7, after) == [3, 5, 7] and ladder.block_ends(7, 1, after) == [1, 2, 3, 4, 5, 6, 7]
    assert ladder.block_ends(7, 2, after) == [2, 3, 5, 7]
    ends = ladder.block_ends(100, 6, ladder.schedule(100, 7, 13, 5)[0])
    assert ends[-1] == 100 and max(np.diff([0] + ends)) <= 6 and all(int(r) + 1 in ends for r in ladder.schedule(100, 7, 13, 5)[0])


# ---------------------------------------------------------------------------------------------- refusals of the public call
def test_public_call_refusals():
    """Every ValueError and NotImplementedError of measure=, before any device work (this test has no device)."""
    s = droplet()
    s.states = np.random.default_rng(4).integers(0, 256, (8, 16)).astype(s.indtype)
    kept = np.copy(s.states)
    betas = [0.5, 1.0]
    for kw, word in ((dict(measure=0), 'measure'), (dict(measure=-2), 'measure'), (dict(measure=1.5), 'measure'), (dict(measure=11), 'no measurement'),
                     (dict(measure=1, measure_from=-1), 'measure_from'), (dict(measure=1, measure_from=11), 'measure_from'),
                     (dict(measure=1, measure_from=10), 'no measurement'), (dict(measure=1, measure_bins=0), 'measure_bins'),
                     (dict(measure=1, measure_pairs='some'), 'measure_pairs'), (dict(measure=1, rounds=0), 'no measurement')):
        with pytest.raises(ValueError, match=word):
            s.temper_samples(betas, **kw)
    # 'halves' with cluster moves: the pairs must stay inside [0, 2) and [2, 4)
    crossing = np.array([[[0, 1], [2, 3]], [[0, 2], [1, 3]]])
    with pytest.raises(ValueError, match='halves'):
        s.temper_samples(betas, rounds=2, pairs=crossing, measure=1, measure_pairs='halves')
    a = tp.check_arguments(s, betas, 2, 1, True, None, crossing[:1].repeat(2, axis=0), None, None, None)
    m = ladder.check_arguments(s, a, 1, 0, 16, 'halves', True)
    assert (m['split'], m['B'], m['n_meas'], m['links']) == (2, 2, 2, True) and m['after'].tolist() == [0, 1] and m['bins'].tolist() == [0, 1]
    a = tp.check_arguments(s, betas, 2, 1, True, 5.0, crossing, None, None, None)       # no temperature makes cluster moves: nothing to cross
    assert ladder.check_arguments(s, a, 2, 0, 16, 'halves', False)['split'] == 2
    a = tp.check_arguments(s, betas, 2, 1, False, None, None, None, None, None)
    m = ladder.check_arguments(s, a, 1, 1, 16, 'all', False)
    assert (m['split'], m['B'], m['n_meas'], m['links']) == (0, 1, 1, False) and m['after'].tolist() == [1] and m['bins'].tolist() == [0]
    one = droplet()
    one.states = kept[:2]
    with pytest.raises(ValueError, match='two chains'):                  # R = 1
        one.temper_samples(betas, cluster_moves=False, measure=1)
    r = rmf()
    r.states = np.zeros((4, 9), dtype=r.indtype)
    with pytest.raises(ValueError, match='Ising'):
        r.temper_samples(betas, cluster_moves=False, measure=1)
    assert np.array_equal(s.states, kept) and not hasattr(s, 'temper_index') and not hasattr(s, 'temper_overlap_hist')


def test_limits_raise_not_implemented(monkeypatch):
    """Rows, link rows or chains above the kernel's limits: NotImplementedError naming the limit (the limits lowered to reach them on a
    small model); measure_links=False leaves the couplings out of the check."""
    assert ladder.MAX_NBITS == lr.MAX_NBITS == 38815
    s = droplet()
    s.states = np.random.default_rng(4).integers(0, 256, (8, 16)).astype(s.indtype)
    n, nl = int(overlap.active_spins(s).size), int(overlap.link_pairs(s.J0).shape[0])
    assert nl > n
    monkeypatch.setattr(ladder, 'MAX_NBITS', nl - 1)
    with pytest.raises(NotImplementedError, match='couplings'):
        s.temper_samples([0.5, 1.0], cluster_moves=False, measure=1)
    a = tp.check_arguments(s, [0.5, 1.0], 2, 1, False, None, None, None, None, None)
    assert ladder.check_arguments(s, a, 1, 0, 16, 'all', False)['links'] is False
    monkeypatch.setattr(ladder, 'MAX_NBITS', n - 1)
    with pytest.raises(NotImplementedError, match='active spins'):
        s.temper_samples([0.5, 1.0], cluster_moves=False, measure=1, measure_links=False)
    monkeypatch.setattr(ladder, 'MAX_NBITS', 38815)
    monkeypatch.setattr(ladder, 'MAX_CHAINS', 3)
    with pytest.raises(NotImplementedError, match='chains'):
        s.temper_samples([0.5, 1.0], cluster_moves=False, measure=1)


# ---------------------------------------------------------------------------------------------- pairs_in_halves
@pytest.mark.parametrize('R', [2, 3, 4, 5, 8, 11])
def test_pairs_in_halves(R):
    """(rounds, Pc, 2) int32 from numpy's global generator: every pair inside one half, no chain twice in a round (a valid pairing for
    exchange.check_pairs), as many pairs as the halves hold, different rounds differ."""
    from tnac4o_amd import exchange as ex
    np.random.seed(3)
    p = ladder.pairs_in_halves(6, R)
    h = R // 2
    assert p.dtype == np.int32 and p.shape == (6, h // 2 + (R - h) // 2, 2)
    assert np.all((p[..., 0] < h) == (p[..., 1] < h)) and np.all((p >= 0) & (p < R))
    for r in range(6):
        assert np.unique(p[r]).size == p[r].size
    assert np.array_equal(ex.check_pairs(p, 6, R), p)
    np.random.seed(3)
    assert np.array_equal(ladder.pairs_in_halves(6, R), p)
    if R >= 8:
        assert any(not np.array_equal(p[0], p[r]) for r in range(1, 6))
    with pytest.raises(ValueError):
        ladder.pairs_in_halves(2, 1)


def test_link_table_follows_link_bits():
    """ladder.link_table: overlap.link_pairs as row positions -- the link row built from the spin row by the reference equals
    1 - overlap.link_bits (the kernel's bit is [s_i != s_j]), so the distances of link rows are those of link_bits."""
    s = ising3x3()
    qs = s._cell_sizes()[s.order]                                        # model order
    s.states = np.random.default_rng(5).integers(0, qs[None, :], size=(6, qs.size)).astype(s.indtype)
    bits = overlap.spin_bits(s)
    n = bits.shape[1]
    links = ladder.link_table(s)
    assert links.dtype == np.int32 and links.shape == (overlap.link_pairs(s.J0).shape[0], 2) and np.all((links >= 0) & (links < n))
    rows = [sum(int(b) << p for p, b in enumerate(row)) for row in bits]
    lrows = lr.link_rows(rows, n, links)
    want = 1 - overlap.link_bits(s)
    assert [[(v >> l) & 1 for l in range(links.shape[0])] for v in lrows] == want.tolist()


# ---------------------------------------------------------------------------------------------- the reference against brute force
def test_reference_against_brute_force_spins():
    """On the synthetic Ising lattice: q n = sum_i s_i s'_i = n - 2 d for the spin histogram and q_l n_l = sum_links (s_i s_j)(s'_i s'_j)
    = n_l - 2 d_l for the link histogram, from +-1 spins, per temperature and with the split rule; a slot entry out of range drops
    its pairs; split = R counts nothing."""
    lat = tr.ising_lattice()
    rng = np.random.default_rng(11)
    qs = np.array([c['q'] for c in lat['cells']])
    T, R = 3, 5
    M = T * R
    states = rng.integers(0, qs[None, :], size=(M, 16))
    slot = np.array([rng.permutation(T) + c * T for c in range(R)])
    n = lat['nbits']
    links = np.argwhere(lat['J'] != 0).astype(np.int32)
    spins = 1 - 2 * np.array([[(int(states[m, k]) >> int(j)) & 1 for k, j in lat['bitcell']] for m in range(M)])      # s = +1 for state bit 0
    for split in (0, 1, 2, R):
        hs, hl = lr.measure(lat['cells'], states, slot, n, lat['bitcell'], links, split)
        ws, wl = np.zeros((T, n + 1), dtype=object), np.zeros((T, len(links) + 1), dtype=object)
        for t in range(T):
            for ca in range(R):
                for cb in range(ca + 1, R):
                    if split and not ca < split <= cb:
                        continue
                    a, b = spins[slot[ca, t]], spins[slot[cb, t]]
                    qn = int(a @ b)
                    ql = int(np.sum(a[links[:, 0]] * a[links[:, 1]] * b[links[:, 0]] * b[links[:, 1]]))
                    ws[t, (n - qn) // 2] += 1
                    wl[t, (len(links) - ql) // 2] += 1
        assert np.array_equal(hs, ws) and np.array_equal(hl, wl)
        assert [int(x) for x in hs.sum(axis=1)] == [len(lr.counted_pairs(R, split))] * T
    assert len(lr.counted_pairs(R, 0)) == 10 and len(lr.counted_pairs(R, 2)) == 6 and lr.counted_pairs(R, R) == []
    bad = slot.copy()
    bad[1, 0], bad[3, 2] = -1, M
    hs, _ = lr.measure(lat['cells'], states, bad, n, lat['bitcell'], None, 0)
    assert [int(x) for x in hs.sum(axis=1)] == [6, 10, 6]


def test_reference_accumulators():
    """add_hist wraps at 2^64 and reads its accumulator as unsigned; add_esums continues a pre-filled accumulator in the order of the
    kernel and skips slot entries out of range."""
    acc = np.array([[0, 2 ** 32 + 5, -1]], dtype=np.int64)
    got = lr.add_hist(acc, np.array([[1, 2 ** 32, 0]], dtype=object))
    assert got.dtype == np.uint64 and got.tolist() == [[1, 2 ** 33 + 5, 2 ** 64 - 1]]
    assert lr.add_hist(np.array([2 ** 64 - 4], dtype=np.uint64), [3]).tolist() == [2 ** 64 - 1]
    E = np.array([0.1, 0.2, 0.3, 1e16, -1e16, 0.7])
    slot = np.array([[0, 3], [1, 4], [2, 5]])
    out = lr.add_esums(np.array([[2.0, 0.5, 0.25], [0.0, 0.0, 0.0]]), slot, E, 6)
    assert out[0].tolist() == [3.0, 0.5 + ((0.1 + 0.2) + 0.3), 0.25 + ((0.1 * 0.1 + 0.2 * 0.2) + 0.3 * 0.3)]
    assert out[1].tolist() == [1.0, (1e16 + -1e16) + 0.7, (1e32 + 1e32) + 0.7 * 0.7]
    slot[1, 0] = 6
    assert lr.add_esums(np.zeros((2, 3)), slot, E, 6)[0].tolist() == [1.0, 0.1 + 0.3, 0.1 * 0.1 + 0.3 * 0.3]


# ---------------------------------------------------------------------------------------------- moments and the jackknife
def test_moments_and_bin_jackknife_on_a_hand_made_histogram():
    """n = 4 spins, T = 2, B = 3 bins.  Temperature 0: all weight at d = 0 and d = 4 (q = +-1): q2 = q4 = 1, binder = 1, chi_sg = 4 in
    every deletion, so the errors vanish.  Temperature 1: the moments by hand from the pooled counts, the errors from the delete-one
    formula written out."""
    h = np.zeros((3, 2, 5), dtype=np.int64)
    h[:, 0, 0], h[:, 0, 4] = [3, 1, 2], [1, 3, 2]
    h[0, 1], h[1, 1], h[2, 1] = [1, 2, 4, 2, 1], [0, 3, 4, 3, 0], [2, 2, 2, 2, 2]
    hl = np.zeros((3, 2, 3), dtype=np.int64)
    hl[:, 0], hl[:, 1] = [[4, 0, 0]] * 3, [[5, 3, 2], [5, 5, 0], [4, 2, 4]]

    class Box:
        pass

    s = Box()
    betas = np.array([0.5, 2.0])
    esums = np.zeros((3, 2, 3))
    esums[:, :, 0] = 2.0                                                 # two measurements per bin, R = 5 rows each
    esums[:, 0, 1], esums[:, 0, 2] = [-10.0, -20.0, -30.0], [20.0, 50.0, 100.0]
    esums[:, 1, 1], esums[:, 1, 2] = -40.0, 160.0                        # E = -4 always: no variance
    ladder.store(s, h, hl, esums, 6, 5, betas)
    assert s.temper_measurements == 6 and s.temper_overlap_hist is not None and s.temper_overlap_values.tolist() == [1.0, 0.5, 0.0, -0.5, -1.0]
    assert s.temper_link_values.tolist() == [1.0, 0.0, -1.0]
    assert np.allclose(s.temper_overlap_P.sum(axis=1), 1.0) and s.temper_overlap_P[0].tolist() == [0.5, 0, 0, 0, 0.5]
    m, e = s.temper_overlap_moments, s.temper_overlap_errors
    assert set(m) == set(e) == set(ladder.MOMENT_KEYS)
    assert (m['q'][0], m['abs_q'][0], m['q2'][0], m['q4'][0], m['binder'][0], m['chi_sg'][0], m['ql'][0]) == (0.0, 1.0, 1.0, 1.0, 1.0, 4.0, 1.0)
    for k in ('abs_q', 'q2', 'q4', 'binder', 'chi_sg', 'ql'):
        assert e[k][0] == 0.0
    assert e['q'][0] > 0
    q = np.array([1.0, 0.5, 0.0, -0.5, -1.0])
    tot = h[:, 1].sum(axis=0)
    P = tot / tot.sum()
    assert np.isclose(m['q2'][1], P @ q ** 2) and np.isclose(m['q4'][1], P @ q ** 4) and np.isclose(m['chi_sg'][1], 4 * (P @ q ** 2))
    assert np.isclose(m['binder'][1], 0.5 * (3 - (P @ q ** 4) / (P @ q ** 2) ** 2))
    ltot = hl[:, 1].sum(axis=0)
    assert np.isclose(m['ql'][1], (ltot[0] - ltot[2]) / ltot.sum())
    th = []
    for b in range(3):
        d = (tot - h[b, 1]) / (tot - h[b, 1]).sum()
        th.append(d @ q ** 2)
    th = np.array(th)
    assert np.isclose(e['q2'][1], np.sqrt(2.0 / 3.0 * np.sum((th - th.mean()) ** 2))) and e['q2'][1] > 0
    # energies: <E> = sum E / (measurements R), c = beta^2 (<E^2> - <E>^2) / n
    assert np.allclose(s.temper_energy_mean, [-60.0 / 30.0, -4.0]) and np.allclose(s.temper_heat_capacity, [0.25 * (170.0 / 30.0 - 4.0) / 4, 0.0])
    assert s.temper_heat_capacity_error[1] == 0.0 and s.temper_energy_mean_error[1] == 0.0
    em = np.array([(-60.0 + 10.0) / 20, (-60.0 + 20.0) / 20, (-60.0 + 30.0) / 20])
    assert np.isclose(s.temper_energy_mean_error[0], np.sqrt(2.0 / 3.0 * np.sum((em - em.mean()) ** 2)))
    # one bin: the estimates stay, the errors are NaN; no link histogram: ql is NaN and the link results are None
    ladder.store(s, h[:1], None, esums[:1], 2, 5, betas)
    assert all(np.all(np.isnan(v)) for v in s.temper_overlap_errors.values()) and np.all(np.isnan(s.temper_energy_mean_error))
    assert np.all(np.isnan(s.temper_overlap_moments['ql'])) and s.temper_overlap_moments['q2'][0] == 1.0
    assert s.temper_link_hist is None and s.temper_link_P is None and s.temper_link_values is None
    # the jackknife of a plain mean is the standard error of the bin means
    x = np.array([[1.0, 1.0], [3.0, 1.0], [8.0, 1.0]])                   # (sum, count) per bin
    assert np.isclose(ladder.jackknife(x, lambda s_: s_[0] / s_[1]), np.std([1.0, 3.0, 8.0], ddof=1) / np.sqrt(3))


def test_histogram_sum_rule():
    """Sum of a bin's histogram = (measurements in the bin) x (counted pairs), at every temperature: the reference walked over a static
    chain (sweeps = 0, no cluster move) with 'all' and with 'halves'."""
    lat = tr.ising_lattice()
    rng = np.random.default_rng(12)
    qs = np.array([c['q'] for c in lat['cells']])
    T, R, rounds = 2, 4, 7
    states = rng.integers(0, qs[None, :], size=(T * R, 16))
    plan, B = lr.schedule(rounds, 2, 1, 2)
    for split in (0, R // 2):
        _, spin, link, esums = lr.walk(lat['cells'], 4, 4, states, [0.3, 0.8], rounds, 0, None, None, T, None, None, rng.random((rounds, R, 1)),
                                      lat['nbits'], lat['bitcell'], np.argwhere(lat['J'] != 0), split, plan, B)
        per_bin = np.bincount([b for _, b in plan], minlength=B)
        pairs = len(lr.counted_pairs(R, split))
        assert per_bin.tolist() == [2, 1] and pairs == (6 if split == 0 else 4)
        assert np.array_equal(spin.sum(axis=2), np.outer(per_bin * pairs, np.ones(T, dtype=np.int64)))
        assert np.array_equal(link.sum(axis=2), spin.sum(axis=2)) and np.array_equal(esums[:, :, 0], np.outer(per_bin, np.ones(T)))
