"""Host side of tnac4o.calculate_state_linkage (tnac4o_amd/linkage.py) and the reference of tests/linkage_ref.py against brute force and
scipy; the driver's argument checks; the argument errors of tn_state_linkage.  No GPU."""
import numpy as np
import pytest

import linkage_ref as lr
from overlap_ref import droplet, ising3x3, last_error, rmf
from tnac4o_amd import linkage as lk
from tnac4o_amd import overlap as ov

# (M, nbits, lanes16, fold, alphabet): small random sets with many ties
SETS = [(1, 5, False, False, 2), (2, 1, False, False, 2), (9, 4, False, False, 2), (23, 7, False, True, 2), (24, 8, False, True, 2),
        (30, 6, True, False, 3), (40, 70, False, False, 2), (17, 3, False, False, 2)]


def tree(case):
    M, n, lanes16, fold, alphabet = case
    rows = lr.random_rows(M, n, 50 + M, lanes16, alphabet)
    D = lr.dense(rows, n, lanes16, fold)
    return D, lr.kruskal(D)


# ---------------------------------------------------------------------------------------------- the reference
def test_dense_distances_by_hand():
    rows = np.array([[0b0000], [0b0111], [0b1111], [0b1000]], dtype=np.uint64)
    assert lr.dense(rows, 4).tolist() == [[0, 3, 4, 1], [3, 0, 1, 4], [4, 1, 0, 3], [1, 4, 3, 0]]
    assert lr.dense(rows, 4, fold=True).tolist() == [[0, 1, 0, 1], [1, 0, 1, 0], [0, 1, 0, 1], [1, 0, 1, 0]]
    assert lr.dense(rows, 3).tolist() == [[0, 3, 3, 0], [3, 0, 0, 3], [3, 0, 0, 3], [0, 3, 3, 0]]        # bit 3 lies beyond nbits
    lanes = lr.pack([[1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [1, 7, 3, 4, 6], [0, 0, 0, 0, 0]], True)
    assert lanes.shape == (4, 2) and lr.dense(lanes, 5, True).tolist() == [[0, 0, 2, 5], [0, 0, 2, 5], [2, 2, 0, 5], [5, 5, 5, 0]]
    framed = lr.frame(lanes, 5, True, 3)
    assert framed.shape == (4, 3) and np.array_equal(lr.dense(framed, 5, True), lr.dense(lanes, 5, True)) and not np.array_equal(framed[:, :2], lanes)


@pytest.mark.parametrize('case', SETS, ids=lambda c: 'M%d-n%d' % c[:2])
def test_kruskal_equals_prim_and_the_nearest_row(case):
    D, (pairs, dist) = tree(case)
    M = D.shape[0]
    p_pairs, p_dist = lr.prim(D)
    assert np.array_equal(pairs, p_pairs) and np.array_equal(dist, p_dist)
    assert pairs.shape == (M - 1, 2) and np.all(pairs[:, 0] < pairs[:, 1])
    keys = [(int(d), int(a), int(b)) for (a, b), d in zip(pairs, dist)]
    assert keys == sorted(keys) and len(set(keys)) == M - 1
    nn, nd = lr.nearest(D)
    for a in range(M):
        want = min(((int(D[a, b]), b) for b in range(M) if b != a), default=(-1, -1))
        assert (int(nd[a]), int(nn[a])) == want
    if M >= 2:                                                           # the smallest edge of a row is a tree edge (the cut property)
        have = {(int(a), int(b)) for a, b in pairs}
        assert all((min(a, int(nn[a])), max(a, int(nn[a]))) in have for a in range(M))


def test_the_ruler_path():
    """Distances add along the path, so the tree is the path; Boruvka needs 3, 5 and 6 rounds for M = 8, 32, 64."""
    for M, rounds in ((8, 3), (32, 5), (64, 6)):
        rows, nbits = lr.ruler_rows(M)
        D = lr.dense(rows, nbits)
        pairs, dist = lr.kruskal(D)
        assert sorted(map(tuple, pairs.tolist())) == [(i - 1, i) for i in range(1, M)]
        assert np.array_equal(np.sort(dist), np.sort([1 + ((i & -i).bit_length() - 1) for i in range(1, M)]))
        assert lr.boruvka_rounds(D) == rounds
    assert lr.ruler_rows(64)[1] == 120


@pytest.mark.parametrize('case', SETS, ids=lambda c: 'M%d-n%d' % c[:2])
def test_labels_counts_and_matrix_of_the_driver(case):
    """The driver's host functions against the reference and against the explicit threshold graph, for every threshold."""
    D, (pairs, dist) = tree(case)
    M, n = D.shape[0], case[1]
    counts = lk.cluster_counts(dist, M, n)
    assert counts.dtype == np.int64 and np.array_equal(counts, lr.cluster_counts(dist, M, n))
    for t in range(n + 1):
        want = lr.threshold_components(D, t)
        got = lk.labels_at(pairs, dist, M, t)
        assert got.dtype == np.int64 and np.array_equal(got, want) and np.array_equal(lr.labels_at(pairs, dist, M, t), want)
        assert counts[t] == want.max() + 1
        sizes, first, rep, emin = lk.cluster_summary(got)
        assert rep is None and emin is None and np.array_equal(sizes, np.bincount(want))
        assert np.array_equal(first, [np.flatnonzero(want == k)[0] for k in range(len(sizes))]) and np.all(np.diff(first) > 0)
    Z = lk.linkage_matrix(pairs, dist, M)
    assert Z.dtype == np.float64 and Z.shape == (M - 1, 4) and np.array_equal(Z, lr.linkage_matrix(pairs, dist, M))
    assert np.all(Z[:, 0] < Z[:, 1]) and np.array_equal(Z[:, 2], dist) and (M < 2 or Z[-1, 3] == M)


def test_representatives():
    labels = np.array([0, 1, 0, 2, 1, 0])
    energy = np.array([3.0, -1.0, 2.0, 5.0, -1.0, 2.0])
    sizes, first, rep, emin = lk.cluster_summary(labels, energy)
    assert sizes.tolist() == [3, 2, 1] and first.tolist() == [0, 1, 3] and rep.tolist() == [2, 1, 3] and emin.tolist() == [2.0, -1.0, 5.0]


def test_a_cycle_is_refused():
    with pytest.raises(ValueError, match='cycle'):
        lk.linkage_matrix(np.array([[0, 1], [1, 2], [0, 2]]), np.array([1, 1, 2]), 4)


@pytest.mark.parametrize('case', [c for c in SETS if c[0] >= 3], ids=lambda c: 'M%d-n%d' % c[:2])
def test_against_scipy(case):
    hier = pytest.importorskip('scipy.cluster.hierarchy')
    from scipy.spatial.distance import squareform
    D, (pairs, dist) = tree(case)
    M, n = D.shape[0], case[1]
    Z = lk.linkage_matrix(pairs, dist, M)
    assert hier.is_valid_linkage(Z)
    S = hier.linkage(squareform(D.astype(np.float64), checks=False), method='single')
    assert np.array_equal(np.sort(S[:, 2]), Z[:, 2])
    for t in range(n + 1):
        assert lr.same_partition(hier.fcluster(Z, t, 'distance'), lk.labels_at(pairs, dist, M, t)), t


# ---------------------------------------------------------------------------------------------- the driver's argument checks
def test_check_arguments_and_packing():
    s = droplet()
    rng = np.random.default_rng(3)
    given = rng.integers(0, 256, (7, 16))
    s.states = given.astype(s.indtype)
    kind, sym, rows, n, lanes16 = lk.check_arguments(s, None, None, None, None)
    fields = bool(np.any(np.asarray(s.J0).diagonal() != 0))
    assert kind == 'spin' and sym == (not fields) and not lanes16 and n == ov.active_spins(s).size
    assert np.array_equal(rows, ov.pack_bits(ov.spin_bits(s)))
    again = lk.check_arguments(s, 3, 'spin', False, given[2:5])
    assert again[1] is False and np.array_equal(again[2], rows[2:5])
    kind, sym, crow, n, lanes16 = lk.check_arguments(s, np.int64(0), 'cell', None, None)
    assert kind == 'cell' and sym is False and lanes16 and n == 16 and np.array_equal(crow, ov.pack_lanes16(given))
    assert np.array_equal(lk.check_arguments(s, None, 'cell', False, given[::-1])[2], crow[::-1])
    r = rmf()
    r.states = np.zeros((5, 9), dtype=r.indtype)
    kind, sym, rows, n, lanes16 = lk.check_arguments(r, None, None, None, None)
    assert kind == 'cell' and sym is False and lanes16 and n == 9 and rows.shape == (5, 3)
    f = ising3x3()                                                       # symmetric=None follows the fields of the model
    f.states = np.zeros((2, 9), dtype=f.indtype)
    assert lk.check_arguments(f, None, None, None, None)[1] == (not np.any(np.asarray(f.J0).diagonal() != 0))


def test_public_call_value_errors():
    r = rmf()
    r.states = np.zeros((5, 9), dtype=r.indtype)
    with pytest.raises(ValueError, match='Ising'):
        r.calculate_state_linkage(kind='spin')
    with pytest.raises(ValueError, match='symmetric'):
        r.calculate_state_linkage(symmetric=True)
    s = droplet()
    with pytest.raises(ValueError, match='stored states'):
        s.calculate_state_linkage()
    given = np.random.default_rng(4).integers(0, 256, (5, 16))
    s.states = given.astype(s.indtype)
    kept = np.copy(s.states)
    with pytest.raises(ValueError, match='symmetric'):
        s.calculate_state_linkage(kind='cell', symmetric=True)
    for bad in (1, 'yes', 0.0):
        with pytest.raises(ValueError, match='symmetric'):
            s.calculate_state_linkage(symmetric=bad)
    for bad in ('link', 'spins', 3):
        with pytest.raises(ValueError, match='kind'):
            s.calculate_state_linkage(kind=bad)
    for bad in (-1, 1.5, True, '4', np.float64(2.0)):
        with pytest.raises(ValueError, match='threshold'):
            s.calculate_state_linkage(threshold=bad)
    for bad in (given.tolist(), given.astype(np.float64), given[0], given[:, :15], given[:0], np.full((2, 16), 256), np.full((2, 16), -1)):
        with pytest.raises(ValueError, match='states'):
            s.calculate_state_linkage(states=bad)
    assert np.array_equal(s.states, kept) and not hasattr(s, 'linkage_pairs') and not hasattr(s, 'state_cluster_labels')


def test_limits_are_named(monkeypatch):
    s = droplet()
    s.states = np.zeros((3, 16), dtype=s.indtype)
    monkeypatch.setattr(lk, 'MAX_STATES', 2)
    with pytest.raises(NotImplementedError, match='2\\^24'):
        s.calculate_state_linkage()
    monkeypatch.setattr(lk, 'MAX_STATES', 2 ** 24)
    monkeypatch.setattr(lk, 'MAX_ENTRIES', 15)
    with pytest.raises(NotImplementedError, match='at most 15'):
        s.calculate_state_linkage(kind='cell')
    assert not hasattr(s, 'linkage_pairs')


def test_store_from_given_edges():
    """Everything the call stores, from edges made by the reference (no device): a solver-like object."""
    class Box:
        pass
    case = SETS[3]
    D, (pairs, dist) = tree(case)
    M, n = D.shape[0], case[1]
    nn, nd = lr.nearest(D)
    energy = np.random.default_rng(1).integers(-3, 3, M).astype(np.float64)
    b = Box()
    ret = lk.store(b, 'spin', True, n, pairs, dist, nn, nd, 4, 2, energy)
    assert ret is b.linkage_distance and np.array_equal(b.linkage_pairs, pairs) and b.linkage_rounds == 4 and b.linkage_symmetric is True
    want = lr.threshold_components(D, 2)
    assert np.array_equal(b.state_cluster_labels, want) and np.array_equal(b.state_cluster_sizes, np.bincount(want))
    for k, rep in enumerate(b.state_cluster_representative):
        members = np.flatnonzero(want == k)
        assert rep == members[np.argmin(energy[members])] and b.state_cluster_energy_min[k] == energy[members].min()
    lk.store(b, 'spin', True, n, pairs, dist, nn, nd, 4, None, energy)
    assert all(getattr(b, a) is None for a in ('state_cluster_labels', 'state_cluster_sizes', 'state_cluster_first', 'state_cluster_representative',
                                               'state_cluster_energy_min'))
    lk.store(b, 'spin', True, n, pairs, dist, nn, nd, 4, 0, None)
    assert b.state_cluster_representative is None and b.state_cluster_energy_min is None and b.state_cluster_labels is not None


# ---------------------------------------------------------------------------------------------- argument errors of the export
def test_state_linkage_argument_errors():
    """rc = -1 with a message and nothing launched: the pointers below are not device memory, they are never followed."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    p = 4096                                                            # stands for a non-null pointer
    names = ('rows', 'M', 'nbits', 'ldr', 'lanes16', 'fold', 'nn_index', 'nn_dist', 'edge_lo', 'edge_hi', 'edge_dist', 'rounds', 'ws', 'ws_bytes')
    base = dict(rows=p, M=10, nbits=130, ldr=3, lanes16=0, fold=0, nn_index=p, nn_dist=p, edge_lo=p, edge_hi=p, edge_dist=p, rounds=p, ws=p, ws_bytes=0)

    def call(**kw):
        a = dict(base)
        a.update(kw)
        return L.tn_state_linkage(*[a[k] for k in names], None)

    cases = [(dict(M=-1), '2^24'), (dict(M=2 ** 24 + 1), '2^24'), (dict(nbits=0), '65534'), (dict(nbits=65535), '65534'), (dict(ldr=2), 'ldr'),
             (dict(lanes16=1, ldr=32), 'ldr'), (dict(lanes16=1, fold=1, ldr=40), 'fold'), (dict(nn_index=None), 'both or neither'),
             (dict(nn_dist=None), 'both or neither')]
    cases += [({k: None}, 'null operand') for k in ('rows', 'edge_lo', 'edge_hi', 'edge_dist', 'rounds')]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        msg = last_error(L)
        assert msg.startswith('tn_state_linkage') and word in msg, (kw, msg)
    assert L.tn_state_linkage_ws_bytes(-1, 130, 0) == 0 and L.tn_state_linkage_ws_bytes(10, 0, 0) == 0 and L.tn_state_linkage_ws_bytes(10, 65535, 0) == 0
    assert L.tn_state_linkage_ws_bytes(0, 130, 0) == 0 and L.tn_state_linkage_ws_bytes(1, 130, 0) == 0
