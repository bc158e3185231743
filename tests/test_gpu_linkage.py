"""tn_state_linkage and tnac4o.calculate_state_linkage on the GPU against the reference of tests/linkage_ref.py: every output is an
integer function of the inputs and is compared for equality.  The raw C-ABI with every buffer between guards, outputs preset to 0x55,
inputs checked unchanged: tile and word edges, ties, the ruler path (depth), fold, lanes, two far groups, grid independence, no
nearest rows, the refusals; the wrapper; the public call on the small solvers."""
import ctypes as ct

import numpy as np
import pytest

import linkage_ref as lr
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_sampling import dv, small      # noqa: E402  (helpers only, no test is imported)

EDGE_KEYS = ('edge_lo', 'edge_hi', 'edge_dist')
ALL_KEYS = EDGE_KEYS + ('nn_index', 'nn_dist')
FILL = 0x55555555


# ---------------------------------------------------------------------------------------------- helpers
def _last_error():
    from tnac4o_amd import _lib
    buf = ct.create_string_buffer(512)
    _lib.lib().tn_last_error(buf, 512)
    return buf.value.decode()


def _log2ceil(M):
    return int(M - 1).bit_length() if M >= 2 else 0


def _buffers(rows, M, nbits, lanes16, short=0):
    """Every buffer of a call between guards: the rows, the outputs preset to 0x55, the workspace of exactly ws_bytes - short bytes."""
    from tnac4o_amd import _lib
    g = {'rows': Guarded.of(torch.int64, rows.shape, 0x55, seed=1)}
    if rows.size:
        g['rows'].tensor().copy_(dv(rows.view(np.int64)))
    for i, k in enumerate(EDGE_KEYS):
        g[k] = Guarded.of(torch.int32, (max(M - 1, 0),), 0x55, seed=10 + i)
    g['nn_index'], g['nn_dist'] = Guarded.of(torch.int32, (max(M, 0),), 0x55, seed=13), Guarded.of(torch.int32, (max(M, 0),), 0x55, seed=14)
    g['rounds'] = Guarded.of(torch.int32, (1,), 0x55, seed=15)
    wsb = int(_lib.lib().tn_state_linkage_ws_bytes(M, nbits, int(lanes16)))
    g['ws'] = Guarded(max(wsb - short, 0), 0x55, seed=16)
    return g, wsb - short


def _call(g, M, nbits, ldr, lanes16, fold, wsb, **null):
    from tnac4o_amd import _lib, ops

    def p(k):
        return None if null.get(k) else g[k].ptr

    rc = _lib.lib().tn_state_linkage(p('rows'), M, nbits, ldr, int(lanes16), int(fold), p('nn_index'), p('nn_dist'), p('edge_lo'), p('edge_hi'),
                                     p('edge_dist'), p('rounds'), p('ws'), wsb, ops._stream())
    torch.cuda.synchronize()
    return rc


def linkage_device(rows, nbits, lanes16=False, fold=False, nearest=True):
    """One call of tn_state_linkage with every buffer between guards: the dict of linkage_ref.run plus 'rounds' (nn_* None without)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    M = rows.shape[0]
    g, wsb = _buffers(rows, M, nbits, lanes16)
    rc = _call(g, M, nbits, rows.shape[1], lanes16, fold, wsb, nn_index=not nearest, nn_dist=not nearest)
    assert rc == 0, (rc, _last_error())
    for b in g.values():
        assert b.intact()
    assert np.array_equal(g['rows'].host().view(np.uint64), rows)
    got = {k: g[k].host().astype(np.int64) for k in ALL_KEYS}
    if not nearest:
        assert g['nn_index'].untouched(0x55) and g['nn_dist'].untouched(0x55)
        got['nn_index'] = got['nn_dist'] = None
    got['rounds'] = int(g['rounds'].host()[0])
    return got


def compare(got, want, M):
    for k in ALL_KEYS:
        if got[k] is not None:
            assert np.array_equal(got[k], want[k]), (k, got[k][:8], want[k][:8])
    assert got['rounds'] == 0 if M < 2 else 1 <= got['rounds'] <= _log2ceil(M), got['rounds']


# ---------------------------------------------------------------------------------------------- 1. tile and word edges
MS = (0, 1, 2, 3, 63, 64, 65, 129, 200)
NS = (1, 63, 64, 65, 1000, 1025)
SHAPES = sorted({(M, 65) for M in MS} | {(M, n) for M in (65, 129) for n in NS} | {(200, 1025), (200, 1), (64, 64), (63, 63), (3, 1), (2, 1000)})
_ref = {}


def reference(M, nbits, lanes16=False, fold=False):
    """(rows, the reference's dict) of the random case, computed once."""
    key = (M, nbits, lanes16, fold)
    if key not in _ref:
        rows = lr.random_rows(M, nbits, 1000 * M + nbits, lanes16)
        _ref[key] = (rows, lr.run(rows, nbits, lanes16, fold))
    return _ref[key]


@pytest.mark.parametrize('M,nbits', SHAPES, ids=['M%d-n%d' % s for s in SHAPES])
def test_tile_and_word_edges(M, nbits):
    """Random bits, ldr = nwords + 1 with poisoned padding, set bits beyond nbits in the last word."""
    rows, want = reference(M, nbits)
    assert rows.shape == (M, -(-nbits // 64) + 1)
    got = linkage_device(rows, nbits)
    compare(got, want, M)
    if M == 1:
        assert got['nn_index'].tolist() == [-1] and got['nn_dist'].tolist() == [-1]


# ---------------------------------------------------------------------------------------------- 2. ties, depth, fold, lanes, groups
def test_identical_rows():
    rows = np.tile(lr.random_rows(1, 100, 5)[:, :2], (130, 1))
    got = linkage_device(lr.frame(rows, 100, False, 6), 100)
    assert got['edge_lo'].tolist() == [0] * 129 and got['edge_hi'].tolist() == list(range(1, 130)) and got['edge_dist'].tolist() == [0] * 129
    assert got['nn_index'].tolist() == [1] + [0] * 129 and got['nn_dist'].tolist() == [0] * 130
    assert 1 <= got['rounds'] <= 8


def test_many_ties():
    """M = 129 with nbits = 4: five distinct distances and many duplicates."""
    rows, want = reference(129, 4)
    assert len(np.unique(lr.dense(rows, 4))) == 5
    compare(linkage_device(rows, 4), want, 129)


def test_ruler_path():
    """Row i differs from row i - 1 in 1 + (the exponent of 2 in i) fresh bits: the tree is the path, Boruvka needs 6 rounds."""
    rows, nbits = lr.ruler_rows(64)
    assert nbits == 120
    rows = lr.frame(rows, nbits, False, 7)
    got = linkage_device(rows, nbits)
    compare(got, lr.run(rows, nbits), 64)
    assert sorted(zip(got['edge_lo'].tolist(), got['edge_hi'].tolist())) == [(i - 1, i) for i in range(1, 64)]
    assert 1 <= got['rounds'] <= 6


@pytest.mark.parametrize('M,nbits', [(100, 64), (100, 65), (67, 10), (67, 129)])
def test_fold(M, nbits):
    """Random rows together with the complements of some of them (distance 0); nbits even (ties at n / 2) and odd."""
    rows = lr.folded_rows(M, nbits, 20 + nbits)
    want = lr.run(rows, nbits, fold=True)
    assert np.count_nonzero(want['edge_dist'] == 0) >= M // 3 - 1 and want['edge_dist'].max() <= nbits // 2
    compare(linkage_device(rows, nbits, fold=True), want, M)
    plain = linkage_device(rows, nbits)
    compare(plain, lr.run(rows, nbits), M)
    assert not np.array_equal(plain['edge_dist'], want['edge_dist'])


@pytest.mark.parametrize('M,lanes,alphabet', [(70, 9, 3), (65, 4, 2), (130, 70, 5)])
def test_lanes16(M, lanes, alphabet):
    rng = np.random.default_rng(lanes)
    X = rng.integers(0, alphabet, (M, lanes)) * 257 + (rng.integers(0, 2, (M, lanes)) << 15)       # low, high and top bits of a lane
    rows = lr.frame(lr.pack(X, True), lanes, True, 30 + lanes)
    compare(linkage_device(rows, lanes, lanes16=True), lr.run(rows, lanes, lanes16=True), M)


def test_two_far_groups():
    rows = lr.two_groups(300, 9)
    want = lr.run(rows, 300)
    assert want['edge_dist'][-1] >= 290 and want['edge_dist'][-2] <= 4 and np.count_nonzero(want['edge_dist'] == 0) > 10
    compare(linkage_device(rows, 300), want, 77)


# ---------------------------------------------------------------------------------------------- 3. grid, optional outputs
def test_grid_independence(monkeypatch):
    rows, want = reference(200, 1025)
    from tnac4o_amd import _lib
    sizes = []
    for wgs in ('1', '3', None):
        if wgs is None:
            monkeypatch.delenv('TN_LINKAGE_WGS', raising=False)
        else:
            monkeypatch.setenv('TN_LINKAGE_WGS', wgs)
        sizes.append(int(_lib.lib().tn_state_linkage_ws_bytes(200, 1025, 0)))
        got = linkage_device(rows, 1025)
        compare(got, want, 200)
        sizes.append(got['rounds'])
    assert sizes[1] == sizes[3] == sizes[5] and sizes[0] > 0


def test_without_nearest_rows():
    rows, want = reference(129, 65)
    got = linkage_device(rows, 65, nearest=False)
    assert got['nn_index'] is None
    compare(got, want, 129)


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_errors_leave_the_outputs_alone():
    rows, _ = reference(65, 65)
    M, ldr = rows.shape

    def refused(rc_want, word, M=M, nbits=65, ldr=ldr, lanes16=False, fold=False, short=0, **null):
        g, wsb = _buffers(rows, max(M, 0), 65, False, short)
        rc = _call(g, M, nbits, ldr, lanes16, fold, wsb, **null)
        assert rc == rc_want and word in _last_error(), (rc, _last_error())
        for k, b in g.items():
            assert b.intact() and (k == 'rows' or b.untouched(0x55)), k

    refused(-1, '2^24', M=-1)
    refused(-1, '65534', nbits=0)
    refused(-1, '65534', nbits=65535, ldr=2000)
    refused(-1, 'ldr', ldr=1)
    refused(-1, 'fold', lanes16=True, fold=True, ldr=20)
    for k in ('rows', 'edge_lo', 'edge_hi', 'edge_dist'):
        refused(-1, 'null operand', **{k: True})
    refused(-1, 'both or neither', nn_index=True)
    refused(-1, 'both or neither', nn_dist=True)
    refused(-3, 'workspace too small', short=1)


# ---------------------------------------------------------------------------------------------- 5. the wrapper
def test_wrapper():
    from tnac4o_amd import ops
    rows, want = reference(129, 65)
    d_rows = dv(rows.view(np.int64))
    got = ops.state_linkage(d_rows, 65)
    assert all(got[k].dtype == torch.int32 and got[k].is_cuda for k in ALL_KEYS + ('rounds',))
    compare({k: (v.cpu().numpy().astype(np.int64) if k != 'rounds' else int(v.cpu()[0])) for k, v in got.items()}, want, 129)
    bare = ops.state_linkage(d_rows, 65, nearest=False)
    assert bare['nn_index'] is None and bare['nn_dist'] is None and torch.equal(bare['edge_hi'], got['edge_hi'])
    folded = ops.state_linkage(d_rows, 65, fold=True)
    assert np.array_equal(folded['edge_dist'].cpu().numpy(), lr.run(rows, 65, fold=True)['edge_dist'])
    none, one = ops.state_linkage(d_rows[:0], 65), ops.state_linkage(d_rows[:1], 65)
    assert none['edge_lo'].numel() == 0 and none['nn_index'].numel() == 0 and int(none['rounds'][0]) == 0
    assert one['edge_lo'].numel() == 0 and one['nn_index'].tolist() == [-1] and one['nn_dist'].tolist() == [-1] and int(one['rounds'][0]) == 0
    with pytest.raises(RuntimeError):
        ops.state_linkage(d_rows.cpu(), 65)
    with pytest.raises(ValueError):
        ops.state_linkage(d_rows, 64 * d_rows.shape[1] + 1)
    from tnac4o_amd._lib import TnError
    with pytest.raises(TnError, match='fold'):
        ops.state_linkage(d_rows, 8, lanes16=True, fold=True)


# ---------------------------------------------------------------------------------------------- 6. the public call
def packed(ins, kind):
    from tnac4o_amd import overlap as ov
    rows, n, lanes16 = ov.rows_of(ins, kind)
    return rows, n, lanes16


def check_public(ins, rows, n, lanes16, fold, threshold):
    D = lr.dense(rows, n, lanes16, fold)
    M = D.shape[0]
    pairs, dist = lr.kruskal(D)
    nn, nd = lr.nearest(D)
    assert np.array_equal(ins.linkage_pairs, pairs) and ins.linkage_pairs.dtype == np.int64 and ins.linkage_pairs.shape == (M - 1, 2)
    assert np.array_equal(ins.linkage_distance, dist) and ins.linkage_distance.dtype == np.int64
    assert np.array_equal(ins.nearest_state, nn) and np.array_equal(ins.nearest_distance, nd)
    assert np.array_equal(ins.linkage_cluster_counts, lr.cluster_counts(dist, M, n)) and ins.linkage_cluster_counts.dtype == np.int64
    assert same_bits(ins.linkage_matrix, lr.linkage_matrix(pairs, dist, M))
    assert ins.linkage_symmetric is fold and 1 <= ins.linkage_rounds <= _log2ceil(M)
    if threshold is None:
        assert all(getattr(ins, a) is None for a in ('state_cluster_labels', 'state_cluster_sizes', 'state_cluster_first',
                                                     'state_cluster_representative', 'state_cluster_energy_min'))
        return
    want = lr.threshold_components(D, threshold)
    assert np.array_equal(ins.state_cluster_labels, want) and np.array_equal(ins.state_cluster_sizes, np.bincount(want))
    assert np.array_equal(ins.state_cluster_first, [np.flatnonzero(want == k)[0] for k in range(want.max() + 1)])
    assert ins.linkage_cluster_counts[min(threshold, n)] == want.max() + 1


@pytest.mark.parametrize('name', ['chimera', 'ising3x3'])
def test_public_call(name):
    """After a seeded sample_boltzmann(M=256): the tree against the reference on binary_states(), labels at two thresholds, symmetric
    both ways, kind 'cell', states=, the representative against energy; every other attribute of the solver is unchanged."""
    ins = small(name, 1.0)
    ins.sample_boltzmann(M=256, Dmax=4, seed=41)
    before = {k: (np.copy(v) if isinstance(v, np.ndarray) and v.dtype != object else v) for k, v in vars(ins).items()}
    rows, n, lanes16 = packed(ins, 'spin')
    fields = bool(np.any(np.asarray(ins.J0).diagonal() != 0))
    ret = ins.calculate_state_linkage()
    assert ret is ins.linkage_distance and ins.linkage_kind == 'spin'
    check_public(ins, rows, n, False, not fields, None)
    for sym in (True, False):
        for t in (1, n // 4):
            ins.calculate_state_linkage(threshold=t, symmetric=sym)
            check_public(ins, rows, n, False, sym, t)
            E = np.asarray(ins.energy)
            assert E.shape == (256,)
            for k, rep in enumerate(ins.state_cluster_representative):
                members = np.flatnonzero(ins.state_cluster_labels == k)
                assert rep == members[np.argmin(E[members])] and ins.state_cluster_energy_min[k] == E[members].min()
    crow, cn, cl = packed(ins, 'cell')
    ins.calculate_state_linkage(kind='cell', threshold=1)
    assert ins.linkage_kind == 'cell'
    check_public(ins, crow, cn, True, False, 1)
    st = np.asarray(ins.states)
    given = (st.view('u%d' % st.dtype.itemsize) if st.dtype.kind == 'i' and st.dtype.itemsize < 8 else st).astype(np.int64)
    ins.calculate_state_linkage(threshold=2, symmetric=False, states=given[40:140][::-1].copy())
    check_public(ins, rows[40:140][::-1], n, False, False, 2)
    assert ins.state_cluster_representative is None and ins.state_cluster_energy_min is None      # 100 states, 256 energies
    new = ('linkage_pairs', 'linkage_distance', 'nearest_state', 'nearest_distance', 'linkage_cluster_counts', 'linkage_matrix', 'linkage_kind',
           'linkage_symmetric', 'linkage_rounds', 'state_cluster_labels', 'state_cluster_sizes', 'state_cluster_first', 'state_cluster_representative',
           'state_cluster_energy_min')
    after = vars(ins)
    assert set(after) == set(before) | set(new)
    for k, v in before.items():                                         # numeric arrays by content, everything else by identity
        assert same_bits(after[k], v) if isinstance(v, np.ndarray) and v.dtype != object else after[k] is v, k


def test_public_call_rmf():
    ins = small('rmf3x3', 1.0)
    ins.sample_boltzmann(M=256, Dmax=64, seed=42)
    rows, n, lanes16 = packed(ins, 'cell')
    assert lanes16 and n == 9
    ins.calculate_state_linkage(threshold=2)
    assert ins.linkage_kind == 'cell'
    check_public(ins, rows, n, True, False, 2)
    with pytest.raises(ValueError, match='Ising'):
        ins.calculate_state_linkage(kind='spin')
