"""Host side of tnac4o.exchange_clusters (tnac4o_amd/exchange.py), the law of the move from the reference of tests/exchange_ref.py, and
the argument errors of tn_cluster_exchange.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

import exchange_ref as xr
from overlap_ref import droplet, ising3x3, last_error, rmf
from tnac4o_amd import exchange as ex
from tnac4o_amd import overlap as ov


# ---------------------------------------------------------------------------------------------- the law of the move
def test_pair_chain_is_symmetric_and_keeps_the_product_law():
    """The exact chain of a pair of replicas on 6 spins (a triangle, a pendant spin, an isolated spin; integer couplings and fields):
    P = P^T exactly, E_a + E_b is conserved on every transition, and (pi x pi) P = pi x pi to 1e-14 in the 1-norm at beta = 0.6."""
    n, edges, J, h = xr.small_model()
    src, dst, num, den = xr.pair_chain(n, edges)
    N = 1 << (2 * n)
    # P as exact integers over a common denominator: every row sums to 1, and the table equals its transpose
    common = int(np.lcm.reduce(np.arange(1, n + 1)))
    K = np.zeros((N, N), dtype=np.int32)
    np.add.at(K, (src, dst), (num * (common // den)).astype(np.int32))
    assert np.all(K.sum(axis=1) == common)
    assert np.array_equal(K, K.T)
    E = xr.model_energies(n, edges, J, h)
    a, b = src >> n, src & ((1 << n) - 1)
    na, nb = dst >> n, dst & ((1 << n) - 1)
    assert np.array_equal(E[a] + E[b], E[na] + E[nb])
    assert np.any((na != a) & (na != b))                               # (a move that is not a swap of the replicas is among them)
    pi = np.exp(-0.6 * (E - E.min()))
    pi /= pi.sum()
    pp = np.outer(pi, pi).reshape(-1)
    after = pp @ (K.astype(np.float64) / common)
    err = float(np.abs(after - pp).sum())
    print('|(pi x pi) P - pi x pi|_1 = %.2e' % err)
    assert err <= 1e-14


def test_reference_rules():
    rowptr, cols = xr.csr(5, xr.path_edges(5))
    assert rowptr.tolist() == [0, 1, 3, 5, 7, 8] and cols.tolist() == [1, 0, 2, 1, 3, 2, 4, 3]
    assert xr.seed_bit(0b101100, 0.0) == 2 and xr.seed_bit(0b101100, 0.34) == 3 and xr.seed_bit(0b101100, xr.U_MAX) == 5
    assert xr.reach(0b11011, 0, 5, rowptr, cols) == 0b00011 and xr.reach(0b11011, 4, 5, rowptr, cols) == 0b11000
    one_way = xr.csr(5, xr.path_edges(5), both=False)
    assert xr.reach(0b11111, 2, 5, *one_way) == 0b11100                # directed reachability
    assert xr.move(0b00111, 0b00000, 0.0, 5, rowptr, cols) == (0b00000, 0b00111, 3, 3)       # all of D: the replicas swap
    bad_ptr = np.array([0, 99, -5, 2, 2, 2], dtype=np.int32)           # clamped to [0, nnz]; a range that ends before it starts is empty
    assert xr.arcs(0, bad_ptr, cols).tolist() == cols.tolist() and xr.arcs(1, bad_ptr, cols).size == 0 and xr.arcs(2, bad_ptr, cols).tolist() == [1, 0]


# ---------------------------------------------------------------------------------------------- the driver's host parts
def test_coupling_csr_of_the_droplet_instance():
    s = droplet()
    rowptr, cols = ex.coupling_csr(s)
    act = ov.active_spins(s)
    n = act.size
    assert rowptr.dtype == np.int32 and cols.dtype == np.int32 and rowptr.shape == (n + 1,) and rowptr[0] == 0 and rowptr[-1] == cols.size
    links = ov.link_pairs(s.J0)
    assert cols.size == 2 * len(links)
    A = np.zeros((n, n), dtype=bool)
    for i in range(n):
        nb = cols[rowptr[i]:rowptr[i + 1]]
        assert np.all(np.diff(nb) > 0) and np.all((nb >= 0) & (nb < n))  # ascending, no arc twice, active spins only
        A[i, nb] = True
    assert np.array_equal(A, A.T) and not A.diagonal().any()
    want = np.zeros((n, n), dtype=bool)
    pos = {int(v): k for k, v in enumerate(act)}
    for i, j in links:
        want[pos[int(i)], pos[int(j)]] = want[pos[int(j)], pos[int(i)]] = True
    assert np.array_equal(A, want)


def test_coupling_csr_maps_to_active_positions_and_refuses_inactive_ends():
    J0 = np.zeros((6, 6))
    J0[1, 4] = J0[4, 5] = 1.0
    J0[2, 2] = 0.5                                                     # a field is no coupling
    s = SimpleNamespace(mode='Ising', J0=J0, ind0=[[[4, 1], [5, 2]]])  # spins 0 and 3 are in no cell
    rowptr, cols = ex.coupling_csr(s)                                  # positions: 1 -> 0, 2 -> 1, 4 -> 2, 5 -> 3
    assert rowptr.tolist() == [0, 1, 1, 3, 4] and cols.tolist() == [2, 0, 3, 2]
    J0[0, 4] = 2.0
    with pytest.raises(ValueError, match='no cell'):
        ex.coupling_csr(s)
    with pytest.raises(ValueError):
        ex.coupling_csr(rmf())


def test_default_pairing_and_uniforms_reproduce():
    np.random.seed(5)
    pairs = ex.check_pairs(None, 3, 11)
    u = ex.check_round_uniforms(None, 3, 5)
    np.random.seed(5)
    want = np.array([np.random.permutation(11)[:10].reshape(5, 2) for _ in range(3)])     # every pairing before any uniform
    assert pairs.dtype == np.int32 and np.array_equal(pairs, want) and np.array_equal(u, np.random.rand(3, 5))
    for k in range(3):
        assert np.unique(pairs[k]).size == 10
    s = droplet()
    s.states = np.random.default_rng(1).integers(0, 256, (7, 16)).astype(s.indtype)
    np.random.seed(9)
    r, p, uu = ex.check_arguments(s, 2, None, None)
    np.random.seed(9)
    assert r == 2 and np.array_equal(p, ex.check_pairs(None, 2, 7)) and np.array_equal(uu, np.random.rand(2, 3))
    assert ex.check_pairs(None, 0, 7).shape == (0, 3, 2)
    given = np.array([[[6, 0], [2, 3]]], dtype=np.int64)
    assert np.array_equal(ex.check_pairs(given, 1, 7), given) and ex.check_pairs(given.astype(np.uint8), 1, 7).dtype == np.int32
    assert ex.check_pairs(np.zeros((2, 0, 2), dtype=np.int64), 2, 7).shape == (2, 0, 2)


def test_unpack_bits_inverts_pack_bits():
    b = np.random.default_rng(0).integers(0, 2, (7, 200))
    assert np.array_equal(ex.unpack_bits(ov.pack_bits(b), 200), b)
    assert np.array_equal(ex.unpack_bits(ov.pack_bits(b[:, :64]), 64), b[:, :64])


def test_public_call_value_errors():
    torch = pytest.importorskip('torch')
    r = rmf()
    r.states = np.zeros((5, 9), dtype=r.indtype)
    with pytest.raises(ValueError, match='Ising'):
        r.exchange_clusters()
    s = droplet()
    with pytest.raises(ValueError, match='two stored states'):          # no states
        s.exchange_clusters()
    s.states = np.zeros((1, 16), dtype=s.indtype)
    with pytest.raises(ValueError, match='two stored states'):          # one state has no partner
        s.exchange_clusters()
    s.states = np.random.default_rng(4).integers(0, 256, (5, 16)).astype(s.indtype)
    kept = np.copy(s.states)
    ok_p, ok_u = np.array([[[0, 1], [4, 2]]]), np.array([[0.5, 0.25]])
    for rounds in (-1, 1.5):
        with pytest.raises(ValueError, match='rounds'):
            s.exchange_clusters(rounds=rounds)
    bad_pairs = ([[[0, 1], [4, 2]]],                                   # a list
                 ok_p.astype(np.float64),                              # no integers
                 ok_p[0],                                              # (P, 2)
                 np.zeros((1, 2, 3), dtype=np.int64),                  # triples
                 np.zeros((2, 2, 2), dtype=np.int64),                  # another number of rounds
                 np.array([[[0, 1], [4, 5]]]),                         # an index of M
                 np.array([[[0, 1], [-1, 2]]]),                        # a negative index
                 np.array([[[0, 1], [1, 2]]]),                         # an index twice in a round
                 np.array([[[3, 3], [1, 2]]]))                         # ... within a pair
    for bad in bad_pairs:
        with pytest.raises(ValueError, match='pairs'):
            s.exchange_clusters(pairs=bad, uniforms=ok_u)
    twice_over_rounds = np.array([[[0, 1]], [[1, 0]]])                 # the same index in two rounds is fine: refused for the uniforms only
    with pytest.raises(ValueError, match='uniforms'):
        s.exchange_clusters(rounds=2, pairs=twice_over_rounds, uniforms=ok_u)
    bad_uniforms = ([[0.5, 0.25]], ok_u[0], np.zeros((1, 3)), np.zeros((2, 2)), ok_u.astype(np.float32), np.array([[0.5, 1.0]]),
                    np.array([[-1e-300, 0.5]]), np.array([[0.5, np.nan]]), np.array([[np.inf, 0.5]]), torch.as_tensor(ok_u).float(),
                    torch.as_tensor(np.array([[0.5, 1.0]])), torch.zeros((2, 1), dtype=torch.float64))
    for bad in bad_uniforms:
        with pytest.raises(ValueError, match='uniforms'):
            s.exchange_clusters(pairs=ok_p, uniforms=bad)
    assert np.array_equal(s.states, kept) and not hasattr(s, 'exchange_pairs') and not hasattr(s, 'exchange_cluster_sizes')
    t = ising3x3()
    t.states = np.zeros((2, 9), dtype=t.indtype)
    with pytest.raises(ValueError, match='uniforms'):                  # M = 2: one pair by default
        t.exchange_clusters(uniforms=np.zeros((1, 2)))


# ---------------------------------------------------------------------------------------------- argument errors of the export
def test_cluster_exchange_argument_errors():
    """rc = -1 with a message and nothing launched: the pointers below are not device memory, they are never followed."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    p = 4096                                                           # stands for a non-null pointer
    M, nbits, ldr, nnz, P = 10, 130, 3, 40, 5

    def call(rows=p, M=M, nbits=nbits, ldr=ldr, rowptr=p, cols=p, nnz=nnz, pairs=p, P=P, u=p, size=p, diff=p):
        return L.tn_cluster_exchange(rows, M, nbits, ldr, rowptr, cols, nnz, pairs, P, u, size, diff, None)

    for kw, word in ((dict(nbits=0), '65534'), (dict(nbits=65535), '65534'), (dict(nbits=-3), '65534'), (dict(ldr=2), 'ldr'),
                     (dict(nbits=4097, ldr=64), 'ldr'), (dict(M=-1), 'M'), (dict(M=2 ** 31), '2^31'), (dict(P=-1), 'P'), (dict(nnz=-1), 'nnz'),
                     (dict(nnz=2 ** 31), '2^31'), (dict(rows=None), 'null operand'), (dict(rowptr=None), 'null operand'),
                     (dict(cols=None), 'null operand'), (dict(pairs=None), 'null operand'), (dict(u=None), 'null operand'),
                     (dict(size=None), 'null operand'), (dict(diff=None), 'null operand')):
        assert call(**kw) == -1, kw
        msg = last_error(L)
        assert msg.startswith('tn_cluster_exchange') and word in msg, (kw, msg)
    assert call(P=0) == 0                                              # a valid no-op, whatever the pointers
    assert call(P=0, rows=None, rowptr=None, cols=None, pairs=None, u=None, size=None, diff=None) == 0
    assert call(P=0, nbits=0) == -1 and call(P=0, ldr=2) == -1        # ... but not whatever the shape
