"""Host side of tnac4o.calculate_droplets (tnac4o_amd/droplets_of_states.py), the reference of tests/droplets_ref.py against brute force,
and the argument errors of tn_droplets.  No GPU."""
import numpy as np
import pytest

import droplets_ref as dr
import exchange_ref as xr
from overlap_ref import droplet, ising3x3, last_error, rmf
from tnac4o_amd import droplets_of_states as ds
from tnac4o_amd import exchange as ex
from tnac4o_amd import overlap as ov
from tnac4o_amd.auxx import energy_Jij


def chimera2x2():
    import tnac4o_amd
    from tnac4o_amd import auxx
    return tnac4o_amd.tnac4o(mode='Ising', Nx=2, Ny=2, Nc=8, J=auxx.synthetic_chimera(2, 2, 29), beta=1.0)


# ---------------------------------------------------------------------------------------------- the reference against brute force
@pytest.mark.parametrize('seed', range(6))
def test_reference_against_brute_force(seed):
    """Random graphs of 3 .. 12 spins with integer couplings and fields, 24 random pairs (x, g) each: roots, sizes and energies equal the
    components found by union-find with dE from two calls of energy_Jij, exactly; the droplets partition x XOR g; sum dE = E(x) - E(g)."""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(3, 13))
    edges = sorted({(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(0, n, (2 * n, 2)) if a != b})
    J, h = dr.integer_J(len(edges), rng), rng.integers(-3, 4, n).astype(np.float64)
    rowptr, cols, vals = dr.wcsr(n, edges, J)
    triples = [(i, j, float(v)) for (i, j), v in zip(edges, J)] + [(i, i, float(h[i])) for i in range(n)]
    for _ in range(24):
        x, g = rng.integers(0, 2, n), rng.integers(0, 2, n)
        xi, gi = (sum(int(b) << k for k, b in enumerate(v)) for v in (x, g))
        drops = dr.row_droplets(xi, gi, n, rowptr, cols, vals, h)
        got = [(root, size, dr.energy_and_bound(terms)[0]) for root, size, _, terms in drops]
        assert got == dr.brute_force(n, edges, J, h, x, g)
        union = 0
        for _, _, C, _ in drops:
            assert union & C == 0
            union |= C
        assert union == xi ^ gi
        total = sum(e for _, _, e in got)
        assert total == energy_Jij(triples, x[None, :])[0] - energy_Jij(triples, g[None, :])[0]


def test_reference_rules():
    """A path of 6 spins by hand: the gap, the field, a one-way CSR, the slots and the counts of run()."""
    edges, J = xr.path_edges(6), [1.0, 2.0, 4.0, -1.0, -2.0]
    rowptr, cols, vals = dr.wcsr(6, edges, J)
    h = np.array([1.0, 0.0, 0.0, 0.0, 0.0, -3.0])
    g = 0b000000                                                        # every g_i = -1
    drops = dr.row_droplets(0b110011, g, 6, rowptr, cols, vals, h)     # droplets {0, 1} and {4, 5}: they share no neighbour, 2 and 3 are equal
    assert [(r, s, C) for r, s, C, _ in drops] == [(0, 2, 0b000011), (4, 2, 0b110000)]
    assert [dr.energy_and_bound(t)[0] for _, _, _, t in drops] == [2.0 * (1.0 - 2.0), 2.0 * (1.0 - 3.0)]       # -h_0 g_0 - J_12; -J_34 - h_5 g_5
    drops = dr.row_droplets(0b011011, g, 6, rowptr, cols, vals, None)   # the gap at spin 2: two droplets that share it as a neighbour
    assert [(r, s) for r, s, _, _ in drops] == [(0, 2), (3, 2)] and [dr.energy_and_bound(t)[0] for _, _, _, t in drops] == [-4.0, -8.0 + 4.0]
    back = dr.wcsr(6, [(i + 1, i) for i in range(5)], J, both=False)    # arcs i + 1 -> i only: spin 1 finds spin 0 taken
    drops = dr.row_droplets(0b000111, g, 6, *back, None)
    assert [(r, s, C) for r, s, C, _ in drops] == [(0, 1, 0b001), (1, 1, 0b010), (2, 1, 0b100)]
    assert [t for _, _, _, t in drops] == [[], [], []]                  # ... and the arc into a droplet's spin adds no term
    out = dr.run(np.array([[0b110011], [0b010101], [0]], dtype=np.uint64), np.array([0], dtype=np.uint64), 6, rowptr, cols, vals, h, 2)
    assert out['count'].tolist() == [2, 3, 0] and out['diff'].tolist() == [4, 3, 0] and out['largest'].tolist() == [2, 1, 0]
    assert out['root'].tolist() == [[0, 4], [0, 2], [-1, -1]] and out['size'].tolist() == [[2, 2], [1, 1], [0, 0]]
    assert out['size_hist'].tolist() == [0, 3, 2, 0, 0, 0, 0] and out['labels'].tolist() == [[0, 0, -1, -1, 1, 1], [0, -1, 1, -1, 2, -1], [-1] * 6]
    assert out['de_total'][1] == 2.0 * ((1.0 - 1.0) + (-2.0 - 4.0) + (1.0 + 2.0)) and out['de_total'][2] == 0.0


# ---------------------------------------------------------------------------------------------- the driver's host parts
def test_weighted_csr_against_J0():
    """The small chimera solver: the arcs are coupling_csr's, every arc carries J0 of its coupling in both directions, the fields are
    the diagonal, and the energy of auxx.energy_Jij is the sum over the arcs and the fields."""
    s = chimera2x2()
    rowptr, cols, vals, field = ex.weighted_coupling_csr(s)
    plain = ex.coupling_csr(s)
    assert np.array_equal(rowptr, plain[0]) and np.array_equal(cols, plain[1])
    assert vals.dtype == np.float64 and vals.shape == cols.shape and field.dtype == np.float64
    act = ov.active_spins(s)
    n = act.size
    J0 = np.asarray(s.J0)
    W = np.zeros((n, n))
    for i in range(n):
        W[i, cols[rowptr[i]:rowptr[i + 1]]] = vals[rowptr[i]:rowptr[i + 1]]
    up = np.triu(J0, 1)[np.ix_(act, act)]
    assert np.array_equal(W, up + up.T) and np.count_nonzero(W) == cols.size and np.array_equal(field, J0.diagonal()[act])
    _, rowptr2, cols2, vals2, field2 = dr.model_graph(s)
    assert np.array_equal(rowptr, rowptr2) and np.array_equal(cols, cols2) and np.array_equal(vals, vals2) and np.array_equal(field, field2)
    bits = np.random.default_rng(2).integers(0, 2, (5, int(s.L)))
    sp = 2.0 * bits[:, act] - 1.0
    triples = [(int(i), int(j), float(J0[i, j])) for i, j in np.argwhere(J0 != 0)]
    assert np.allclose(0.5 * np.einsum('mi,ij,mj->m', sp, W, sp) + sp @ field, energy_Jij(triples, bits), rtol=0, atol=1e-12)
    assert ds.reference_energy(J0, bits[0]) == pytest.approx(energy_Jij(triples, bits[:1])[0], abs=1e-12)
    with pytest.raises(ValueError):
        ex.weighted_coupling_csr(rmf())


def test_state_bits_and_the_reference_forms():
    s = droplet()
    rng = np.random.default_rng(3)
    s.states = rng.integers(0, 256, (7, 16)).astype(s.indtype)
    act = ov.active_spins(s)
    st = s.states.view(np.uint8).astype(np.int64)
    assert np.array_equal(ds.state_bits(s, st), ov.spin_bits(s))
    s.energy = np.array([3.0, -2.0, 5.0, -2.0, np.nan, 0.0, 1.0])
    full = s.binary_states()
    by_energy, by_index, by_bits = ds.check_reference(s, None), ds.check_reference(s, 1), ds.check_reference(s, full[1])
    assert np.array_equal(by_energy, by_index) and np.array_equal(by_index, by_bits)        # the first of the two lowest
    assert by_bits.dtype == np.uint8 and np.array_equal(by_bits[act], full[1][act]) and by_bits.sum() == full[1][act].sum()
    assert np.array_equal(ds.check_reference(s, np.int64(6)), ds.check_reference(s, full[6].astype(np.int64)))
    ref, bits, K = ds.check_arguments(s, 3, 5, False, None, None)
    assert K == 5 and np.array_equal(bits, ov.spin_bits(s)) and np.array_equal(ref[act], bits[3])
    ref, bits, K = ds.check_arguments(s, full[0], 0, True, st[2:4], 1)
    assert K == 0 and np.array_equal(bits, ov.spin_bits(s)[2:4])


def test_public_call_value_errors():
    r = rmf()
    r.states = np.zeros((5, 9), dtype=r.indtype)
    with pytest.raises(ValueError, match='Ising'):
        r.calculate_droplets()
    s = droplet()
    with pytest.raises(ValueError, match='stored states'):               # no states
        s.calculate_droplets()
    L = int(s.L)
    with pytest.raises(ValueError, match='stored states'):               # ... also with a reference given as bits
        s.calculate_droplets(reference=np.zeros(L, dtype=np.int64))
    given = np.random.default_rng(4).integers(0, 256, (5, 16))
    with pytest.raises(ValueError, match='reference'):                   # states= given, but no stored state to take the reference from
        s.calculate_droplets(states=given)
    s.states = given.astype(s.indtype)
    kept = np.copy(s.states)
    with pytest.raises(ValueError, match='energy'):                      # reference=None needs the energies
        s.calculate_droplets()
    s.energy = np.zeros(4)
    with pytest.raises(ValueError, match='energy'):
        s.calculate_droplets()
    s.energy = np.full(5, np.nan)
    with pytest.raises(ValueError, match='energy'):
        s.calculate_droplets()
    s.energy = np.arange(5.0)
    ok = s.binary_states()[0]
    for bad in (5, -1, 2 ** 40):
        with pytest.raises(ValueError, match='reference'):
            s.calculate_droplets(reference=bad)
    two = ok.copy()
    two[ov.active_spins(s)[3]] = 2
    for bad in (True, 1.0, 'lowest', ok.tolist(), ok.astype(np.float64), ok[:-1], ok[None, :], two):
        with pytest.raises(ValueError, match='reference'):
            s.calculate_droplets(reference=bad)
    for bad in (-1, 1.5, True, None, 2 ** 31, '4'):
        with pytest.raises(ValueError, match='max_droplets'):
            s.calculate_droplets(reference=0, max_droplets=bad)
    for bad in (1, None, 'yes'):
        with pytest.raises(ValueError, match='labels'):
            s.calculate_droplets(reference=0, labels=bad)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError, match='chunk'):
            s.calculate_droplets(reference=0, chunk=bad)
    for bad in (given.tolist(), given.astype(np.float64), given[0], given[:, :15], given[:0], np.full((2, 16), 256), np.full((2, 16), -1)):
        with pytest.raises(ValueError, match='states'):
            s.calculate_droplets(reference=0, states=bad)
    assert np.array_equal(s.states, kept) and not hasattr(s, 'droplet_count') and not hasattr(s, 'droplet_sizes')
    t = ising3x3()
    t.states = np.zeros((2, 9), dtype=t.indtype)
    with pytest.raises(ValueError, match='reference'):                   # L = 18 bits, not 9
        t.calculate_droplets(reference=np.zeros(9, dtype=np.int64))


# ---------------------------------------------------------------------------------------------- argument errors of the export
def test_droplets_argument_errors():
    """rc = -1 with a message and nothing launched: the pointers below are not device memory, they are never followed."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    p = 4096                                                           # stands for a non-null pointer
    names = ('rows', 'M', 'nbits', 'ldr', 'ref', 'rowptr', 'cols', 'vals', 'nnz', 'field', 'K', 'count', 'diff', 'largest', 'de_total', 'root', 'size',
             'de', 'hist', 'labels', 'ldl')
    base = dict(rows=p, M=10, nbits=130, ldr=3, ref=p, rowptr=p, cols=p, vals=p, nnz=40, field=p, K=4, count=p, diff=p, largest=p, de_total=p, root=p,
                size=p, de=p, hist=p, labels=p, ldl=130)

    def call(**kw):
        a = dict(base)
        a.update(kw)
        return L.tn_droplets(*[a[k] for k in names], None)

    cases = [(dict(nbits=0), '65534'), (dict(nbits=65535), '65534'), (dict(nbits=-3), '65534'), (dict(ldr=2), 'ldr'), (dict(nbits=4097, ldr=64, ldl=4097), 'ldr'),
             (dict(M=-1), 'M'), (dict(M=2 ** 31), '2^31'), (dict(nnz=-1), 'nnz'), (dict(nnz=2 ** 31), '2^31'), (dict(K=-1), 'K'), (dict(K=2 ** 31), 'K'),
             (dict(M=2 ** 31 - 1, K=2 ** 31 - 1), 'M K'), (dict(ldl=129), 'ldl'), (dict(ldl=-1), 'ldl'), (dict(M=2 ** 31 - 1, ldl=2 ** 40), 'ldl')]
    cases += [({k: None}, 'null operand') for k in ('rows', 'ref', 'rowptr', 'cols', 'vals', 'count', 'diff', 'largest', 'de_total', 'root', 'size', 'de', 'hist')]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        msg = last_error(L)
        assert msg.startswith('tn_droplets') and word in msg, (kw, msg)
    assert call(M=0) == 0                                              # a valid no-op, whatever the pointers
    assert call(M=0, **{k: None for k in names if base[k] == p}) == 0
    assert call(M=0, nbits=0) == -1 and call(M=0, ldr=2) == -1 and call(M=0, K=-1) == -1 and call(M=0, ldl=3) == -1       # ... but not whatever the shape
    assert call(M=0, labels=None, ldl=0) == 0                          # without labels ldl is not looked at
