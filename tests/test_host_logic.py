"""CPU-only checks of the product's host-side logic (coupling split, rotations, PEPS factor tables, energy
bookkeeping) against the oracle, and of the C-ABI library's exports.  No GPU compute here."""
import ctypes
import os
import re

import numpy as np
import pytest

import golden_inputs as gi
from oracle import solver_ref as sr


def test_library_exports_every_declared_symbol():
    from tnac4o_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'tnpeps.h')).read()
    declared = set(re.findall(r'\b(tn_[a-z0-9_]+)\s*\(', header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    assert _lib.lib().tn_version() == _lib.ABI_VERSION
    # argument errors are reported without touching a GPU
    rc = _lib.lib().tn_qr(None, 1, 1, 4, 4, None, 1, 1, None, 1, 1, 32, 0.0, None, None, 0, None)
    assert rc < 0
    buf = ctypes.create_string_buffer(256)
    _lib.lib().tn_last_error(buf, 256)
    assert b'null operand' in buf.value


def test_every_switch_the_sources_read_is_in_the_switch_table():
    """INTEGRATION.md §3 lists every environment switch: the ones the library reads through the readers of csrc/common.h
    (env_flag_on, env_int, ...) and the ones the Python package takes from os.environ."""
    from tnac4o_amd import _lib
    names = set()
    for f in sorted(os.listdir(_lib.CSRC)):
        if f.endswith(('.hip', '.h')):
            text = open(os.path.join(_lib.CSRC, f)).read()
            assert 'getenv(' not in text or f == 'common.h', '%s reads the environment past the readers of common.h' % f
            names |= set(re.findall(r'\benv_[a-z0-9_]+\(\s*"(TN_[A-Z0-9_]+)"', text))
    for f in sorted(os.listdir(_lib.HERE)):
        if f.endswith('.py'):
            text = open(os.path.join(_lib.HERE, f)).read()
            names |= set(re.findall(r'os\.environ(?:\.get\(|\[)\s*[\'"](TN_[A-Z0-9_]+)[\'"]', text))
    assert {'TN_QR_NBO', 'TN_PANEL_CAPTURE_MIN', 'TN_PANEL_CAPTURE_MAXROWS', 'TN_NATIVE_CHAIN'} <= names      # both kinds of reader are seen
    table = open(os.path.join(os.path.dirname(_lib.HERE), 'INTEGRATION.md')).read()
    listed = set(re.findall(r'TN_[A-Z0-9_]+', table))
    assert names <= listed, sorted(names - listed)


def test_product_refuses_cpu_tensors():
    import torch
    from tnac4o_amd import ops
    with pytest.raises(RuntimeError):
        ops.mm(torch.zeros(2, 2, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.float64))


@pytest.mark.parametrize('rot', [0, 1, 2, 3])
def test_host_tables_match_oracle(rot):
    import tnac4o_amd
    J = gi.droplet_J(128, 2)
    a = tnac4o_amd.tnac4o(mode='Ising', Nx=4, Ny=4, Nc=8, J=J, beta=3.0)
    b = sr.RefSolver(mode='Ising', Nx=4, Ny=4, Nc=8, J=J, beta=3.0)
    if rot:
        a.rotate_graph(rot)
        b.rotate_graph(rot)
    assert np.array_equal(a.J, b.J) and np.array_equal(a.order, b.order) and np.array_equal(a.order_i, b.order_i)
    assert a.rotation == b.rotation
    rng = np.random.default_rng(rot)
    a.Xu = b.Xu = rng.uniform(0.5, 2, a.Xu.shape)
    a.Xd = b.Xd = rng.uniform(0.5, 2, a.Xd.shape)
    for ny in range(4):
        for nx in range(4):
            Fa, da, ra, pda, bra = a._peps_factor(ny, nx)
            Fb, db, rb, pdb, brb = b.peps_factor(ny, nx)
            assert np.array_equal(Fa, Fb) and np.array_equal(da, db) and np.array_equal(ra, rb) and (pda, bra) == (pdb, brb)
            assert np.array_equal(a._mpo_site(ny, nx), b.mpo_site(ny, nx))
            st = rng.integers(0, 256, (7, 16)).astype(np.int8)
            assert np.array_equal(a._update_Eng(st, ny, nx), b._update_Eng(st, ny, nx))
            assert np.array_equal(a._ind_bond_down(st[:, 0], ny, nx), b._ind_bond_down(st[:, 0], ny, nx))
            assert np.array_equal(a._ind_bond_right(st[:, 0], ny, nx), b._ind_bond_right(st[:, 0], ny, nx))


def test_host_tables_rmf():
    import tnac4o_amd
    J = gi.minimal_rmf()
    a = tnac4o_amd.tnac4o(mode='RMF', Nx=J['Nx'], Ny=J['Ny'], J=J, beta=2.0)
    b = sr.RefSolver(mode='RMF', Nx=J['Nx'], Ny=J['Ny'], J=J, beta=2.0)
    a.rotate_graph(1)
    b.rotate_graph(1)
    for ny in range(a.Ny):
        for nx in range(a.Nx):
            assert np.array_equal(a._mpo_site(ny, nx), b.mpo_site(ny, nx))


def test_synthetic_chimera_topology():
    from tnac4o_amd.auxx import synthetic_chimera
    J = synthetic_chimera(4, 4, 20260003)
    ref = np.loadtxt(os.path.join(gi.INST_DIR, 'chimera128_001.txt'))
    assert len(J) == len(ref)
    assert sorted((i, j) for i, j, _ in J) == sorted((int(r[0]) - 1, int(r[1]) - 1) for r in ref)
    assert all(v != 0 and abs(round(v * 75) - v * 75) < 1e-9 for _, _, v in J)
    assert synthetic_chimera(4, 4, 20260003) == J


def test_fast_unique_and_merge_match_reference_semantics():
    """The packed-key unique and the vectorised merge reproduce np.unique(axis=0) and the reference's group loop
    (tnac4o.py:481-509) exactly, including tie-breaking."""
    import itertools
    from tnac4o_amd.tnac4o import _unique_rows, _merge_groups
    rng = np.random.default_rng(0)
    for (n, w, hi) in [(5000, 17, 16), (3000, 5, 16), (2000, 9, 3), (1000, 1, 2), (4000, 17, 2), (1500, 20, 128)]:
        vind = rng.integers(0, hi, (n, w)).astype(np.int8 if hi <= 127 else np.int16)
        vind[rng.integers(0, n, n // 2)] = vind[rng.integers(0, n, n // 2)]          # plenty of duplicates
        u0, i0 = np.unique(vind, return_inverse=True, axis=0)
        u1, i1 = _unique_rows(vind)
        assert np.array_equal(u0, u1) and np.array_equal(i0.reshape(-1), i1)
        Eng = np.round(rng.standard_normal(n), 1)                                      # many exact ties
        prob = rng.standard_normal(n)
        deg = rng.integers(1, 5, n)
        min_dEng = 1e-12
        order = i1.argsort()
        inv = i1[order]
        sizes = [len(list(g)) for _, g in itertools.groupby(inv)]
        indn, degn, probn = np.zeros(len(sizes), dtype=int), np.zeros(len(sizes), dtype=int), np.zeros(len(sizes))
        lo = 0
        for k, sz in enumerate(sizes):
            ind = order[lo:lo + sz]
            Ek = Eng[ind]
            imin = np.argmin(Ek)
            indn[k] = ind[imin]
            same = ind[(Ek - Ek[imin]) <= min_dEng]
            if len(same) > 1:
                degn[k], probn[k] = sum(deg[same]), np.mean(prob[same])
            else:
                degn[k], probn[k] = deg[same][0], prob[same][0]
            lo += sz
        a, b, c, _, _ = _merge_groups(i1, Eng, prob, deg, min_dEng, canonical=False)
        assert np.array_equal(a, indn) and np.array_equal(b, degn) and np.array_equal(c, probn)
        # the canonical order (tnac4o_amd/beam.py): members in candidate order, first minimal-energy member, mean in member order
        order = i1.argsort(kind='stable')
        lo = 0
        for k, sz in enumerate(sizes):
            ind = order[lo:lo + sz]
            assert np.all(np.diff(ind) > 0)
            Ek = Eng[ind]
            imin = np.argmin(Ek)
            indn[k] = ind[imin]
            same = ind[(Ek - Ek[imin]) <= min_dEng]
            acc = 0.0
            for v in prob[same]:
                acc += float(v)
            degn[k], probn[k] = sum(deg[same]), (acc / len(same) if len(same) > 1 else prob[same][0])
            lo += sz
        a, b, c, _, _ = _merge_groups(i1, Eng, prob, deg, min_dEng)
        assert np.array_equal(a, indn) and np.array_equal(b, degn) and np.array_equal(c, probn)


# ---------------------------------------------------------------- I/O formats
def test_load_result_saved_by_reference(tmp_path):
    """tests/golden/g9_saved_by_reference.npy was written by the reference's own `save` (tools/make_golden.py g9)."""
    import tnac4o_amd
    import golden_inputs as gi
    ins = tnac4o_amd.load(os.path.join(gi.GOLDEN_DIR, 'g9_saved_by_reference.npy'))
    E, bits = gi.golden_groundstate(128, 1)
    assert ins.energy[0] == pytest.approx(E, abs=1e-5)
    assert ins.mode == 'Ising' and (ins.Nx, ins.Ny, ins.Nc) == (4, 4, 8) and ins.beta == 3.0
    assert np.array_equal(ins.binary_states()[0], bits)
    # our save -> our load round trip keeps everything; the file has the reference's keys
    out = str(tmp_path / 'again.npy')
    ins.save(out)
    d = np.load(out, allow_pickle=True).item()
    assert set(d) == {'mode', 'rotation', 'energy', 'probability', 'degeneracy', 'states', 'discarded_probability',
                      'negative_probability', 'Nx', 'Ny', 'Nc', 'beta', 'ind'}
    again = tnac4o_amd.load(out)
    assert np.array_equal(again.energy, ins.energy) and np.array_equal(again.states, ins.states)
    assert again.degeneracy == ins.degeneracy and np.array_equal(again.binary_states(), ins.binary_states())


def test_states_text_format_round_trip(tmp_path):
    from tnac4o_amd import auxx
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, size=(5, 128)).astype(np.int8)
    E = np.round(rng.normal(size=5) * 100, 6)
    f = str(tmp_path / 'states.txt')
    auxx.save_states_txt(f, E, bits)
    lines = open(f).read().splitlines()
    assert lines[0].startswith('# One line per state') and len(lines) == 6
    assert lines[1].split()[0] == '%4.6f' % E[0] and len(lines[1].split()) == 129
    E2, b2 = auxx.load_states_txt(f)
    assert np.allclose(E2, E, atol=1e-6) and np.array_equal(b2, bits)


# ---------------------------------------------------------------- low-energy spectrum bookkeeping
def _spectrum_check(s, g, tag, bits=True):
    assert len(s.energy) == len(g[tag + '_energy'])
    np.testing.assert_allclose(s.energy, g[tag + '_energy'], rtol=0, atol=1e-9)
    # states with (numerically) equal energies may come out in either order: compare as sets per energy level
    key = tag + ('_bits' if bits else '_states')
    got = s.binary_states() if bits else np.asarray(s.states)
    want = g[key]
    assert sorted(map(bytes, np.asarray(got, dtype=np.int16))) == sorted(map(bytes, np.asarray(want, dtype=np.int16)))


@pytest.mark.parametrize('rot,chi', [(0, 16), (3, 8)])
def test_spectrum_encoding1_droplet_golden(rot, chi):
    """examples/test_examples.py test_e03 (31 states within dE < 1 of droplet instance 1), encoding 1."""
    import golden_inputs as gi
    from spectrum_ref import SpectrumRef
    g = np.load(os.path.join(gi.GOLDEN_DIR, 'g10_spectrum.npz'))
    s = SpectrumRef(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=3.0)
    if rot:
        s.rotate_graph(rot)
    s.search_low_energy_spectrum(excitations_encoding=1, M=1024, relative_P_cutoff=1e-8, Dmax=chi, max_dEng=1.0, lim_hd=0)
    tag = 'L128_i1_r%d_chi%d' % (rot, chi)
    assert [len(s.d), len(s.el)] == list(g[tag + '_n_shapes'])
    s.decode_low_energy_states(max_dEng=1.0)
    assert len(s.energy) == 31
    _spectrum_check(s, g, tag)
    from oracle import solver_ref as sr
    E = sr.energy_Jij(gi.droplet_J(128, 1), s.binary_states())
    assert np.abs(E - s.energy).max() < 1e-6                  # every decoded state really has the energy it is listed with


def test_spectrum_hamming_limit_and_rmf_golden():
    import golden_inputs as gi
    from spectrum_ref import SpectrumRef
    g = np.load(os.path.join(gi.GOLDEN_DIR, 'g10_spectrum.npz'))
    s = SpectrumRef(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 2), beta=3.0)
    s.search_low_energy_spectrum(excitations_encoding=1, M=1024, relative_P_cutoff=1e-8, Dmax=16, max_dEng=0.8, lim_hd=3)
    s.decode_low_energy_states(max_dEng=0.8, max_states=20)
    _spectrum_check(s, g, 'L128_i2_r0_chi16_hd3')
    J = gi.e05_rmf()                                           # test_e05: 26 states within dE < 3.1
    for rot in (0, 1):
        s = SpectrumRef(mode='RMF', Nx=J['Nx'], Ny=J['Ny'], J=J, beta=4)
        if rot:
            s.rotate_graph(rot)
        s.search_low_energy_spectrum(excitations_encoding=1, M=1024, relative_P_cutoff=1e-12, Dmax=32, max_dEng=3.1, lim_hd=0)
        s.decode_low_energy_states(max_dEng=3.1, max_states=100)
        assert len(s.energy) == 26
        _spectrum_check(s, g, 'RMF_r%d' % rot, bits=False)


def test_unpack_snake_small_forest():
    """Hand-made forest: two droplets that do not overlap along the snake combine, a nested one needs its parent."""
    from tnac4o_amd import droplets
    a = ((0.5, 1, 6, 7, 0.0), ())                  # cells 6..7
    inner = ((0.2, 3, 2, 2, 0.0), ())              # cell 2, only valid inside b
    b = ((0.3, 2, 1, 3, 0.0), (inner,))            # cells 1..3
    E, flips = droplets.unpack_snake([b, a], 8, max_dEng=10.0)
    got = sorted((round(float(e), 6), tuple(sorted(f))) for e, f in zip(E, flips))
    assert got == sorted([(0.0, ()), (0.5, (1,)), (0.3, (2,)), (0.5, (2, 3)), (0.8, (1, 2)), (1.0, (1, 2, 3))])
    E, _ = droplets.unpack_snake([b, a], 8, max_dEng=0.55)
    assert sorted(np.round(E, 6)) == [0.0, 0.3, 0.5, 0.5]
    E, _ = droplets.unpack_snake([b, a], 8, max_dEng=10.0, max_states=3)
    assert len(E) <= 3 and 0.0 in E


def _adjacency_case(enc, rot, hd):
    import golden_inputs as gi
    from spectrum_ref import SpectrumRef
    g = np.load(os.path.join(gi.GOLDEN_DIR, 'g11_spectrum_adjacency.npz'))
    s = SpectrumRef(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=3.0)
    if rot:
        s.rotate_graph(rot)
    np.random.seed(100 + enc)
    s.add_noise(amplitude=1e-7)
    s.search_low_energy_spectrum(excitations_encoding=enc, M=1024, relative_P_cutoff=1e-8, Dmax=16, max_dEng=1.0, lim_hd=hd)
    tag = 'L128_i1_e%d_r%d_hd%d' % (enc, rot, hd)
    assert [len(s.d), len(s.el)] == list(g[tag + '_n_shapes'])
    s.decode_low_energy_states(max_dEng=1.0)
    return s, g, tag


@pytest.mark.parametrize('enc,rot,hd,n', [(2, 2, 0, 31), (3, 3, 0, 31), (3, 1, 2, 6)])
def test_spectrum_adjacency_encodings_golden(enc, rot, hd, n):
    """Encodings 2 and 3 (elementary droplets from the coupling graph) with the reference's seeded noise: same number of
    shapes, same decoded states (test_examples.py test_e03: 31 states within dE < 1)."""
    s, g, tag = _adjacency_case(enc, rot, hd)
    assert len(s.energy) == n
    np.testing.assert_allclose(s.energy, g[tag + '_energy'], rtol=0, atol=1e-9)
    assert sorted(map(bytes, np.asarray(s.binary_states(), dtype=np.int16))) == \
        sorted(map(bytes, np.asarray(g[tag + '_bits'], dtype=np.int16)))


def test_spectrum_adjacency_rmf_golden():
    import golden_inputs as gi
    from spectrum_ref import SpectrumRef
    g = np.load(os.path.join(gi.GOLDEN_DIR, 'g11_spectrum_adjacency.npz'))
    J = gi.e05_rmf()
    for enc, rot in ((2, 2), (3, 3)):
        s = SpectrumRef(mode='RMF', Nx=J['Nx'], Ny=J['Ny'], J=J, beta=4)
        s.rotate_graph(rot)
        np.random.seed(200 + enc)
        s.add_noise(amplitude=1e-7)
        s.search_low_energy_spectrum(excitations_encoding=enc, M=1024, relative_P_cutoff=1e-12, Dmax=32, max_dEng=3.1, lim_hd=0)
        s.decode_low_energy_states(max_dEng=3.1, max_states=100)
        assert len(s.energy) == 26
        np.testing.assert_allclose(s.energy, g['RMF_e%d_r%d_energy' % (enc, rot)], rtol=0, atol=1e-9)
        assert sorted(map(bytes, np.asarray(s.states, dtype=np.int16))) == \
            sorted(map(bytes, np.asarray(g['RMF_e%d_r%d_states' % (enc, rot)], dtype=np.int16)))


def test_droplet_shape_algebra():
    from tnac4o_amd import droplets
    a = (np.array([1, 4, 7]), np.array([3, 5, 1]))
    b = (np.array([4, 7, 9]), np.array([5, 2, 8]))
    c = droplets.combine_shapes(a, b)
    assert list(c[0]) == [1, 7, 9] and list(c[1]) == [3, 3, 8]                 # cell 4 cancels, cell 7 xors
    assert droplets.shape_distance(a, b, 'Ising') == 2 + 0 + 2 + 1             # bits of 3 | 5^5 | 1^2 | 8
    assert droplets.shape_distance(a, b, 'RMF') == 3                           # cells 1, 7, 9 differ
    conn = droplets.Connectivity('RMF', 5)
    assert conn.elementary((np.array([0, 1, 6]), np.array([1, 1, 1])))         # (0,0)-(0,1)-(1,1) connected
    assert not conn.elementary((np.array([0, 7]), np.array([1, 1])))
    assert conn.touch((np.array([0]), np.array([1])), (np.array([5]), np.array([2])))      # vertical neighbours
    assert not conn.touch((np.array([0]), np.array([1])), (np.array([7]), np.array([2])))


def test_decode_spectrum_file_saved_by_reference():
    """A result file of an encoding-2 search written by the reference's `save` (forest, shape table, adjacency as CSR):
    our `load` + `decode_low_energy_states` rebuild the reference's 31 states from it."""
    import tnac4o_amd
    import golden_inputs as gi
    g = np.load(os.path.join(gi.GOLDEN_DIR, 'g11_spectrum_adjacency.npz'))
    ins = tnac4o_amd.load(os.path.join(gi.GOLDEN_DIR, 'g11_saved_by_reference_e2.npy'))
    assert ins.excitations_encoding == 2
    ins.decode_low_energy_states(max_dEng=1.0)
    tag = 'L128_i1_e2_r2_hd0'
    np.testing.assert_allclose(ins.energy, g[tag + '_energy'], rtol=0, atol=1e-12)
    assert sorted(map(bytes, np.asarray(ins.binary_states(), dtype=np.int16))) == \
        sorted(map(bytes, np.asarray(g[tag + '_bits'], dtype=np.int16)))


def test_lazy_schmidt_values_are_evaluated_only_when_the_bond_keeps_its_dimension(monkeypatch):
    """mps._LazyS / _SchmidtList / _previous_S (the update_S bookkeeping of mps.py:550-560 with deferred evaluation): a recorded
    centre matrix is decomposed when the next update_S at that bond has the same length or when psi.S is read, and dropped
    unevaluated when the length differs -- in every case the numbers are the ones the eager evaluation would have stored."""
    import numpy as np
    from tnac4o_amd import mps

    calls = []

    class FakeC:
        def __init__(self, vals):
            self.vals = np.asarray(vals, dtype=float)
            self.shape = (len(vals), len(vals) + 3)

    monkeypatch.setattr(mps._LazyS, 'values', lambda self: (calls.append(self.size), self.Cm.vals.copy())[1])

    class Psi:
        _one_S = staticmethod(lambda D: np.concatenate([[1.0], np.zeros(D - 1)]))

    psi = Psi()
    psi.S = mps._SchmidtList([Psi._one_S(2), Psi._one_S(2), Psi._one_S(2)])
    psi.S[0] = mps._LazyS(FakeC([0.8, 0.6]))
    psi.S[1] = mps._LazyS(FakeC([0.9, 0.3, 0.1]))
    psi.S[2] = mps._LazyS(FakeC([0.5, 0.5]))
    # same length: evaluated, and what comes back is the recorded spectrum
    assert np.array_equal(mps._previous_S(psi, 0, 2), [0.8, 0.6]) and calls == [2]
    # different length: dropped without evaluation, the reference's reset value is used
    assert np.array_equal(mps._previous_S(psi, 1, 2), [1.0, 0.0]) and calls == [2]
    # a plain array of the wrong length is reset as well (mps.py:555-556)
    psi.S[1] = np.array([0.7, 0.2, 0.1])
    assert np.array_equal(mps._previous_S(psi, 1, 4), [1.0, 0.0, 0.0, 0.0])
    # reading the attribute evaluates (once) and yields plain arrays
    assert np.array_equal(psi.S[2], [0.5, 0.5]) and calls == [2, 2]
    assert np.array_equal(psi.S[2], [0.5, 0.5]) and calls == [2, 2]
    assert all(isinstance(x, np.ndarray) for x in psi.S)
