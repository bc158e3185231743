"""CPU checks of the thermal-correlation surface: argument errors of tn_cluster_bond_marginal and its workspace query (no GPU
needed), and the host mapping of rotated-frame bond tables to model-frame correlations, pair marginals and the mean energy."""
import ctypes

import numpy as np
import pytest

import correlations_ref as cr
import marginals_ref as mr


def _lib():
    from tnac4o_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _msg(L):
    buf = ctypes.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    return buf.value.decode()


def _expect_neg(L, rc, text):
    assert rc < 0, rc
    assert text in _msg(L), _msg(L)


def test_cluster_bond_marginal_argument_errors():
    L = _lib()
    host = (ctypes.c_double * 64)()
    P = ctypes.cast(host, ctypes.c_void_p)               # a host address standing in for device memory: never dereferenced
    assert L.tn_cluster_bond_marginal_ws_bytes(16, 2, 2, 2, 2, 16) > L.tn_cluster_marginal_ws_bytes(2, 2, 2, 2, 16)
    assert L.tn_cluster_bond_marginal_ws_bytes(0, 2, 2, 2, 2, 16) == 0
    assert L.tn_cluster_bond_marginal_ws_bytes(16, 2, 2, -2, 2, 16) == 0
    big = 1 << 30

    def cbm(HL=P, HR=P, F=P, rm=P, Pl=P, Pu=P, mB=P, lz=P, q=16, bl=2, pd=2, br=2, pu=2, K=16, ws=P, wsb=big):
        return L.tn_cluster_bond_marginal(HL, HR, F, P, rm, q, bl, pd, br, pu, K, None, None, Pl, Pu, mB, lz, ws, wsb, None)
    for kw in ('HL', 'HR', 'F', 'rm', 'Pl', 'Pu', 'mB', 'lz', 'ws'):
        _expect_neg(L, cbm(**{kw: None}), 'null operand')
    _expect_neg(L, cbm(q=0), 'non-positive dimension')
    _expect_neg(L, cbm(pu=0), 'non-positive dimension')
    _expect_neg(L, cbm(K=-1), 'non-positive dimension')
    _expect_neg(L, cbm(q=16385), 'cell states')
    need = L.tn_cluster_bond_marginal_ws_bytes(16, 2, 2, 2, 2, 16)
    _expect_neg(L, cbm(wsb=need - 1), 'workspace too small')


@pytest.mark.parametrize('beta', [0.5, 3.0])
def test_model_correlations_ising_under_rotation(beta):
    """Exact bond tables of the ROTATED lattice (enumeration with the rotated couplings and bond indices) must give the model's own
    exact correlations on every coupling and its exact mean energy, under all four rotations."""
    import tnac4o_amd
    from tnac4o_amd.tnac4o import model_correlations
    J = mr.ising_3x3_nc2()
    pairs, C, Em, _ = cr.exact_ising(J, 18, beta)
    assert len(pairs) == 18 and not np.any(pairs == 9)     # 8 intra-cell, 4 right, 6 down; spin 9 is inactive
    for rot in range(4):
        ins = tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=J, beta=beta)
        ins.rotate_graph(rot)
        Pl, Pu = cr.enum_bond_tables(ins)
        for c in range(9):
            np.testing.assert_allclose(Pl[c].sum(1), Pu[c].sum(1), rtol=0, atol=1e-13)
        bp, Cm = model_correlations(Pl, Pu, ins.order, ins.Nx, ins.Ny, J0=ins.J0, ind=ins.ind, ir=ins.ir, idn=ins.id)
        assert bp.dtype == np.int64 and np.array_equal(bp, pairs), rot
        assert np.all(bp[:, 0] < bp[:, 1])
        np.testing.assert_allclose(Cm, C, rtol=0, atol=1e-12, err_msg='rot %d' % rot)
        assert abs(ins._bond_energy(Pl, Pu) - Em) <= 1e-12 * max(1.0, abs(Em))


def test_model_correlations_rmf_key_order():
    """RMF on a 3 x 2 lattice (not square) with half the two-cell keys given in reverse order (tables transposed, so the model is
    the same): pair marginals come back under the user's keys, in each key's order, under every rotation."""
    import tnac4o_amd
    from tnac4o_amd import auxx
    from tnac4o_amd.tnac4o import model_correlations
    J = auxx.synthetic_rmf(3, 2, 3, 4)
    fac, fun, k = {}, dict(J['fun']), 0
    for key, val in J['fac'].items():
        if len(key) == 4 and k % 2 == 0:
            fun[val] = J['fun'][val].T.copy()
            key = key[2:] + key[:2]
        k += len(key) == 4
        fac[key] = val
    J = dict(J, fac=fac, fun=fun)
    ref, Em = cr.exact_rmf(J, 1.0)
    assert any(key[0] * 3 + key[1] > key[2] * 3 + key[3] for key in ref)
    for rot in range(4):
        ins = tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=2, J=J, beta=1.0)
        ins.rotate_graph(rot)
        Pl, Pu = cr.enum_bond_tables(ins)
        out = model_correlations(Pl, Pu, ins.order, ins.Nx, ins.Ny, keys=list(ins.J['fac']), Nx_model=ins.Nx_model)
        assert sorted(out) == sorted(ref)
        for key, P in ref.items():
            np.testing.assert_allclose(out[key], P, rtol=0, atol=1e-13, err_msg='rot %d key %s' % (rot, key))
        assert abs(ins._bond_energy(Pl, Pu) - Em) <= 1e-12 * max(1.0, abs(Em))


def test_model_correlations_rejects_distant_couplings():
    import tnac4o_amd
    from tnac4o_amd.tnac4o import model_correlations
    J = mr.ising_3x3_nc2()
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=J, beta=1.0)
    Pl, Pu = cr.enum_bond_tables(ins)
    J0 = ins.J0.copy()
    J0[0, 16] = 0.5                                     # cell 0 to cell 8: not neighbours
    with pytest.raises(ValueError):
        model_correlations(Pl, Pu, ins.order, 3, 3, J0=J0, ind=ins.ind, ir=ins.ir, idn=ins.id)


def test_chimera_ring_reference_against_enumeration():
    """The ring reference for pair correlations and <E>, against plain enumeration on a 2 x 2 chimera with two coupled spins per
    cell and field-only spins elsewhere."""
    from tnac4o_amd import auxx
    J = auxx.synthetic_chimera(2, 2, 3)
    keep = {c * 8 + m for c in range(4) for m in (0, 4)}
    Js = [r for r in J if r[0] in keep and r[1] in keep] + [[i, i, 0.25] for i in range(32) if i not in keep]
    pairs, C, Em = cr.exact_chimera_2x2(Js, 1.5)
    idx = sorted(keep)
    Jsub = [[idx.index(i), idx.index(j), v] for i, j, v in Js if i in keep and j in keep]
    sp, sC, sE, _ = cr.exact_ising(Jsub, 8, 1.5)
    assert np.array_equal(np.array(idx)[sp], pairs)
    np.testing.assert_allclose(C, sC, rtol=0, atol=1e-12)
    free = 24 * 0.25 * np.tanh(-1.5 * 0.25)            # <E> of the 24 independent field-only spins
    assert abs(Em - (sE + free)) <= 1e-10
