"""CPU checks of the thermal-marginal surface: argument errors of the new library entry points (no GPU needed) and the host
mapping from rotated-frame cell marginals to model order and magnetisations."""
import ctypes

import numpy as np
import pytest

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


def test_env3_argument_errors():
    L = _lib()
    host = (ctypes.c_double * 64)()
    P = ctypes.cast(host, ctypes.c_void_p)               # a host address standing in for device memory: never dereferenced
    dims = (4, 2, 4, 2, 2, 2, 4, 4)
    for side in (0, 1):
        assert L.tn_env3_ws_bytes(side, *dims) > 0
    assert L.tn_env3_ws_bytes(2, *dims) == 0
    assert L.tn_env3_ws_bytes(0, 4, 0, 4, 2, 2, 2, 4, 4) == 0
    big = 1 << 30
    _expect_neg(L, L.tn_env3(0, None, P, P, P, *dims, None, P, P, None, P, big, None), 'null operand')
    _expect_neg(L, L.tn_env3(1, P, P, P, P, *dims, None, None, P, None, P, big, None), 'null operand')
    _expect_neg(L, L.tn_env3(0, P, P, P, P, *dims, None, P, P, None, None, big, None), 'null operand')
    _expect_neg(L, L.tn_env3(0, P, P, P, P, 4, 2, 4, 2, -2, 2, 4, 4, None, P, P, None, P, big, None), 'non-positive dimension')
    _expect_neg(L, L.tn_env3(1, P, P, P, P, 4, 2, 0, 2, 2, 2, 4, 4, None, P, P, None, P, big, None), 'non-positive dimension')
    _expect_neg(L, L.tn_env3(3, P, P, P, P, *dims, None, P, P, None, P, big, None), 'side')
    need = L.tn_env3_ws_bytes(1, *dims)
    _expect_neg(L, L.tn_env3(1, P, P, P, P, *dims, None, P, P, None, P, need - 1, None), 'workspace too small')


def test_cluster_marginal_argument_errors():
    L = _lib()
    host = (ctypes.c_double * 64)()
    P = ctypes.cast(host, ctypes.c_void_p)
    assert L.tn_cluster_marginal_ws_bytes(2, 2, 2, 2, 16) > 0
    assert L.tn_cluster_marginal_ws_bytes(2, 0, 2, 2, 16) == 0
    big = 1 << 30

    def cm(HL=P, F=P, dm=P, out=P, q=16, bl=2, pd=2, br=2, pu=2, K=16, ws=P, wsb=big):
        return L.tn_cluster_marginal(HL, P, F, dm, P, q, bl, pd, br, pu, K, None, None, out, P, P, ws, wsb, None)
    _expect_neg(L, cm(HL=None), 'null operand')
    _expect_neg(L, cm(F=None), 'null operand')
    _expect_neg(L, cm(dm=None), 'null operand')
    _expect_neg(L, cm(out=None), 'null operand')
    _expect_neg(L, cm(ws=None), 'null operand')
    _expect_neg(L, cm(q=0), 'non-positive dimension')
    _expect_neg(L, cm(K=-1), 'non-positive dimension')
    _expect_neg(L, cm(q=1 << 20), 'cell states')
    need = L.tn_cluster_marginal_ws_bytes(2, 2, 2, 2, 16)
    _expect_neg(L, cm(wsb=need - 1), 'workspace too small')


@pytest.mark.parametrize('beta', [0.5, 3.0])
def test_model_order_and_magnetisation_under_rotation(beta):
    """Exact cell marginals of the ROTATED lattice (enumeration with the rotated couplings and cell structure) must come back in
    model order as the model's own exact marginals, with the model's exact magnetisations (spin 9 is inactive: exactly 0)."""
    import tnac4o_amd
    from tnac4o_amd.tnac4o import model_marginals
    J = mr.ising_3x3_nc2()
    ref_marg, ref_m = mr.exact_ising(J, 3, 3, 2, beta)
    assert ref_marg[4].size == 2                            # the cell holding the inactive spin
    for rot in range(4):
        ins = tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=J, beta=beta)
        ins.rotate_graph(rot)
        rows, cols = np.nonzero(ins.J)
        Jrot = [[int(i), int(j), float(ins.J[i, j])] for i, j in zip(rows, cols)]
        P_rot, _ = mr.exact_ising(Jrot, ins.Nx, ins.Ny, 2, beta)
        for ny in range(ins.Ny):                             # the enumeration's cells are the solver's rotated cells
            for nx in range(ins.Nx):
                assert P_rot[ny * ins.Nx + nx].size == ins.N[ny][nx]
        marg, m = model_marginals(P_rot, ins.order, ins.ind0, ins.L)
        assert len(marg) == 9
        for k in range(9):
            np.testing.assert_allclose(marg[k], ref_marg[k], rtol=0, atol=1e-12, err_msg='rot %d cell %d' % (rot, k))
        np.testing.assert_allclose(m, ref_m, rtol=0, atol=1e-12)
        assert m[9] == 0.0
        assert np.all(np.abs(m) <= 1)


def test_model_order_rmf_under_rotation():
    """RMF: no magnetisation; the cell order of a 3 x 2 lattice (not square) maps back under every rotation."""
    import tnac4o_amd
    from tnac4o_amd import auxx
    from tnac4o_amd.tnac4o import model_marginals
    J = auxx.synthetic_rmf(3, 2, 3, 4)
    ref = mr.exact_rmf(J, 1.0)
    for rot in range(4):
        ins = tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=2, J=J, beta=1.0)
        ins.rotate_graph(rot)
        Jr = {'fun': ins.J['fun'], 'fac': ins.J['fac'], 'N': ins.N, 'Nx': ins.Nx, 'Ny': ins.Ny}
        P_rot = mr.exact_rmf(Jr, 1.0)
        marg, m = model_marginals(P_rot, ins.order)
        assert m is None
        for k in range(6):
            np.testing.assert_allclose(marg[k], ref[k], rtol=0, atol=1e-13)


def test_exact_references_agree_on_a_shared_case():
    """The ring-of-transfer-matrices reference against plain enumeration, on couplings small enough to enumerate: the 2 x 2
    chimera with every spin but two of each cell switched off (4 x 2 = 8 active spins)."""
    from tnac4o_amd import auxx
    J = auxx.synthetic_chimera(2, 2, 3)
    keep = {c * 8 + m for c in range(4) for m in (0, 4)}
    Js = [r for r in J if r[0] in keep and r[1] in keep]
    # the ring reference needs all 8 spins of a cell active: give the others a field only
    Js += [[i, i, 0.25] for i in range(32) if i not in keep]
    ring, ring_m = mr.exact_chimera_2x2(Js, 1.5)
    # enumeration over the 8 coupled spins; the field-only spins are independent
    idx = sorted(keep)
    Jsub = [[idx.index(i), idx.index(j), v] for i, j, v in Js if i in keep and j in keep]
    binary = ((np.arange(256)[:, None] >> np.arange(8)[None, :]) & 1).astype(np.int8)
    E = auxx.energy_Jij(Jsub, binary)
    w = np.exp(-1.5 * (E - E.min()))
    w /= w.sum()
    m_sub = w @ (2.0 * binary - 1.0)
    np.testing.assert_allclose(ring_m[idx], m_sub, rtol=0, atol=1e-12)
    free = [i for i in range(32) if i not in keep]
    np.testing.assert_allclose(ring_m[free], np.tanh(-1.5 * 0.25), rtol=0, atol=1e-12)
    for c in range(4):
        assert abs(ring[c].sum() - 1) < 1e-12
