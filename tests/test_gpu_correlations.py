"""tnac4o.calculate_correlations on the GPU: exact nearest-neighbour correlations, pair marginals and mean energies on small
instances (enumeration / transfer matrices), rotation and gauge invariance, parity of the HIP pass with its numpy restatement at
truncating bond dimensions, the consistency of the tables of one three-layer network, the energy identities, and the headline
size."""
import time

import numpy as np
import pytest

import correlations_ref as cr
import golden_inputs as gi
import marginals_ref as mr

pytestmark = pytest.mark.gpu

BETAS = (0.5, 1.0, 3.0)
CASES = ('ising3x3', 'rmf3x3', 'chimera2x2')


def _make(case, beta):
    import tnac4o_amd
    from tnac4o_amd import auxx
    if case == 'ising3x3':
        return tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=beta)
    if case == 'rmf3x3':
        return tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=3, J=auxx.synthetic_rmf(3, 3, 3, 17), beta=beta)
    return tnac4o_amd.tnac4o(mode='Ising', Nx=2, Ny=2, Nc=8, J=auxx.synthetic_chimera(2, 2, 29), beta=beta)


def _exact(case, beta):
    """(bond_pairs, correlations, pair_marginals, energy_mean) of the model."""
    from tnac4o_amd import auxx
    if case == 'ising3x3':
        pairs, C, Em, _ = cr.exact_ising(mr.ising_3x3_nc2(), 18, beta)
        return pairs, C, None, Em
    if case == 'rmf3x3':
        pm, Em = cr.exact_rmf(auxx.synthetic_rmf(3, 3, 3, 17), beta)
        return None, None, pm, Em
    pairs, C, Em = cr.exact_chimera_2x2(auxx.synthetic_chimera(2, 2, 29), beta)
    return pairs, C, None, Em


def _row_constant(log2z, tol=1e-10):
    for ny in range(log2z.shape[0]):
        row = log2z[ny]
        assert np.all(np.isfinite(row)), row
        assert np.max(np.abs(row - row[0])) <= tol * max(abs(row[0]), 1.0), (ny, row)


def _same_outputs(a, b, tol):
    assert abs(a.energy_mean - b.energy_mean) <= tol * max(1.0, abs(b.energy_mean))
    if b.mode == 'Ising':
        assert np.array_equal(a.bond_pairs, b.bond_pairs)
        assert float(np.max(np.abs(a.correlations - b.correlations))) <= tol
    else:
        assert sorted(a.pair_marginals) == sorted(b.pair_marginals)
        for key, P in b.pair_marginals.items():
            assert a.pair_marginals[key].shape == P.shape, key
            assert float(np.max(np.abs(a.pair_marginals[key] - P))) <= tol, key


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('case', CASES)
def test_exact_on_small_instances(case, beta):
    ins = _make(case, beta)
    out = ins.calculate_correlations(Dmax=64)
    pairs, C, pm, Em = _exact(case, beta)
    if pm is None:
        assert out is ins.correlations and ins.pair_marginals is None
        assert ins.bond_pairs.dtype == np.int64 and np.array_equal(ins.bond_pairs, pairs)
        assert float(np.max(np.abs(ins.correlations - C))) <= 1e-10
    else:
        assert out is ins.pair_marginals and ins.correlations is None
        assert sorted(out) == sorted(pm)
        for key, P in pm.items():
            assert out[key].shape == P.shape
            assert float(np.max(np.abs(out[key] - P))) <= 1e-10, key
    assert abs(ins.energy_mean - Em) <= 1e-10 * abs(Em), (ins.energy_mean, Em)
    assert ins.correlations_negative <= 0 and ins.correlations_negative > -1e-14
    _row_constant(ins.correlation_row_log2)


@pytest.mark.parametrize('rot', [1, 2, 3])
@pytest.mark.parametrize('case', CASES)
def test_rotation_invariance(case, rot):
    a = _make(case, 3.0)
    a.calculate_correlations(Dmax=64)
    b = _make(case, 3.0)
    b.rotate_graph(rot)
    b.calculate_correlations(Dmax=64)
    _same_outputs(b, a, 1e-10)


@pytest.mark.parametrize('case', CASES)
def test_gauge_invariance(case):
    a = _make(case, 1.0)
    a.calculate_correlations(Dmax=64)
    b = _make(case, 1.0)
    b.precondition()
    b.calculate_correlations(Dmax=64)
    _same_outputs(b, a, 1e-9)


def test_leaves_search_results_and_marginals_alone():
    ins = _make('ising3x3', 3.0)
    ins.rotate_graph(1)
    ins.search_ground_state(M=64, Dmax=64)
    ins.calculate_marginals(Dmax=64)
    keep = {k: np.copy(getattr(ins, k)) for k in ('energy', 'states', 'probability', 'degeneracy', 'Xu', 'Xd', 'Xl', 'Xr', 'order',
                                                  'magnetization', 'marginal_row_log2')}
    marg = [np.copy(p) for p in ins.marginals]
    rot, neg = ins.rotation, ins.marginals_negative
    ins.calculate_correlations(Dmax=64)
    for k, v in keep.items():
        assert np.array_equal(getattr(ins, k), v), k
    assert ins.rotation == rot and ins.marginals_negative == neg
    assert all(np.array_equal(p, q) for p, q in zip(ins.marginals, marg))


def _parity(ins, tol=1e-11):
    Pl, Pu, minB, log2z = ins._correlation_pass()
    rPl, rPu, rminB, rlog2z = cr.row_bond_tables_np(ins)
    for c in range(len(Pl)):
        assert Pl[c].shape == rPl[c].shape and Pu[c].shape == rPu[c].shape, c
        assert float(np.max(np.abs(Pl[c] - rPl[c]))) <= tol, c
        assert float(np.max(np.abs(Pu[c] - rPu[c]))) <= tol, c
    assert float(np.max(np.abs(minB - rminB))) <= 1e-12
    assert float(np.max(np.abs(log2z - rlog2z))) <= 1e-9 * max(1.0, float(np.max(np.abs(rlog2z))))
    assert np.array_equal(log2z, ins.correlation_row_log2)            # the pass is deterministic on the same boundaries


def _droplet(beta=3.0, rot=0):
    import tnac4o_amd
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=beta)
    ins.rotate_graph(rot)
    return ins


@pytest.mark.parametrize('rot', [0, 1])
@pytest.mark.parametrize('chi', [8, 16])
def test_kernel_parity_droplet128(chi, rot):
    ins = _droplet(rot=rot)
    ins.calculate_correlations(Dmax=chi)
    _parity(ins)
    _row_constant(ins.correlation_row_log2)
    assert np.all(np.abs(ins.correlations) <= 1 + 1e-12)


def test_kernel_parity_minimal_rmf():
    import tnac4o_amd
    ins = tnac4o_amd.tnac4o(mode='RMF', Nx=5, Ny=3, J=gi.minimal_rmf(), beta=2.0)
    ins.calculate_correlations(Dmax=2)
    _parity(ins)
    _row_constant(ins.correlation_row_log2)
    for key, P in ins.pair_marginals.items():
        assert P.shape == (3, 3) and abs(P.sum() - 1) <= 1e-12, key


def test_consistency_within_one_network():
    """Droplet L=128 at chi = 8 (truncating): the tables of a cell and of its left neighbour come from the same row network."""
    ins = _droplet()
    ins.calculate_marginals(Dmax=8)
    P_rot, minP, mlog2z = ins._marginal_pass()
    ins.calculate_correlations(Dmax=8)
    _row_constant(ins.correlation_row_log2)
    assert float(np.max(np.abs(ins.correlation_row_log2 - ins.marginal_row_log2))) <= 1e-10 * float(np.max(np.abs(mlog2z)))
    Pl, Pu, _, _ = ins._correlation_pass()
    Nx = ins.Nx
    compared = 0
    for ny in range(ins.Ny):
        for nx in range(Nx):
            c = ny * Nx + nx
            p = Pl[c].sum(1)
            assert float(np.max(np.abs(p - Pu[c].sum(1)))) <= 1e-12, c
            if nx > 0:
                rmap = ins._peps_factor(ny, nx - 1)[2]
                left = np.bincount(rmap, weights=Pl[c - 1].sum(1), minlength=Pl[c].shape[1])
                assert float(np.max(np.abs(Pl[c].sum(0) - left))) <= 1e-12, c
            if minP[c] == 0:                # the marginal was not lifted by the negative-probability rule
                assert float(np.max(np.abs(p - P_rot[c]))) <= 1e-12, c
            else:                           # it was: the rule (invariant under scaling) applied to p gives the marginal
                lifted, mn = mr._negative_rule(p)
                assert float(np.max(np.abs(lifted - P_rot[c]))) <= 1e-12, c
                assert abs(mn - minP[c]) <= 1e-12, c
            compared += 1
    assert compared == ins.Nx * ins.Ny


def test_energy_identities():
    """<E> from the tables equals sum J_ij C_ij + sum J_ii m_i (m from the same tables), lies above the ground state and falls
    with beta."""
    from tnac4o_amd.tnac4o import model_marginals
    E0 = gi.golden_groundstate(128, 1)[0]
    Ems = []
    for beta in (0.5, 1.0, 3.0):
        ins = _droplet(beta=beta, rot=1)
        ins.calculate_correlations(Dmax=16)
        Pl, _, _, _ = ins._correlation_pass()
        _, m = model_marginals([t.sum(1) for t in Pl], ins.order, ins.ind0, ins.L)
        J0 = ins.J0
        i, j = ins.bond_pairs[:, 0], ins.bond_pairs[:, 1]
        E = float(np.sum(J0[i, j] * ins.correlations) + J0.diagonal() @ m)
        assert abs(E - ins.energy_mean) <= 1e-10 * abs(E), (E, ins.energy_mean)
        Ems.append(ins.energy_mean)
    assert Ems[2] >= E0 - 1e-9 * abs(E0), (Ems, E0)
    assert Ems[0] > Ems[1] > Ems[2], Ems


def test_full_size_chimera():
    """The bench.py instance (synthetic chimera 16 x 16 cells, L = 2048, seed 20260004), beta = 3, chi = 64."""
    import torch
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, 20260004), beta=3.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ins.calculate_correlations(Dmax=64)
    torch.cuda.synchronize()
    t_call = time.perf_counter() - t0
    assert ins.bond_pairs.shape[0] == ins.correlations.size > 0
    assert np.all(np.isfinite(ins.correlations)) and np.all(np.abs(ins.correlations) <= 1 + 1e-12)
    assert np.isfinite(ins.energy_mean)
    _row_constant(ins.correlation_row_log2)
    t_corr, t_marg = [], []
    for _ in range(3):                     # both passes alone, on the boundaries just built
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Pl, Pu, _, _ = ins._correlation_pass()
        torch.cuda.synchronize()
        t_corr.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        ins._marginal_pass()
        torch.cuda.synchronize()
        t_marg.append(time.perf_counter() - t0)
    assert len(Pl) == len(Pu) == 256
    for t in Pl + Pu:
        assert np.all(np.isfinite(t))
        assert abs(t.sum() - 1) <= 1e-12
    print('\ncorrelations L=2048 chi=64: whole call %.3f s, correlation pass %.1f ms (min of 3: %s ms), marginal pass %.1f ms '
          '(min of 3: %s ms)' % (t_call, 1e3 * min(t_corr), ', '.join('%.1f' % (1e3 * t) for t in t_corr), 1e3 * min(t_marg),
                                 ', '.join('%.1f' % (1e3 * t) for t in t_marg)))
