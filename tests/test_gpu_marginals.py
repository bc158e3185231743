"""tnac4o.calculate_marginals on the GPU: exact cell marginals on small instances (enumeration / transfer matrices), rotation and
gauge invariance, parity of the HIP pass with its numpy restatement at truncating bond dimensions, constancy of the row
contraction along each row, and the headline size."""
import time

import numpy as np
import pytest

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
    from tnac4o_amd import auxx
    if case == 'ising3x3':
        return mr.exact_ising(mr.ising_3x3_nc2(), 3, 3, 2, beta)
    if case == 'rmf3x3':
        return mr.exact_rmf(auxx.synthetic_rmf(3, 3, 3, 17), beta), None
    return mr.exact_chimera_2x2(auxx.synthetic_chimera(2, 2, 29), beta)


def _close(a, b, tol):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape, k
        err = float(np.max(np.abs(x - y)))
        assert err <= tol, (k, err)


def _row_constant(log2z, tol=1e-10):
    for ny in range(log2z.shape[0]):
        row = log2z[ny]
        assert np.all(np.isfinite(row)), row
        ref = row[0]
        assert np.max(np.abs(row - ref)) <= tol * max(abs(ref), 1.0), (ny, row)


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('case', CASES)
def test_exact_on_small_instances(case, beta):
    ins = _make(case, beta)
    out = ins.calculate_marginals(Dmax=64)
    marg, m = _exact(case, beta)
    assert out is ins.marginals
    _close(ins.marginals, marg, 1e-10)
    if m is None:
        assert ins.magnetization is None
    else:
        assert ins.magnetization.shape == (ins.L,)
        assert float(np.max(np.abs(ins.magnetization - m))) <= 1e-10
    assert ins.marginals_negative <= 0 and ins.marginals_negative > -1e-14
    _row_constant(ins.marginal_row_log2)


@pytest.mark.parametrize('rot', [1, 2, 3])
@pytest.mark.parametrize('case', CASES)
def test_rotation_invariance(case, rot):
    a = _make(case, 3.0)
    a.calculate_marginals(Dmax=64)
    b = _make(case, 3.0)
    b.rotate_graph(rot)
    b.calculate_marginals(Dmax=64)
    assert b.rotation == rot % 4 or case == 'rmf3x3'
    _close(b.marginals, a.marginals, 1e-10)
    if a.magnetization is not None:
        assert float(np.max(np.abs(b.magnetization - a.magnetization))) <= 1e-10


@pytest.mark.parametrize('case', CASES)
def test_gauge_invariance(case):
    a = _make(case, 1.0)
    a.calculate_marginals(Dmax=64)
    b = _make(case, 1.0)
    b.precondition()
    b.calculate_marginals(Dmax=64)
    _close(b.marginals, a.marginals, 1e-9)


def test_leaves_search_results_alone():
    ins = _make('ising3x3', 3.0)
    ins.rotate_graph(1)
    ins.search_ground_state(M=64, Dmax=64)
    keep = {k: np.copy(getattr(ins, k)) for k in ('energy', 'states', 'probability', 'degeneracy', 'Xu', 'Xd', 'Xl', 'Xr', 'order')}
    rot = ins.rotation
    ins.calculate_marginals(Dmax=64)
    for k, v in keep.items():
        assert np.array_equal(getattr(ins, k), v), k
    assert ins.rotation == rot
    marg, _ = _exact('ising3x3', 3.0)
    for k in range(9):                     # the found state's marginal, in the encoding of states[:, k]
        s = int(ins.states[0, k])
        assert abs(ins.marginals[k][s] - marg[k][s]) <= 1e-10


def _parity(ins, tol=1e-11):
    from tnac4o_amd.tnac4o import model_marginals
    P_rot, minP, log2z = mr.row_marginals_np(ins)
    ref, _ = model_marginals(P_rot, ins.order)
    _close(ins.marginals, ref, tol)
    assert abs(ins.marginals_negative - min(float(minP.min()), 0.0)) <= 1e-12
    assert float(np.max(np.abs(ins.marginal_row_log2 - log2z))) <= 1e-9 * max(1.0, float(np.max(np.abs(log2z))))


@pytest.mark.parametrize('rot', [0, 1])
@pytest.mark.parametrize('chi', [8, 16])
def test_kernel_parity_droplet128(chi, rot):
    import tnac4o_amd
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=3.0)
    ins.rotate_graph(rot)
    ins.calculate_marginals(Dmax=chi)
    _parity(ins)
    _row_constant(ins.marginal_row_log2)
    for p in ins.marginals:
        assert abs(p.sum() - 1) < 1e-12 and np.all(p >= 0)
    assert np.all(np.abs(ins.magnetization) <= 1)


def test_kernel_parity_minimal_rmf():
    import tnac4o_amd
    ins = tnac4o_amd.tnac4o(mode='RMF', Nx=5, Ny=3, J=gi.minimal_rmf(), beta=2.0)
    ins.calculate_marginals(Dmax=2)
    _parity(ins)
    _row_constant(ins.marginal_row_log2)
    assert ins.magnetization is None


def test_full_size_chimera():
    """The bench.py instance (synthetic chimera 16 x 16 cells, L = 2048, seed 20260004), beta = 3, chi = 64."""
    import torch
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=synthetic_chimera(16, 16, 20260004), beta=3.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ins.calculate_marginals(Dmax=64)
    torch.cuda.synchronize()
    t_call = time.perf_counter() - t0
    assert len(ins.marginals) == 256
    for p in ins.marginals:
        assert np.all(np.isfinite(p)) and np.all(p >= 0)
        assert abs(p.sum() - 1) <= 1e-12
    assert ins.magnetization.shape == (2048,) and np.all(np.abs(ins.magnetization) <= 1)
    _row_constant(ins.marginal_row_log2)
    t_pass = []
    for _ in range(3):                     # the marginal pass alone, on the boundaries just built
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P_rot, _, _ = ins._marginal_pass()
        torch.cuda.synchronize()
        t_pass.append(time.perf_counter() - t0)
    print('\nmarginals L=2048 chi=64: whole call %.3f s, marginal pass %.1f ms (min of 3: %s ms)'
          % (t_call, 1e3 * min(t_pass), ', '.join('%.1f' % (1e3 * t) for t in t_pass)))
