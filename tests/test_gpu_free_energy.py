"""tnac4o.calculate_free_energy on the GPU: exact log2 Z and entropy on the enumerable instances in every rotation and gauge, every
term against numpy on the same truncated boundaries, the cancellation of the norm and sign of the interior boundaries, and the link
to the per-sample estimates of sample_boltzmann."""
import numpy as np
import pytest

import free_energy_ref as fr
import sampling_ref as sref
from guarded import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_sampling import BETAS, CASES, droplet, small      # noqa: E402  (helpers only, no test is imported)

LN2 = float(np.log(2.0))


def _check_exact(ins, case, beta, rot=0):
    exact = fr.exact_log2Z(case, beta)
    Ny = ins.Ny
    assert ins.log2Z_rows.shape == (Ny,) and ins.log2Z_overlaps.shape == (Ny - 1,)
    print('%s beta %.1f rot %d: log2 Z = %.12f (exact %.12f, off by %.3e), row spread %.3e'
          % (case, beta, rot, ins.log2Z, exact, ins.log2Z - exact, ins.free_energy_row_spread))
    assert abs(ins.log2Z - exact) <= 1e-10
    assert ins.free_energy == pytest.approx(-exact * LN2 / beta, abs=1e-9)
    assert ins.free_energy_row_spread <= 1e-10
    if case in ('ising3x3', 'rmf3x3'):
        S = fr.exact_entropy(case, beta)
        print('    entropy %.12f (exact %.12f), <E> = %.12f' % (ins.entropy, S, ins.energy_mean))
        assert abs(ins.entropy - S) <= 1e-9
        assert abs(ins.entropy - (ins.log2Z * LN2 + beta * ins.energy_mean)) <= 1e-12 * max(1.0, abs(ins.entropy))


# ---------------------------------------------------------------------------------------------- 8. exact
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('case', CASES)
def test_exact(case, beta):
    ins = small(case, beta)
    out = ins.calculate_free_energy(Dmax=64)
    assert out == ins.log2Z
    _check_exact(ins, case, beta)


@pytest.mark.parametrize('rot', [1, 2, 3])
@pytest.mark.parametrize('case', CASES)
def test_exact_rotated(case, rot):
    ins = small(case, 1.0)
    ins.rotate_graph(rot)
    ins.calculate_free_energy(Dmax=64)
    _check_exact(ins, case, 1.0, rot)


@pytest.mark.parametrize('case', CASES)
def test_exact_after_precondition(case):
    """The gauges on the vertical bonds sit in the boundaries and in the rows alike: Z does not move."""
    ins = small(case, 1.0)
    ins.precondition()
    print('largest gauge deviation from 1: %.3e' % max(float(np.max(np.abs(x - 1.0))) for x in (ins.Xu, ins.Xd)))
    ins.calculate_free_energy(Dmax=64)
    _check_exact(ins, case, 1.0)


# ---------------------------------------------------------------------------------------------- 9. truncated, against numpy
def _truncated(which):
    if which == 'droplet':
        return droplet(), 8
    return small('rmf3x3', 3.0), 2


@pytest.mark.parametrize('which', ['droplet', 'rmf3x3'])
def test_truncated_against_numpy_on_the_same_boundaries(which):
    ins, chi = _truncated(which)
    ins.calculate_free_energy(Dmax=chi)
    assert max(float(d) for d in ins.rhoT_discarded) > 0 and max(float(d) for d in ins.rhoB_discarded) > 0
    ref, rows, cuts = fr.log2Z_np(ins)
    Ny = ins.Ny
    dr, dc = np.abs(ins.log2Z_rows - rows), np.abs(ins.log2Z_overlaps - cuts)
    print('%s chi %d: log2 Z = %.10f, numpy %.10f; rows off by at most %.3e, overlaps %.3e, total %.3e; row spread %.3e'
          % (which, chi, ins.log2Z, ref, dr.max(), dc.max(), abs(ins.log2Z - ref), ins.free_energy_row_spread))
    assert float(dr.max()) <= 1e-10 and float(dc.max()) <= 1e-10
    assert abs(ins.log2Z - ref) <= (2 * Ny - 1) * 1e-10
    assert ins.free_energy_row_spread <= 1e-10
    if which == 'rmf3x3':                                                # the truncation is felt, and the estimate stays near
        exact = fr.exact_log2Z('rmf3x3', 3.0)
        assert 1e-9 < abs(ins.log2Z - exact) < 1e-2


# ---------------------------------------------------------------------------------------------- 10. cancellation
@pytest.mark.parametrize('which', ['droplet', 'rmf3x3'])
def test_norm_and_sign_of_the_interior_boundaries_cancel(which):
    ins, chi = _truncated(which)
    Z0 = ins.calculate_free_energy(Dmax=chi)
    rows0, cuts0, Em0 = np.copy(ins.log2Z_rows), np.copy(ins.log2Z_overlaps), ins.energy_mean
    assert ins.calculate_free_energy(boundary='keep') == Z0              # the same boundaries: the same number
    ins.rhoT[2].A[1].mul_(-3.7)
    ins.rhoB[1].A[ins.Nx - 1].mul_(0.25)
    Z1 = ins.calculate_free_energy(boundary='keep')
    print('%s: log2 Z moved by %.3e; rows by %s, overlaps by %s' % (which, Z1 - Z0, ins.log2Z_rows - rows0, ins.log2Z_overlaps - cuts0))
    assert abs(Z1 - Z0) <= 1e-11
    # the terms did move: row 1 holds both factors, overlap 1 the second, overlap 2 the first
    assert ins.log2Z_rows[1] - rows0[1] == pytest.approx(np.log2(3.7) - 2.0, abs=1e-9)
    assert ins.log2Z_overlaps[0] - cuts0[0] == pytest.approx(-2.0, abs=1e-9)
    assert ins.log2Z_overlaps[1] - cuts0[1] == pytest.approx(np.log2(3.7), abs=1e-9)
    assert ins.energy_mean == pytest.approx(Em0, abs=1e-9)


# ---------------------------------------------------------------------------------------------- 11. link to sampling
@pytest.mark.parametrize('case', ['ising3x3', 'chimera2x2'])
def test_link_to_sampling(case):
    """Exact contraction: every sample's estimate of log2 Z is the number calculate_free_energy returns."""
    ins = small(case, 1.0)
    np.random.seed(99)
    ins.sample_boltzmann(M=256, Dmax=64)
    keep = {k: np.copy(getattr(ins, k)) for k in ('energy', 'states', 'probability', 'sample_log2Z', 'Xu', 'Xd', 'Xl', 'Xr', 'order')}
    rot = ins.rotation
    Z = ins.calculate_free_energy(Dmax=64)
    dev = float(np.max(np.abs(ins.sample_log2Z - Z)))
    print('%s: largest |sample_log2Z - log2Z| = %.3e over %d samples' % (case, dev, ins.sample_log2Z.size))
    assert ins.sample_log2Z.shape == (256,) and dev <= 2e-10
    for k, v in keep.items():
        assert same_bits(np.asarray(getattr(ins, k)), v), k
    assert ins.rotation == rot
