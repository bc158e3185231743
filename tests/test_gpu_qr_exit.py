"""The rank-revealing exit of tn_qr / tn_qr_batched / tn_site_qr (reveal_check in csrc/qr.hip) against the longdouble reference and
the restated rule of tests/qr_exit_ref.py: the exit column, orthonormal Q, upper-trapezoidal R, the column-wise residual of the
header's contract, the norm of the dropped block, the attach products and the Q^T / R^T layout of side 1, the norm factor.  The
inputs keep every checkpoint ratio a factor 1.5 away from 1 (tests/test_qr_exit_host.py), so the exit column is held exactly.

Bounds: 5e-14 for orthogonality and for the column-relative residual is check_qr's (tests/test_gpu_kernels.py); after an exit the
residual of column j may exceed it by rank_tol x (1 + 1e-6) x the scale of the rule that was asked for -- the largest column norm of
the input, or its Frobenius norm with frobenius_exit -- which is what the exit test has verified about every column that is left."""
import os

import numpy as np
import pytest

import qr_exit_ref as qx

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

LD = np.longdouble
LAPACK_FACTOR = 8.0
check_factors = qx.check_factors


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def ops():
    from tnac4o_amd import ops as o
    return o


def _with_env(name, value, fn):
    saved = os.environ.get(name)
    try:
        os.environ[name] = value
        return fn()
    finally:
        if saved is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = saved


def run_qr(ops, M, rank_tol, colmajor):
    """tn_qr on a copy of M, row-major (orth_left's strides) or as the column-major view of a row-major n x m array with Q^T and R^T
    as outputs (orth_right's).  The outputs start as NaN: whatever the call reports as produced must have been written."""
    m, n = M.shape
    k = min(m, n)
    nan = lambda *sh: torch.full(sh, float('nan'), dtype=torch.float64, device='cuda')
    if colmajor:
        T, Q, R = dev(M.T).t(), nan(k, m).t(), nan(n, k).t()
    else:
        T, Q, R = dev(M), nan(m, k), nan(k, n)
    _, _, keff = ops.qr_into(T, Q, R, rank_tol=rank_tol)
    return host(Q)[:, :keff], host(R)[:keff], keff


# ------------------------------------------------------------------------------------------------------------------ tn_qr
@pytest.mark.parametrize('colmajor', [False, True])
@pytest.mark.parametrize('name', list(qx.INPUTS))
def test_qr_exit_against_reference(ops, name, colmajor):
    c = qx.INPUTS[name]
    ref = qx.reference(name)
    k_ref, _, trailing2 = qx.exit_reference(ref.M, c.rank_tol, False, R=ref.R)
    Q, R, keff = run_qr(ops, c.build(), c.rank_tol, colmajor)
    assert keff == k_ref == c.k
    check_factors(ref, Q, R, keff, c.rank_tol, False, trailing2, c.noisy, '%s colmajor=%d' % (name, colmajor))
    if not ref.col2.any():                                           # the zero matrix (qr_into has checked the return code)
        assert not R.any()


@pytest.mark.parametrize('colmajor', [False, True])
@pytest.mark.parametrize('name', qx.WELL_CONDITIONED)
def test_qr_exit_factors_entrywise(ops, name, colmajor):
    """Where the leading keff columns are well conditioned their factorisation is unique, and two backward-stable algorithms differ by
    a modest multiple of each one's own error.  The yardstick is the distance of float64 numpy.linalg.qr (signs fixed) from the
    longdouble reference on the same input, measured here as (max |dQ|, max_j ||dR[:, j]|| / ||M[:, j]||) over the leading keff
    columns of Q / rows of R:  'graded' (keff 128): 2.9e-16, 5.9e-16;  'no_exit' (keff 160): 1.5e-7, 2.5e-15 (its last 20 columns
    of Q are fixed by the 1e-9 noise alone, to 1e-16 / 1e-9).  The kernel may lie 8 times as far away."""
    c = qx.INPUTS[name]
    Q, R, keff = run_qr(ops, c.build(), c.rank_tol, colmajor)
    assert keff == c.k
    dq, dr = qx.lapack_deviation(name, keff)
    Ql, Rl = qx.q_reference(name)
    cn = np.sqrt(np.asarray(qx.reference(name).col2, dtype=np.float64))
    gq = float(np.abs(Q - Ql[:, :keff]).max())
    dR = np.asarray(R - Rl[:keff], dtype=np.float64)
    gr = float((np.sqrt((dR * dR).sum(0)) / cn).max())
    print(name, 'colmajor', colmajor, 'Q: kernel', gq, 'LAPACK', dq, ' R: kernel', gr, 'LAPACK', dr)
    assert gq <= LAPACK_FACTOR * dq and gr <= LAPACK_FACTOR * dr


def test_qr_exit_column_same_on_every_launch_form(ops):
    """The single-launch and the six-launch panel step, the merged and the panel-by-panel Q accumulation: one exit column (their
    factors are held bit-identical elsewhere)."""
    c = qx.INPUTS['merged_q']
    M = c.build()
    for fused in '01':
        for merged in '01':
            keff = _with_env('TN_PANEL_FUSED', fused, lambda: _with_env('TN_QR_MERGED_Q', merged, lambda: run_qr(ops, M, c.rank_tol, False)[2]))
            assert keff == c.k, (fused, merged)


# ------------------------------------------------------------------------------------------------------------------ tn_site_qr
@pytest.mark.parametrize('frob', [False, True])
@pytest.mark.parametrize('side', [0, 1])
@pytest.mark.parametrize('name', list(qx.SITES))
def test_site_qr_exit_against_reference(ops, name, side, frob):
    """ops.site_qr with normalise=True against site_matrix in longdouble: the attach product, the side-1 layout (Q^T, R^T), the exit
    column under the rule asked for, the norm factor taken by the library (run to the end) or by the wrapper (after an exit), and
    'dropped2'."""
    s = qx.SITES[name]
    ref = qx.site_reference(name, side)
    m, n = ref.M.shape
    full = min(m, n)
    k_ref, _, trailing2 = qx.exit_reference(ref.M, s.rank_tol, frob, R=ref.R)
    assert k_ref == (s.k_frob if frob else s.k)
    A, C = qx.site_operands(name, side)
    info = {}
    Qd, Rd, k, nf = ops.site_qr(side, dev(A), None if C is None else dev(C), s.rank_tol, True, info, frobenius_exit=frob)
    label = '%s side=%d frob=%d' % (name, side, frob)
    assert k == k_ref, label
    assert Qd.is_contiguous() and Rd.is_contiguous(), label
    assert tuple(Qd.shape) == ((m, k) if side == 0 else (k, m)) and tuple(Rd.shape) == ((k, n) if side == 0 else (n, k)), label
    Q, R = (host(Qd), host(Rd)) if side == 0 else (host(Qd).T, host(Rd).T)
    nf0, nf1 = (float(v) for v in host(nf))
    assert np.frexp(nf0)[0] == 0.5 and nf0 * nf1 == 1.0, label       # a power of two and its inverse
    assert 1.0 <= np.abs(R).max() < 2.0, label
    res = check_factors(ref, Q, nf0 * R, k, s.rank_tol, frob, trailing2, s.noisy, label)
    d2 = info['dropped2']
    if k == full:
        assert d2 == 0.0, label
        return
    fro = float(np.sqrt(ref.col2.sum()))
    print(label, 'sqrt(dropped2) - ||M - Q R||_F over ||M||_F', (np.sqrt(d2) - res) / fro)
    assert abs(np.sqrt(d2) - res) <= 1e-12 * fro, label
    if s.noisy:
        print(label, 'dropped2 / reference - 1', d2 / trailing2 - 1)
        assert abs(d2 - trailing2) <= 1e-5 * trailing2, label


# ------------------------------------------------------------------------------------------------------------------ tn_qr_batched
@pytest.mark.parametrize('nside', [0, 2])
def test_qr_batched_exit(ops, nside):
    """Four 300 x 160 items that leave at 64, at 128, not at all, and at 64 as the zero matrix: every item's own exit column, and the
    factors of its own tn_qr call bit for bit."""
    items = [qx.INPUTS[name].build() for name in qx.BATCH]
    tol = qx.INPUTS[qx.BATCH[0]].rank_tol
    assert all(qx.INPUTS[name].rank_tol == tol for name in qx.BATCH) and [qx.INPUTS[name].k for name in qx.BATCH] == qx.BATCH_KEFF
    sides = [torch.cuda.Stream() for _ in range(nside)]
    Q, R, keff = ops.qr_batched(dev(np.stack(items)), side_streams=sides, rank_tol=tol)
    torch.cuda.synchronize()
    assert keff == qx.BATCH_KEFF
    for i, M in enumerate(items):
        Q1, R1, k1 = run_qr(ops, M, tol, False)
        assert k1 == keff[i]
        assert np.array_equal(host(Q[i])[:, :k1], Q1) and np.array_equal(host(R[i])[:k1], R1), qx.BATCH[i]
