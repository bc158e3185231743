"""The panel-pivoted, truncating QR of tn_site_qr (pivot_perm_host != NULL: colnorm2_kernel, the Frobenius exit test, the selection of the
32 largest residuals on the device -- pivot_select_kernel, swap_columns_dev_kernel, the verdict ring -- or on the host -- pivot_on_host,
select_pivots, compose_swaps --, csrc/qr.hip) against the longdouble reference and the restated rule of tests/qr_pivot_ref.py: the
accepted rank, the leading permutation under the tie rule of the form that ran, orthonormal Q, upper-trapezoidal R, the column-wise
residual, the dropped norm, the attach product, both sides' layouts, and the factors entrywise where they are well conditioned.  The
inputs keep every exit ratio a factor 1.5 away from 1 and every gap among the 33 largest residuals above 1e-4
(tests/test_qr_pivot_host.py), so rank and leading permutation are held exactly.

Bounds: those of tests/test_gpu_qr_exit.py (qr_exit_ref.check_factors, the Frobenius rule), taken over unchanged."""
import os

import numpy as np
import pytest

import qr_exit_ref as qx
import qr_pivot_ref as qp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

LD = np.longdouble
LAPACK_FACTOR = 8.0


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def ops():
    from tnac4o_amd import ops as o
    return o


def _with_env(env, fn):
    saved = {name: os.environ.get(name) for name in env}
    try:
        os.environ.update(env)
        return fn()
    finally:
        for name, v in saved.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


_runs = {}


def run_site(ops, name, side, device_form, **env):
    """ops.site_qr of a site of qp.SITES with panel pivoting: (Q (m x k), R (k x n), k, perm, dropped2) on the host, the layout of the
    device outputs checked on the way.  One run per (site, side, form) and process."""
    key = (name, side, device_form, tuple(sorted(env.items())))
    if key in _runs:
        return _runs[key]
    s = qp.SITES[name]
    A, C = qp.site_operands(name, side)
    m, n = (s.p * (A.shape[0] if C is None else s.kc), A.shape[2]) if side == 0 else (s.p * (A.shape[2] if C is None else s.kc), A.shape[0])
    info = {}
    env = dict(env, TN_PIVOT_DEVICE=str(device_form))
    Qd, Rd, k, nf = _with_env(env, lambda: ops.site_qr(side, dev(A), None if C is None else dev(C), qp.INPUTS[s.core].rank_tol, False, info,
                                                       frobenius_exit=True, pivot=True))
    label = '%s side=%d device=%d' % (name, side, device_form)
    assert nf is None and Qd.is_contiguous() and Rd.is_contiguous(), label
    assert tuple(Qd.shape) == ((m, k) if side == 0 else (k, m)) and tuple(Rd.shape) == ((k, n) if side == 0 else (n, k)), label
    Q, R = (host(Qd), host(Rd)) if side == 0 else (host(Qd).T, host(Rd).T)
    perm = host(info['perm'])
    assert perm.shape == (n,) and sorted(perm.tolist()) == list(range(n)), label
    _runs[key] = (Q, R, k, perm, info['dropped2'])
    return _runs[key]


@pytest.mark.parametrize('device_form', [1, 0])
@pytest.mark.parametrize('side', [0, 1])
@pytest.mark.parametrize('name', list(qp.SITES))
def test_pivoted_site_qr_against_reference(ops, name, side, device_form):
    """Every site x side x selection form: k and perm[:k] exactly, then everything check_factors asks of M[:, perm] ~ Q R with the
    permutation the call returned, and 'dropped2'."""
    c = qp.INPUTS[qp.SITES[name].core]
    ref = qp.site_reference(name, side, qp.tie_rule(name, device_form))
    m, n = ref.M.shape
    Q, R, k, perm, d2 = run_site(ops, name, side, device_form)
    label = '%s side=%d device=%d' % (name, side, device_form)
    assert k == ref.keff == c.k, label
    assert np.array_equal(perm[:k], ref.perm[:k]), (label, perm[:k], ref.perm[:k])
    permuted = qx.Ref(ref.M[:, perm], None, ref.col2[perm])
    res = qx.check_factors(permuted, Q, R, k, c.rank_tol, True, ref.dropped2, c.noisy, label)
    if not ref.col2.any():                                            # the zero matrix
        assert perm.tolist() == list(range(n)) and not R.any() and d2 == 0.0, label
    if k == min(m, n):
        assert d2 == 0.0, label
        return
    fro = float(np.sqrt(ref.col2.sum()))
    print(label, 'sqrt(dropped2) - ||M - Q R||_F over ||M||_F', (np.sqrt(d2) - res) / fro if fro else 0.0)
    assert abs(np.sqrt(d2) - res) <= 1e-12 * fro, label
    if c.noisy:
        print(label, 'dropped2 / reference - 1', d2 / ref.dropped2 - 1)
        assert abs(d2 - ref.dropped2) <= 1e-5 * ref.dropped2, label


@pytest.mark.parametrize('device_form', [1, 0])
@pytest.mark.parametrize('side', [0, 1])
@pytest.mark.parametrize('name', list(qp.ENTRYWISE))
def test_pivoted_site_qr_factors_entrywise(ops, name, side, device_form):
    """Where the leading columns of M[:, perm] are well conditioned (all 160 of 'no_exit', the accepted 128 of 'graded_exit', 96 of the
    rank 100 of 'exit_128_tall') their factorisation is unique: Q's leading columns and R's leading rows -- R's columns behind the rank
    taken through perm -- lie within 8 x the distance of float64 numpy.linalg.qr of the same permuted input from the longdouble
    reference, in the two measures of test_qr_exit_factors_entrywise (max |dQ|, max_j ||dR[:, j]|| / ||M[:, j]||)."""
    kk = qp.ENTRYWISE[name]
    ref = qp.site_reference(name, side, qp.tie_rule(name, device_form))
    Q, R, k, perm, _ = run_site(ops, name, side, device_form)
    assert k == ref.keff and np.array_equal(perm[:k], ref.perm[:k])
    dq, dr = qp.lapack_deviation(ref, qp.INPUTS[name].build(), kk)
    Rin = np.empty_like(R)
    Rin[:, perm] = R                                                  # by input column
    cn = np.sqrt(np.asarray(ref.col2[ref.perm], dtype=np.float64))
    gq = float(np.abs(Q[:, :kk] - ref.Q[:, :kk]).max())
    dR = np.asarray(Rin[:kk, ref.perm] - ref.R[:kk], dtype=np.float64)
    gr = float((np.sqrt((dR * dR).sum(0)) / cn).max())
    print(name, 'side', side, 'device', device_form, 'Q: kernel', gq, 'LAPACK', dq, ' R: kernel', gr, 'LAPACK', dr)
    assert gq <= LAPACK_FACTOR * dq and gr <= LAPACK_FACTOR * dr


@pytest.mark.parametrize('device_form', [1, 0])
def test_pivoted_rank_and_permutation_same_on_every_launch_form(ops, device_form):
    """The single-launch and the six-launch panel step, the rank-32 update kernel and the GEMM pair, the merged and the panel-by-panel Q
    accumulation: one rank and one leading permutation."""
    name, side = 'exit_128_tall', 1
    ref = qp.site_reference(name, side, qp.tie_rule(name, device_form))
    for fused in '01':
        for ru in '01':
            for merged in '01':
                _, _, k, perm, _ = run_site(ops, name, side, device_form, TN_PANEL_FUSED=fused, TN_QR_RANK_UPDATE=ru, TN_QR_MERGED_Q=merged)
                assert k == ref.keff and np.array_equal(perm[:k], ref.perm[:k]), (fused, ru, merged)
