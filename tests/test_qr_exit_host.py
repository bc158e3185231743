"""CPU checks of what the GPU tests of the rank-revealing exit of tn_qr / tn_site_qr stand on (tests/qr_exit_ref.py): the longdouble
Householder reference agrees with LAPACK, every checkpoint ratio of every input and site keeps the margin, and the rule gives the
exit column the table states, under the column-norm rule and under the Frobenius rule."""
import numpy as np
import pytest

import qr_exit_ref as qx


def _ratios(ref, rank_tol):
    out = []
    for frob in (False, True):
        out += qx.exit_reference(ref.M, rank_tol, frob, R=ref.R)[1]
    return out


@pytest.mark.parametrize('name', qx.FULL_RANK)
def test_reference_against_lapack(name):
    """Both inputs are a Gaussian matrix (400 x 160, condition number about 4.5) with scaled columns.  Householder QR is backward stable
    column by column, so LAPACK's R[:, j] lies within c eps cond ||M[:, j]|| of the true one and its Q within c eps cond: 1e-12 leaves
    c = 1000.  The reference itself is held to 100 eps of longdouble (at least 1e-17: eps is 1.1e-19 where longdouble has 64 bits of
    mantissa) in orthogonality and column-relative residual."""
    M = qx.INPUTS[name].build()
    Ql, Rl = qx.q_reference(name)
    Q, R = qx.fix_signs(*np.linalg.qr(M))
    k = min(M.shape)
    assert Ql.dtype == Rl.dtype == np.longdouble and Ql.shape == (M.shape[0], k) and Rl.shape == (k, M.shape[1])
    assert (np.diag(Rl) >= 0).all() and np.abs(np.tril(Rl, -1)).max() == 0
    cn = np.sqrt(np.asarray(qx.reference(name).col2))
    tight = max(100 * float(np.finfo(np.longdouble).eps), 1e-17)
    assert float(np.abs(Ql.T @ Ql - np.eye(k)).max()) < tight
    assert float((np.sqrt(((Ql @ Rl - M) ** 2).sum(0)) / cn).max()) < tight
    dR = np.asarray(R - Rl, dtype=np.float64)
    assert float((np.sqrt((dR * dR).sum(0)) / cn).max()) < 1e-12
    assert float(np.abs(Q - Ql).max()) < 1e-12


def test_reference_handles_wide_zero_and_trivial_columns():
    """m < n, a zero matrix, a column that is a non-negative multiple of e_1 already (no reflection) and a 1 x 1 matrix."""
    M = qx.gauss(31, 7, 12)
    Q, R = qx.householder_qr_ld(M)
    assert Q.shape == (7, 7) and R.shape == (7, 12) and (np.diag(R) >= 0).all()
    assert float(np.abs(Q @ R - M).max()) < 1e-17 and float(np.abs(Q.T @ Q - np.eye(7)).max()) < 1e-17
    Q, R = qx.householder_qr_ld(np.zeros((5, 3)))
    assert np.array_equal(Q, np.eye(5, 3)) and not R.any()
    M = np.triu(qx.gauss(32, 4, 4))
    M[np.arange(4), np.arange(4)] = np.abs(np.diag(M))
    Q, R = qx.householder_qr_ld(M)
    assert np.array_equal(Q, np.eye(4)) and np.array_equal(R, M)
    Q, R = qx.householder_qr_ld(np.array([[-3.0]]))
    assert abs(float(Q[0, 0]) + 1) < 1e-17 and R[0, 0] == 3


def test_exit_rule_on_hand_made_matrices():
    """The rule itself, on diagonal matrices whose trailing norms can be read off: checkpoints at 64 and 128 only while another panel
    follows, the first one that passes is taken, both measures."""
    d = np.ones(160)
    d[64:] = 1e-3
    d[128:] = 1e-9
    M = np.diag(d)
    assert qx.exit_reference(M, 1e-6, False)[0] == 128
    k, ratios, tr2 = qx.exit_reference(M, 1e-2, False)
    assert k == 64 and ratios == [pytest.approx(0.1)] and tr2 == pytest.approx(64e-6 + 32e-18)
    k, ratios, _ = qx.exit_reference(M, 1e-2, True)                    # sqrt(64e-6 / 64) / 1e-2 = 0.1 again (scale: 64 + 64e-6)
    assert k == 64 and ratios == [pytest.approx(0.1, rel=1e-5)]
    k, ratios, tr2 = qx.exit_reference(M, 1e-12, False)
    assert k == 160 and len(ratios) == 2 and tr2 == 0.0
    assert qx.exit_reference(np.diag(d[:128]), 1e-2, False)[0] == 64   # P = 4: checkpoint at 64 only
    assert qx.exit_reference(np.diag(d[:96]), 1e-2, False)[0] == 64    # P = 3
    assert qx.exit_reference(np.diag(d[:64]), 0.5, False) == (64, [], 0.0)     # P = 2: no exit exists
    assert qx.exit_reference(np.eye(129)[:, :128] * 1e-30, 0.5, False)[0] == 128   # nothing is small against itself
    assert qx.exit_reference(np.zeros((70, 65)), 1e-6, False) == (64, [0.0], 0.0)


@pytest.mark.parametrize('name', list(qx.INPUTS))
def test_margin_and_exit_column_of_every_input(name):
    c = qx.INPUTS[name]
    ref = qx.reference(name)
    for r in _ratios(ref, c.rank_tol):
        assert not 1.0 / qx.MARGIN <= r <= qx.MARGIN, (name, r)
    assert qx.exit_reference(ref.M, c.rank_tol, False, R=ref.R)[0] == c.k
    assert qx.exit_reference(ref.M, c.rank_tol, True, R=ref.R)[0] == c.k_frob


@pytest.mark.parametrize('side', [0, 1])
@pytest.mark.parametrize('name', list(qx.SITES))
def test_margin_and_exit_column_of_every_site(name, side):
    s = qx.SITES[name]
    A, C = qx.site_operands(name, side)
    ref = qx.site_reference(name, side)
    m = s.p * (s.inner if s.kc is None else s.kc)
    assert ref.M.shape == (m, A.shape[2] if side == 0 else A.shape[0])
    assert A.flags.c_contiguous and (C is None or C.flags.c_contiguous) and A.dtype == np.float64
    for r in _ratios(ref, s.rank_tol):
        assert not 1.0 / qx.MARGIN <= r <= qx.MARGIN, (name, side, r)
    assert qx.exit_reference(ref.M, s.rank_tol, False, R=ref.R)[0] == s.k
    assert qx.exit_reference(ref.M, s.rank_tol, True, R=ref.R)[0] == s.k_frob


def test_site_matrix_layouts():
    """site_matrix against an index-by-index evaluation of the two attach products and the two views."""
    g = np.random.default_rng(3)
    A = g.standard_normal((3, 2, 4))
    M0, M1 = qx.site_matrix(0, A), qx.site_matrix(1, A)
    C0, C1 = g.standard_normal((5, 3)), g.standard_normal((4, 5))
    N0, N1 = qx.site_matrix(0, A, C0), qx.site_matrix(1, A, C1)
    assert M0.shape == (6, 4) and M1.shape == (8, 3) and N0.shape == (10, 4) and N1.shape == (10, 3)
    for l in range(3):
        for p in range(2):
            for r in range(4):
                assert M0[l * 2 + p, r] == A[l, p, r] and M1[p * 4 + r, l] == A[l, p, r]
    for c in range(5):
        for p in range(2):
            for r in range(4):
                assert float(N0[c * 2 + p, r]) == pytest.approx(sum(C0[c, l] * A[l, p, r] for l in range(3)), abs=1e-14)
            for l in range(3):
                assert float(N1[p * 5 + c, l]) == pytest.approx(sum(A[l, p, r] * C1[r, c] for r in range(4)), abs=1e-14)


def test_site_operands_reproduce_the_plain_input_and_the_kronecker_form():
    """Without an attach both sides factor the 'three panels' matrix itself; with one, side 0 factors (C (x) I_p) B and side 1
    (I_p (x) C^T) B of the same core B."""
    M = qx.INPUTS['three_panels'].build()
    for side in (0, 1):
        assert np.array_equal(np.asarray(qx.site_reference('three_panels_plain', side).M, dtype=np.float64), M)
    s = qx.SITES['tiny_attach']
    B = s.core()
    A, C = qx.site_operands('tiny_attach', 0)
    assert np.abs(np.asarray(qx.site_matrix(0, A, C), dtype=np.float64) - np.kron(C, np.eye(s.p)) @ B).max() < 1e-14
    A, C = qx.site_operands('tiny_attach', 1)
    assert np.abs(np.asarray(qx.site_matrix(1, A, C), dtype=np.float64) - np.kron(np.eye(s.p), C.T) @ B).max() < 1e-14
    sv = np.linalg.svd(C, compute_uv=False)
    assert 0.8 - 1e-12 <= sv.min() and sv.max() <= 1.25 + 1e-12
