"""CPU checks of what the GPU tests of the panel-pivoted QR of tn_site_qr stand on (tests/qr_pivot_ref.py): the two tie rules on the hand
examples, the conditions that make the rank and the leading permutation exact (every exit ratio outside [1 / MARGIN, MARGIN], every gap
among the b + 1 largest residuals at least MIN_GAP, every selected column keeps MIN_FLOOR of its input norm), the rank the table states,
the reference's own factorisation in longdouble, the two rules against each other, and the reference against LAPACK."""
import numpy as np
import pytest

import qr_exit_ref as qx
import qr_pivot_ref as qp

LD = np.longdouble
TIGHT = max(100 * float(np.finfo(LD).eps), 1e-17)        # as tests/test_qr_exit_host.py holds householder_qr_ld
CASES = [(name, side) for name in qp.SITES for side in ((0, 1) if qp.SITES[name].kc is not None else (0,))]


def _rules(name):
    return ('host', 'device') if qp.SITES[name].core in qp.TIES else ('host',)


def test_tie_rules_on_the_hand_examples():
    assert qp.select_order([5, 5, 9], 3, 'host').tolist() == [2, 1, 0]           # 9, the second 5, the first 5
    assert qp.select_order([5, 5, 9], 3, 'device').tolist() == [2, 0, 1]
    assert qp.select_order([1, 2, 0, 10, 20], 2, 'host').tolist() == [4, 3, 2, 1, 0]
    assert qp.select_order([1, 2, 0, 10, 20], 2, 'device').tolist() == [4, 3, 2, 0, 1]
    for rule in ('host', 'device'):
        assert qp.select_order([0, 0, 0, 0], 2, rule).tolist() == [0, 1, 2, 3]   # the zero matrix: nothing moves
        assert qp.select_order([3, 7, 1, 5], 4, rule).tolist() == [1, 3, 0, 2]   # b = ntr: a full sort
        assert qp.select_order([4], 1, rule).tolist() == [0]
    # a whole factorisation: 3 x 3 diagonal, one panel
    r = qp.pivoted_reference(np.diag([1.0, -3.0, 2.0]), 1e-3)
    assert r.keff == 3 and r.perm.tolist() == [1, 2, 0] and r.dropped2 == 0.0 and float(np.abs(r.R - np.diag([3.0, 2.0, 1.0])).max()) < TIGHT
    assert r.log == [qp.Panel(0, None, pytest.approx(1.25), 1.0)]


def test_exit_rule_on_a_hand_made_matrix():
    """Diagonal, 96 columns: 40 at 1, 24 at 1e-3, 32 at 1e-7 (shuffled).  What is left in front of panel 1 is 8 + 24e-6 + 32e-14, in
    front of panel 2 it is 32e-14: the ratios can be read off, the exit is Frobenius, and there is no test behind the last panel."""
    d = np.concatenate([np.ones(40), np.full(24, 1e-3), np.full(32, 1e-7)])
    sh = np.random.default_rng(5).permutation(96)
    M = np.diag(d[sh])
    r = qp.pivoted_reference(M, 1e-6)
    assert r.keff == 64 and r.dropped2 == pytest.approx(32e-14)
    assert [l.ratio for l in r.log] == [None, pytest.approx(np.sqrt(8.000024 / 40.000024) * 1e6, rel=1e-6), pytest.approx(np.sqrt(32e-14 / 40.000024) * 1e6, rel=1e-6)]
    assert sorted(r.perm[:40].tolist()) == sorted(np.flatnonzero(d[sh] == 1.0).tolist())
    assert sorted(r.perm[64:].tolist()) == sorted(np.flatnonzero(d[sh] == 1e-7).tolist())
    assert qp.pivoted_reference(M, 1e-9).keff == 96 and qp.pivoted_reference(M, 1e-9).dropped2 == 0.0
    assert qp.pivoted_reference(M, 0.5).keff == 32                                # sqrt(8 / 40) = 0.45 <= 0.5
    assert qp.pivoted_reference(M, 0.4).keff == 64
    assert qp.pivoted_reference(np.diag(d[:32] * 1e-30), 0.5).keff == 32          # one panel: no test exists
    assert [l.ratio for l in qp.pivoted_reference(np.zeros((70, 65)), 1e-6).log] == [None, 0.0]


@pytest.mark.parametrize('name,side', CASES)
def test_conditions_and_rank_of_every_site(name, side):
    s = qp.SITES[name]
    c = qp.INPUTS[s.core]
    A, C = qp.site_operands(name, side)
    assert A.flags.c_contiguous and A.dtype == np.float64 and (C is None or C.flags.c_contiguous)
    for rule in _rules(name):
        r = qp.site_reference(name, side, rule)
        m, n = r.M.shape
        assert m == s.p * (A.shape[0] if side == 0 else A.shape[2]) if C is None else m == s.p * s.kc
        assert n == (A.shape[2] if side == 0 else A.shape[0])
        assert r.keff == c.k, (name, side, rule)
        for l in r.log:
            print(name, side, rule, l)
            assert l.ratio is None or not 1.0 / qp.MARGIN <= l.ratio <= qp.MARGIN, (name, side, rule, l)
            if l.gap is not None and l.p not in c.tie_panels:
                assert l.gap >= qp.MIN_GAP, (name, side, rule, l)
            assert l.floor is None or l.floor >= qp.MIN_FLOOR, (name, side, rule, l)


def test_both_sides_of_a_plain_site_factor_the_input_itself():
    for name in ('wide_full', 'b1'):
        M = qp.INPUTS[name].build()
        for side in (0, 1):
            assert np.array_equal(np.asarray(qx.site_matrix(side, *qp.site_operands(name, side)), dtype=np.float64), M)
    s = qp.SITES['attach_exit_64']
    B = qp.INPUTS[s.core].build()
    A, C = qp.site_operands('attach_exit_64', 0)
    assert np.abs(np.asarray(qx.site_matrix(0, A, C), dtype=np.float64) - np.kron(C, np.eye(s.p)) @ B).max() < 1e-13
    A, C = qp.site_operands('attach_exit_64', 1)
    assert np.abs(np.asarray(qx.site_matrix(1, A, C), dtype=np.float64) - np.kron(np.eye(s.p), C.T) @ B).max() < 1e-13
    sv = np.linalg.svd(C, compute_uv=False)
    assert 0.8 - 1e-12 <= sv.min() and sv.max() <= 1.25 + 1e-12


@pytest.mark.parametrize('name,side', CASES)
def test_reference_factors_the_permuted_input(name, side):
    """In longdouble: M[:, perm] = Q R on the accepted columns, the columns behind them within rank_tol ||M||_F (what the exit test
    has verified about them, all together), and what is left is dropped2."""
    c = qp.INPUTS[qp.SITES[name].core]
    for rule in _rules(name):
        r = qp.site_reference(name, side, rule)
        m, n = r.M.shape
        k = r.keff
        assert r.Q.dtype == r.R.dtype == LD and r.Q.shape == (m, k) and r.R.shape == (k, n)
        assert sorted(r.perm.tolist()) == list(range(n))
        assert (np.diag(r.R) >= 0).all() and (k < 2 or np.abs(np.tril(r.R[:, :k], -1)).max() == 0)
        assert float(np.abs(r.Q.T @ r.Q - np.eye(k)).max()) < TIGHT
        E = r.M[:, r.perm] - r.Q @ r.R
        res = np.sqrt((E * E).sum(0))
        cn = np.sqrt(r.col2[r.perm])
        fro = np.sqrt(r.col2.sum())
        assert (res[:k] <= TIGHT * cn[:k]).all()
        assert (res[k:] <= TIGHT * cn[k:] + LD(c.rank_tol) * fro).all()
        assert abs(float(np.sqrt((E * E).sum())) - np.sqrt(r.dropped2)) <= TIGHT * float(fro)
        if k == min(m, n):
            assert r.dropped2 == 0.0
        if not r.col2.any():                                             # the zero matrix
            assert r.perm.tolist() == list(range(n)) and not r.R.any() and r.dropped2 == 0.0


@pytest.mark.parametrize('name', list(qp.INPUTS))
def test_the_two_tie_rules_against_each_other(name):
    """Without ties: one rank, one leading permutation, the same factors (R's columns behind the rank through perm).  With ties the
    leading permutations differ -- the GPU test would notice a form that follows the other form's rule."""
    c = qp.INPUTS[name]
    M = c.build()
    h, d = qp.pivoted_reference(M, c.rank_tol, 'host'), qp.pivoted_reference(M, c.rank_tol, 'device')
    k = h.keff
    assert d.keff == k and sorted(h.perm[k:].tolist()) == sorted(d.perm[k:].tolist())
    if name in qp.TIES:
        assert not np.array_equal(h.perm[:k], d.perm[:k])
        return
    assert np.array_equal(h.perm[:k], d.perm[:k])
    assert h.dropped2 == pytest.approx(d.dropped2, rel=1e-15)
    n = M.shape[1]
    Rh, Rd = np.zeros((k, n), dtype=LD), np.zeros((k, n), dtype=LD)
    Rh[:, h.perm], Rd[:, d.perm] = h.R, d.R
    assert float(np.abs(h.Q - d.Q).max()) <= TIGHT
    assert (np.sqrt(((Rh - Rd) ** 2).sum(0)) <= TIGHT * np.sqrt(h.col2)).all()


def test_ties_are_exact_and_where_the_names_say():
    """Sign-flipped columns have squared norms that agree bit for bit; in 'ties_sort' every column of the one panel is in a tied triple,
    in 'ties_edge' the 32nd and the 33rd largest of panel 0 are equal."""
    for name, groups in (('ties_sort', 8), ('ties_edge', 16)):
        M = qp.INPUTS[name].build()
        for r2 in ((M * M).sum(0), (M.astype(LD) ** 2).sum(0)):
            top = np.sort(r2)[::-1]
            assert np.array_equal(top[0::3], top[1::3]) and np.array_equal(top[0::3], top[2::3])
            assert (top[0:-3:3] > 2 * top[3::3]).all() and top.size == 3 * groups       # (a factor 4, times the ratio of two chi^2_100 / 100)
    top = np.sort((qp.INPUTS['ties_edge'].build() ** 2).sum(0))[::-1]
    assert top[31] == top[32] and top[29] > top[30]


@pytest.mark.parametrize('name', list(qp.ENTRYWISE))
def test_reference_against_lapack(name):
    """numpy.linalg.qr of the float64 input in the reference's column order, signs fixed, on the leading columns that are well
    conditioned (all 160, the accepted 128, and 96 of a rank of 100): Householder QR is backward stable column by column, so R[:, j] lies
    within c eps cond ||M[:, j]|| of the true one and Q within c eps cond; 1e-12 leaves c cond = 4500."""
    kk = qp.ENTRYWISE[name]
    r = qp.site_reference(name, 0, 'host')
    dq, dr = qp.lapack_deviation(r, qp.INPUTS[name].build(), kk)
    print(name, 'LAPACK against the reference: Q', dq, 'R', dr)
    assert dq < 1e-12 and dr < 1e-12
