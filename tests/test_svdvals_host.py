"""CPU checks of tests/svdvals_ref.py: the 40-digit reference against numpy's SVD on every input kind, its exactness on the exact
inputs, the determinism of the generator, and the stored reference values against a fresh mpmath computation."""
import numpy as np
import pytest

import svdvals_ref as sv

EPS = 2.220446049250313e-16
BLAS_FREE = ('gauss_', 'row_graded', 'dup_rows', 'tiny_row', 'view', 'zero', 'diagonal', 'signed_perm', 'hadamard', 'range_base')


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_reference_agrees_with_numpy():
    """|ref - numpy| <= 4 eps max(k, n) S0: LAPACK's backward error bound p(k, n) eps ||A||_2 with a modest p, which holds for every
    singular value whatever the grading."""
    for name, A in sv.all_reference_inputs().items():
        k, n = A.shape
        ref = sv.ref_svdvals(A)
        got = np.linalg.svd(A, compute_uv=False)
        assert ref.shape == (min(k, n),) and ref.dtype == np.float64, name
        assert np.all(np.diff(ref) <= 0) and np.all(ref >= 0), name
        assert np.abs(ref - got).max() <= 4 * EPS * max(k, n) * ref[0], (name, np.abs(ref - got).max(), ref[0])


def test_reference_exact_on_exact_inputs():
    for name, (A, vals) in sv.exact_cases().items():
        k, n = A.shape
        assert vals.shape == (min(k, n),), name
        norms = np.sort(np.sqrt((A * A).sum(axis=1)))[::-1][:min(k, n)]
        assert _same_bits(norms, vals), name                     # the stated values are the row norms
        G = A @ A.T
        assert np.count_nonzero(G - np.diag(np.diag(G))) == 0, name      # rows exactly orthogonal
        pos = norms[norms > 0]
        assert pos.max() / pos.min() < 2.0 ** 40, name           # nothing is deflated (the kernel drops rows below 2^-56)
        assert _same_bits(sv.ref_svdvals(A), vals), name
    assert _same_bits(sv.mp_svdvals(sv.exact_cases()['diagonal'][0]), sv.exact_cases()['diagonal'][1])


def test_generator_deterministic_and_as_specified():
    a, b = sv.all_reference_inputs(), sv.all_reference_inputs()
    assert list(a) == list(b)
    for name in a:
        assert _same_bits(a[name], b[name]), name
        assert a[name] is not b[name]
    c = sv.cases()
    assert [c['gauss_%dx%d' % s].shape for s in sv.GAUSS_SHAPES] == list(sv.GAUSS_SHAPES)
    assert all(max(A.shape) <= 64 for A in c.values()) and all(max(A.shape) <= 64 for A, _ in sv.exact_cases().values())
    assert c['col_graded'].shape == (60, 60) and c['row_graded'].shape == (64, 64) and c['usv'].shape == (64, 48)
    assert c['rank7'].shape == (40, 33) and np.linalg.matrix_rank(c['rank7']) == 7
    d = c['dup_rows']
    assert d.shape == (20, 30) and np.array_equal(d[5], d[2]) and np.array_equal(d[17], d[2]) and np.array_equal(d[11], d[9])
    assert np.abs(c['orth3'] @ c['orth3'].T - 9.0 * np.eye(64)).max() < 1e-13
    s = np.linalg.svd(c['clusters'], compute_uv=False)
    assert abs(s[15] - 1.0) < 1e-14 and abs(s[16] - (1.0 - 1e-10)) < 1e-14
    t = c['tiny_row']
    assert np.linalg.norm(t[9]) < 2.0 ** -56 * np.linalg.norm(t[:9], axis=1).max()
    v = c['view']
    root, off, strides = sv.root_and_view(v)
    assert v.shape == (40, 30) and not v.flags['C_CONTIGUOUS'] and root.shape == (50, 90) and (off, strides) == (10, (90, 2))
    assert not c['zero'].any() and c['zero'].shape == (4, 9)
    bc = sv.boundary_cases()
    for name in ('gauss_64x64', 'usv'):
        assert bc[name + '_64'].shape[0] == 64 and bc[name + '_65'].shape[0] == 65
        assert _same_bits(bc[name + '_65'][:64], bc[name + '_64'])
    assert sv.range_base().shape == sv.RANGE_SHAPE
    assert set(sv.RANGE_EXPONENTS) >= {-500, -300, -260, 250, 300, 480, -100, 100}


def test_stored_values_cover_the_inputs():
    """Inputs made without BLAS / LAPACK have the same bits everywhere, so their stored values must be found (the others are
    recomputed when another BLAS moves a bit)."""
    for name, A in sv.all_reference_inputs().items():
        if name.startswith(BLAS_FREE):
            assert sv.stored(A) is not None, name


def test_stored_values_fresh_small():
    """The stored values of the inputs up to 33 on the longer side equal a fresh mpmath computation bit for bit."""
    n = 0
    for name, A in sv.all_reference_inputs().items():
        st = sv.stored(A)
        if st is not None and max(A.shape) <= 33:
            assert _same_bits(st, sv.mp_svdvals(A)), name
            n += 1
    assert n >= 8


@pytest.mark.slow
def test_stored_values_fresh_all():
    seen = []
    for name, A in sv.all_reference_inputs().items():
        st = sv.stored(A)
        if st is not None and not any(A.shape == B.shape and np.array_equal(A, B) for B in seen):
            seen.append(A)
            assert _same_bits(st, sv.mp_svdvals(A)), name
