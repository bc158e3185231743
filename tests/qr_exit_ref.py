"""Reference, inputs and expected exit columns for the direct tests of the un-pivoted rank-revealing exit of tn_qr / tn_qr_batched /
tn_site_qr (reveal_check and qr_factor_impl in csrc/qr.hip), restated from the wording of include/tnpeps.h.  numpy only, no GPU.

- householder_qr_ld(M): un-pivoted Householder QR in np.longdouble with diag(R) >= 0: Q (m x k), R (k x n), k = min(m, n).  Its two
  halves, reflect_columns (some reflections, in place) and accumulate_q, also serve the panel steps of tests/qr_pivot_ref.py.
- exit_reference(M, rank_tol, frob): the exit rule on the reference's R.  With P = ceil(k / 32) panels there is no exit unless P > 2;
  the checkpoints lie behind the panels p = 1, 3, ... with p + 1 < P, i.e. at j1 = 64, 128, ...; "left" is the largest squared column
  norm of R[j1:, j1:] (frob: the sum of them), the scale the same measure over the columns of the input; the factorisation stops at the
  first j1 with left <= rank_tol^2 scale.  Returns (k_ref, [sqrt(left / (rank_tol^2 scale)) at every checkpoint reached], the squared
  Frobenius norm of R[k_ref:, k_ref:] -- 0.0 where no exit is taken).  A ratio is 0.0 where left == 0 (the zero matrix: 0 <= 0 exits).
- site_matrix(side, A, C): the matrix tn_site_qr factors, in longdouble.  Side 0: (C . A).reshape(kc p, Dr); side 1: the transposed
  (p kc) x Dl view of A . C; C = None: A itself.
- INPUTS: name -> Case, the matrices of the tn_qr tests (fixed seeds: every call of a builder returns the same bits), with rank_tol and
  the exit column under the column-norm rule (k) and under the Frobenius rule (k_frob).  "Low rank r" is
  G(m x r) G(r x n) / sqrt(r) + 1e-9 G(m x n): the dropped block sits far above rounding and far below the threshold.
- SITES: name -> Site, operands of tn_site_qr.  A site holds a core matrix B ((inner p) x n) as its tensor; with an attach the factored
  matrix is (C (x) I_p) B on side 0 and (I_p (x) C^T) B on side 1, so low rank and column scaling of B carry over; C has singular
  values between 0.8 and 1.25.  site_operands(name, side) gives (A, C) as float64 arrays.
- MARGIN: every checkpoint ratio of every input and site lies outside [1 / MARGIN, MARGIN] (tests/test_qr_exit_host.py), so that a
  disagreement about the exit column can never be a rounding tie.
reference(name) / site_reference(name, side) keep M (longdouble) and its R per process; q_reference(name) adds Q.
- check_factors(ref, Q, R, keff, ...): what a (possibly truncated) factorisation from the GPU owes the reference, with the bounds of
  tests/test_gpu_qr_exit.py and tests/test_gpu_qr_pivot.py.
"""
import collections
import functools

import numpy as np

LD = np.longdouble
MARGIN = 1.5
NB = 32

Case = collections.namedtuple('Case', 'build rank_tol k k_frob noisy')
Site = collections.namedtuple('Site', 'core p inner kc rank_tol k k_frob noisy')


# ------------------------------------------------------------------------------------------------------------------ the reference
def reflect_columns(A, steps):
    """The first `steps` Householder reflections of the un-pivoted QR, applied in place to the longdouble array A: rows 0 .. steps-1 then
    hold those rows of R (zeros below the diagonal in the first `steps` columns), A[steps:, steps:] the updated trailing block.  Returns
    the reflectors [(v, beta) or None], H_j = I - beta v v^T acting on rows j.. ."""
    m, n = A.shape
    refl = []
    for j in range(steps):
        x = A[j:, j]
        x0 = x[0]
        sigma = x[1:] @ x[1:]
        alpha = np.sqrt(x0 * x0 + sigma)
        v = x.copy()
        v[0] = x0 - alpha if x0 <= 0 else -sigma / (x0 + alpha)          # x - alpha e_1 without cancellation
        vv = v @ v
        if vv == 0:                                                      # the column is alpha e_1 already (alpha >= 0): H = I
            refl.append(None)
            continue
        beta = LD(2) / vv
        if j + 1 < n:
            A[j:, j + 1:] -= np.outer(beta * v, v @ A[j:, j + 1:])
        A[j, j] = alpha
        A[j + 1:, j] = 0
        refl.append((v, beta))
    return refl


def accumulate_q(refl, m):
    """The first len(refl) columns of H_0 H_1 ... H_{len(refl)-1} (m rows), reflector j acting on rows j.. ."""
    k = len(refl)
    Q = np.zeros((m, k), dtype=LD)
    Q[np.arange(k), np.arange(k)] = 1
    for i in range(k - 1, -1, -1):
        if refl[i] is not None:
            v, beta = refl[i]
            Q[i:, i:] -= np.outer(beta * v, v @ Q[i:, i:])
    return Q


def householder_qr_ld(M, want_q=True):
    """(Q, R) of the un-pivoted Householder QR of M in longdouble, diag(R) >= 0; Q is None with want_q=False."""
    A = np.array(M, dtype=LD)
    m, n = A.shape
    k = min(m, n)
    refl = reflect_columns(A, k)
    R = np.triu(A[:k])
    return (accumulate_q(refl, m) if want_q else None), R


def _measure(c2, frob):
    c2 = np.asarray(c2, dtype=LD)
    return c2.sum() if frob else (c2.max() if c2.size else LD(0))


def exit_reference(M, rank_tol, frob, R=None):
    """(k_ref, ratios, trailing2) of the exit rule; R: the reference's triangular factor of M when the caller has it already."""
    M = np.asarray(M, dtype=LD)
    m, n = M.shape
    k = min(m, n)
    P = -(-k // NB)
    if P <= 2:
        return k, [], 0.0
    if R is None:
        R = householder_qr_ld(M, want_q=False)[1]
    scale = _measure((M * M).sum(0), frob)
    thr = LD(rank_tol) * LD(rank_tol) * scale
    ratios = []
    for p in range(1, P, 2):
        if not p + 1 < P:
            break
        j1 = (p + 1) * NB
        T = R[j1:, j1:]
        left = _measure((T * T).sum(0), frob)
        ratios.append(0.0 if left == 0 else float(np.sqrt(left / thr)))
        if left <= thr:
            return j1, ratios, float((T * T).sum())
    return k, ratios, 0.0


def site_matrix(side, A, C=None):
    """The matrix tn_site_qr factors for the site tensor A (Dl, p, Dr) and the centre matrix C, in longdouble."""
    A = np.asarray(A, dtype=LD)
    Dl, p, Dr = A.shape
    if side == 0:
        T = A if C is None else np.tensordot(np.asarray(C, dtype=LD), A, axes=(1, 0))          # (kc, p, Dr)
        return T.reshape(-1, Dr)
    T = A if C is None else np.tensordot(A, np.asarray(C, dtype=LD), axes=(2, 0))              # (Dl, p, kc)
    return T.reshape(Dl, -1).T


def fix_signs(Q, R):
    """(Q, R) with diag(R) >= 0 (numpy.linalg.qr leaves the signs to LAPACK)."""
    s = np.where(np.diag(R) < 0, -1.0, 1.0)
    return Q * s[None, :], R * s[:, None]


# ------------------------------------------------------------------------------------------------------------------ inputs
def _rng(*seed):
    return np.random.default_rng([20240, *seed])


def gauss(seed, m, n):
    return _rng(seed).standard_normal((m, n))


def low_rank(seed, m, n, r):
    g = _rng(seed)
    return g.standard_normal((m, r)) @ g.standard_normal((r, n)) / np.sqrt(r) + 1e-9 * g.standard_normal((m, n))


def graded(seed, m, n):
    return gauss(seed, m, n) * (10.0 ** (-np.arange(n) / 16.0))[None, :]


SPLIT_TOL = 1e-8


def rule_split(seed, m, n):
    """Column 0 at scale 1, columns 1..63 at 0.01, 64..127 at 0.5 tol, the rest at 1e-3 tol: the largest column left behind column 64
    is below tol times the largest column, the Frobenius norm of what is left is above tol times the Frobenius norm."""
    s = np.full(n, 1e-3 * SPLIT_TOL)
    s[0], s[1:64], s[64:128] = 1.0, 0.01, 0.5 * SPLIT_TOL
    return gauss(seed, m, n) / np.sqrt(m) * s[None, :]


INPUTS = {
    'three_panels': Case(lambda: low_rank(1, 200, 96, 40), 1e-6, 64, 64, True),              # P = 3: the only checkpoint
    'merged_q': Case(lambda: low_rank(2, 2100, 200, 70), 1e-6, 128, 128, True),              # m k > 256 * 512: merged-reflector Q after an exit
    'wide': Case(lambda: low_rank(3, 150, 400, 70), 1e-6, 128, 128, True),                   # m < n, 22 rows left below the exit
    'no_exit': Case(lambda: low_rank(4, 300, 160, 140), 1e-6, 160, 160, True),               # the rank lies behind the last checkpoint
    'rank64': Case(lambda: low_rank(5, 333, 150, 64), 1e-6, 64, 64, True),                   # the rank on a checkpoint ...
    'rank65': Case(lambda: low_rank(6, 333, 150, 65), 1e-6, 128, 128, True),                 # ... and one behind it
    'graded': Case(lambda: graded(7, 400, 160), 1e-6, 128, 128, False),
    'rule_split': Case(lambda: rule_split(8, 400, 160), SPLIT_TOL, 64, 128, False),
    'two_panels_300x64': Case(lambda: low_rank(9, 300, 64, 20), 1e-6, 64, 64, True),         # P <= 2: no exit exists
    'two_panels_100x60': Case(lambda: low_rank(10, 100, 60, 20), 1e-6, 60, 60, True),
    'zero': Case(lambda: np.zeros((200, 96)), 1e-6, 64, 64, False),                          # scale 0, 0 <= 0
    'batch_rank40': Case(lambda: low_rank(11, 300, 160, 40), 1e-6, 64, 64, True),            # the items of the tn_qr_batched test ...
    'batch_rank100': Case(lambda: low_rank(12, 300, 160, 100), 1e-6, 128, 128, True),
    'batch_zero': Case(lambda: np.zeros((300, 160)), 1e-6, 64, 64, False),                   # ... with 'no_exit'
}
FULL_RANK = ('graded', 'rule_split')                      # compared with LAPACK column by column
WELL_CONDITIONED = ('graded', 'no_exit')                  # factors compared entrywise on the GPU
BATCH = ('batch_rank40', 'batch_rank100', 'no_exit', 'batch_zero')
BATCH_KEFF = [64, 128, 160, 64]

SITES = {
    # core (a name of INPUTS: no attach, or a builder of the (inner p) x n matrix), p, inner, kc
    'three_panels_plain': Site('three_panels', 8, 25, None, 1e-6, 64, 64, True),                         # (25, 8, 96)
    'three_panels_attach': Site(lambda: low_rank(21, 19 * 8, 96, 40), 8, 19, 25, 1e-6, 64, 64, True),    # C (25 x 19) . A (19, 8, 96)
    'rank64_attach': Site(lambda: low_rank(22, 40 * 9, 150, 64), 9, 40, 37, 1e-6, 64, 64, True),         # 333 x 150
    'rank65_attach': Site(lambda: low_rank(23, 40 * 9, 150, 65), 9, 40, 37, 1e-6, 128, 128, True),
    'rule_split_attach': Site(lambda: rule_split(24, 45 * 8, 160), 8, 45, 50, SPLIT_TOL, 64, 128, False),    # 400 x 160
    'tiny_attach': Site(lambda: gauss(25, 5 * 4, 20), 4, 5, 3, 1e-6, 12, 12, False),                     # (3, 4, 20): one workgroup
    'one_launch_attach': Site(lambda: gauss(26, 33 * 8, 60), 8, 33, 40, 1e-6, 60, 60, False),            # (40, 8, 60): one launch
    'blocked_attach': Site(lambda: gauss(27, 23 * 8, 130), 8, 23, 20, 1e-6, 130, 130, False),            # (20, 8, 130): blocked
}


def _orth(g, m, n):
    return np.linalg.qr(g.standard_normal((m, n)))[0]


def spread_matrix(g, rows, cols):
    """A random rows x cols matrix from the generator g with singular values spread evenly over [0.8, 1.25]."""
    r = min(rows, cols)
    return (_orth(g, rows, r) * np.linspace(0.8, 1.25, r)[None, :]) @ _orth(g, cols, r).T


def centre_matrix(name, rows, cols):
    """The centre matrix of a site of SITES (see spread_matrix)."""
    return spread_matrix(_rng(99, sorted(SITES).index(name)), rows, cols)


def site_operands(name, side):
    """(A (Dl, p, Dr), C or None) of a site as contiguous float64 arrays.  Side 0 factors (C (x) I_p) B, side 1 (I_p (x) C^T) B."""
    s = SITES[name]
    B = INPUTS[s.core].build() if isinstance(s.core, str) else s.core()
    n = B.shape[1]
    assert B.shape[0] == s.inner * s.p
    if side == 0:
        A = B.reshape(s.inner, s.p, n).copy()                            # B's rows are (l, p)
        C = None if s.kc is None else centre_matrix(name, s.kc, s.inner)
    else:
        A = np.ascontiguousarray(B.T).reshape(n, s.p, s.inner)           # B's rows are (p, r):  A[l, p, r] = B[(p, r), l]
        C = None if s.kc is None else centre_matrix(name, s.inner, s.kc)
    return A, C


# ------------------------------------------------------------------------------------------------------------------ per-process store
Ref = collections.namedtuple('Ref', 'M R col2')           # M, R in longdouble; col2: squared column norms of M


def _ref(M):
    M = np.asarray(M, dtype=LD)
    return Ref(M, householder_qr_ld(M, want_q=False)[1], (M * M).sum(0))


@functools.lru_cache(maxsize=None)
def reference(name):
    return _ref(INPUTS[name].build())


@functools.lru_cache(maxsize=None)
def site_reference(name, side):
    return _ref(site_matrix(side, *site_operands(name, side)))


@functools.lru_cache(maxsize=None)
def q_reference(name):
    """(Q, R) of householder_qr_ld for an input."""
    return householder_qr_ld(INPUTS[name].build())


def lapack_deviation(name, keff):
    """How far float64 numpy.linalg.qr (signs fixed) lies from the longdouble reference on the leading keff columns of an input:
    (max |dQ|, max_j ||dR[:keff, j]|| / ||M[:, j]||)."""
    M = INPUTS[name].build()
    Q, R = fix_signs(*np.linalg.qr(M))
    Ql, Rl = q_reference(name)
    cn = np.sqrt(np.asarray(reference(name).col2, dtype=np.float64))
    dR = np.asarray(R[:keff] - Rl[:keff], dtype=np.float64)
    return float(np.abs(Q[:, :keff] - Ql[:, :keff]).max()), float((np.sqrt((dR * dR).sum(0)) / cn).max())


# ------------------------------------------------------------------------------------------------------------------ what a factorisation owes its reference
TOL = 5e-14


def check_factors(ref, Q, R, keff, rank_tol, frob, trailing2, noisy, label):
    """Everything a (possibly truncated) factorisation M ~ Q R owes the reference `ref` of M; returns ||M - Q R||_F (longdouble)."""
    m, n = ref.M.shape
    full = min(m, n)
    print(label, 'keff', keff)
    assert Q.shape == (m, keff) and R.shape == (keff, n), label
    assert np.isfinite(Q).all() and np.isfinite(R).all(), label
    orth = np.abs(Q.T @ Q - np.eye(keff)).max()
    print(label, 'orthogonality', orth)
    assert orth < TOL, label
    assert np.abs(np.tril(R[:, :keff], -1)).max() == 0.0 and (np.diag(R) >= 0).all(), label
    E = ref.M - Q.astype(LD) @ R.astype(LD)
    res = np.sqrt((E * E).sum(0))
    cn = np.sqrt(ref.col2)
    scale = np.sqrt(ref.col2.sum()) if frob else cn.max()
    bound = TOL * cn + (LD(rank_tol) * scale * (1 + LD(1e-6)) if keff < full else 0)
    print(label, 'largest residual / bound', float((res / np.where(bound > 0, bound, 1)).max()))
    assert (res <= bound).all(), label
    fro2 = float((E * E).sum())
    if keff < full and noisy:
        print(label, 'dropped block: ||M - Q R||_F^2 / reference - 1', fro2 / trailing2 - 1)
        assert abs(fro2 - trailing2) <= 1e-5 * trailing2, label
    return float(np.sqrt(LD(fro2)))
