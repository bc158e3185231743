"""Reference, inputs and expected ranks for the direct tests of the panel-pivoted, truncating QR of tn_site_qr (pivot_perm_host != NULL,
rank_tol > 0, 32-wide panels: qr_factor_impl, pivot_select_kernel / pivot_on_host in csrc/qr.hip), restated from the wording of
include/tnpeps.h.  numpy only, no GPU.  The Householder step, site_matrix and the bounds are those of tests/qr_exit_ref.py.

The rule.  M (m x n) is the factored matrix, k = min(m, n), panel p starts at j0 = 32 p with b = min(32, k - j0) columns.
 1. r2[j] = squared norm of rows j0.. of column j of the current (updated, permuted) matrix, j = j0 .. n-1; fro2 = their sum.
 2. p = 0: scale2 = fro2, never an exit.  p > 0: fro2 <= rank_tol^2 scale2 stops in front of the panel, keff = j0, dropped2 = fro2
    (0 <= 0: the zero matrix stops at 32).  There is no test behind the last panel; without a stop keff = k, dropped2 = 0.  The measure
    is the Frobenius one whatever frobenius_exit says.
 3. Otherwise position j0 + t receives the column with the t-th largest r2, t = 0 .. b-1; the b columns are factored without pivoting
    (diag(R) >= 0) and the trailing columns updated.
 4. Ties.  'host' (pivot_on_host: TN_PIVOT_DEVICE=0 or n > 4096): step t takes the leftmost maximum among the CURRENT positions t.. and
    swaps it to t.  'device' (pivot_select_kernel): rank by (r2 descending, position at the start of the panel ascending); the front
    columns that are not selected go, in ascending order, to the positions the selected columns from behind vacate, in ascending order.
    r2 = [5, 5, 9], b = 3: host 2, 1, 0; device 2, 0, 1.
 5. Only perm[:keff] is fixed by the rule: b = 2, r2 = [1, 2, 0, 10, 20] leaves [4, 3, 2, 1, 0] on the host and [4, 3, 2, 0, 1] on the
    device.  perm[keff:] is a set, and R's columns behind keff are compared through perm.

- select_order(r2, b, ties): order[i] = the position, before the moves of one panel, of the column that sits at position i after them.
- pivoted_reference(M, rank_tol, ties): Pivoted(keff, perm, Q (m x keff), R (keff x n, pivoted order), dropped2, log, M, col2) in
  longdouble; perm[j] = input column at position j; log holds one Panel(p, ratio, gap, floor) per panel reached:
    ratio  sqrt(fro2 / (rank_tol^2 scale2)) (None at p = 0; 0.0 where fro2 == 0),
    gap    the smallest r2[i] / r2[i+1] - 1 among the b + 1 largest residuals (nan where a zero divides; inf where there is one column),
    floor  the smallest r2 / (squared norm of that column of the input) over the selected columns (0 / 0 counts as 1);
  gap and floor are None on the panel in front of which the factorisation stops.
- INPUTS: name -> Case(build, rank_tol, k, noisy, tie_panels).  scaled(seed, m, n, r, rho, noise) is
  (G(m x r) G(r x n) / sqrt(r) + noise G(m x n)) diag(d), d = rho^-j shuffled (r = None: G(m x n) diag(d)); sign_ties: columns s (.) x_g
  with random sign vectors s, groups g of three columns at scattered positions, the groups a factor 2 apart -- squared norms that agree
  bit for bit in any arithmetic that adds x^2 up in one order.  tie_panels: the panels that are exempt from the gap condition.
- SITES: name -> Site(core, p, kc): how the factored matrix (kc None) or the core B of an attach is cut into a site tensor.  Side 0:
  A = M.reshape(Dl, p, Dr); side 1: A[l, p, r] = M[(p r), l].  With kc the factored matrix is (C (x) I_p) B / (I_p (x) C^T) B as in
  qr_exit_ref.SITES.
- Conditions on every input (tests/test_qr_pivot_host.py; conditions, not tolerances): every ratio outside [1 / MARGIN, MARGIN], every
  gap at least MIN_GAP outside tie_panels, every floor at least MIN_FLOOR.  The device's error in r2 is of the order of
  eps / sqrt(MIN_FLOOR) relative, ten orders below MIN_GAP, so k and perm[:k] are asserted exactly.
"""
import collections
import functools

import numpy as np

import qr_exit_ref as qx

LD = qx.LD
NB = qx.NB
MARGIN = qx.MARGIN
MIN_GAP = 1e-4
MIN_FLOOR = 1e-4
PIV_MAXN = 4096                                           # more columns: the host form whatever TN_PIVOT_DEVICE says

Panel = collections.namedtuple('Panel', 'p ratio gap floor')
Pivoted = collections.namedtuple('Pivoted', 'keff perm Q R dropped2 log M col2')
Case = collections.namedtuple('Case', 'build rank_tol k noisy tie_panels')
Site = collections.namedtuple('Site', 'core p kc')


# ------------------------------------------------------------------------------------------------------------------ the reference
def select_order(r2, b, ties):
    """The moves of one panel: order[i] = old position (0 .. ntr-1) of the column at position i afterwards."""
    r2 = np.asarray(r2, dtype=LD)
    ntr = r2.size
    order = np.arange(ntr)
    if ties == 'host':
        v = r2.copy()
        for t in range(b):
            a = t + int(np.argmax(v[t:]))                                # the first maximum
            v[[t, a]] = v[[a, t]]
            order[[t, a]] = order[[a, t]]
        return order
    assert ties == 'device'
    sel = sorted(range(ntr), key=lambda j: (-r2[j], j))[:b]
    vacated = sorted(j for j in sel if j >= b)
    displaced = sorted(set(range(b)) - set(sel))
    order[:b] = sel
    order[vacated] = displaced
    return order


def _gap(r2, b):
    top = np.sort(r2)[::-1][:b + 1]
    if top.size < 2:
        return float('inf')
    with np.errstate(divide='ignore', invalid='ignore'):
        return float((top[:-1] / top[1:] - 1).min())


def pivoted_reference(M, rank_tol, ties='host'):
    M = np.asarray(M, dtype=LD)
    m, n = M.shape
    k = min(m, n)
    col2 = (M * M).sum(0)
    A = M.copy()
    perm = np.arange(n)
    refl, log = [], []
    keff, dropped2, scale2 = k, LD(0), None
    for p in range(-(-k // NB)):
        j0 = p * NB
        b = min(NB, k - j0)
        T = A[j0:, j0:]
        r2 = (T * T).sum(0)
        fro2 = r2.sum()
        ratio = None
        if p == 0:
            scale2 = fro2
        else:
            thr = LD(rank_tol) * LD(rank_tol) * scale2
            ratio = 0.0 if fro2 == 0 else float(np.sqrt(fro2 / thr))
            if fro2 <= thr:
                log.append(Panel(p, ratio, None, None))
                keff, dropped2 = j0, fro2
                break
        order = select_order(r2, b, ties)
        A[:, j0:] = A[:, j0 + order]
        perm[j0:] = perm[j0 + order]
        kept, was = r2[order[:b]], col2[perm[j0:j0 + b]]
        floor = float(np.where(was > 0, kept / np.where(was > 0, was, 1), 1).min())
        log.append(Panel(p, ratio, _gap(r2, b), floor))
        refl += qx.reflect_columns(A[j0:, j0:], b)
    return Pivoted(keff, perm, qx.accumulate_q(refl[:keff], m), A[:keff].copy(), float(dropped2), log, M, col2)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _rng(*seed):
    return np.random.default_rng([20241, *seed])


def scaled(seed, m, n, r, rho, noise=0.0):
    g = _rng(seed)
    if r is None:
        B = g.standard_normal((m, n))
    else:
        B = g.standard_normal((m, r)) @ g.standard_normal((r, n)) / np.sqrt(r)
        if noise:
            B = B + noise * g.standard_normal((m, n))
    return B * g.permutation(rho ** -np.arange(n, dtype=np.float64))[None, :]


def sign_ties(seed, m, groups):
    g = _rng(seed)
    n = 3 * groups
    x = np.abs(g.standard_normal((m, groups))) * (2.0 ** -np.arange(groups))[None, :]
    cols = np.repeat(x, 3, axis=1) * g.choice([-1.0, 1.0], size=(m, n))
    return np.ascontiguousarray(cols[:, g.permutation(n)])


INPUTS = {
    'exit_64': Case(lambda: scaled(0, 300, 160, 50, 1.05, 1e-9), 1e-6, 64, True, ()),             # an exit behind two panels
    'exit_128_tall': Case(lambda: scaled(0, 1200, 200, 100, 1.03, 1e-9), 1e-6, 128, True, ()),    # m k > 256 * 512: merged-reflector Q
    'no_exit': Case(lambda: scaled(0, 300, 160, None, 1.05), 1e-4, 160, False, ()),               # one input ...
    'graded_exit': Case(lambda: scaled(0, 300, 160, None, 1.05), 3e-3, 128, False, ()),           # ... two verdicts
    'wide_exit': Case(lambda: scaled(0, 128, 200, 40, 1.03, 1e-9), 1e-6, 64, True, ()),           # m < n
    'wide_full': Case(lambda: scaled(0, 48, 100, None, 1.05), 1e-9, 48, False, ()),               # the last panel: b = 16 of 68 columns
    'one_panel': Case(lambda: scaled(0, 200, 20, None, 1.3), 1e-9, 20, False, ()),                # b = ntr = 20: a full sort
    'b1': Case(lambda: scaled(0, 100, 33, None, 1.2), 1e-9, 33, False, ()),                       # the second panel: b = ntr = 1
    'rank3': Case(lambda: scaled(0, 330, 70, 3, 1.0), 1e-6, 32, False, ()),                       # dropped2 is pure rounding
    'zero': Case(lambda: np.zeros((100, 70)), 1e-6, 32, False, (0,)),                             # 0 <= 0
    'maxn': Case(lambda: scaled(0, 40, 4096, None, 1.01), 1e-9, 40, False, ()),                   # the LDS table of the device form is full
    'over_maxn': Case(lambda: scaled(0, 40, 4097, None, 1.01), 1e-9, 40, False, ()),              # one column more: the host form
    'ties_sort': Case(lambda: sign_ties(0, 100, 8), 1e-9, 24, False, (0,)),                       # one panel, eight tied triples
    'ties_edge': Case(lambda: sign_ties(0, 100, 16), 1e-9, 48, False, (0,)),                      # a triple across the 32nd / 33rd largest
}
TIES = ('ties_sort', 'ties_edge')
ENTRYWISE = {'no_exit': 160, 'graded_exit': 128, 'exit_128_tall': 96}      # leading columns of Q / rows of R compared entrywise on the GPU

SITES = {
    'exit_64': Site('exit_64', 4, None),
    'exit_128_tall': Site('exit_128_tall', 8, None),
    'no_exit': Site('no_exit', 4, None),
    'graded_exit': Site('graded_exit', 4, None),
    'wide_exit': Site('wide_exit', 4, None),
    'wide_full': Site('wide_full', 4, None),
    'one_panel': Site('one_panel', 8, None),
    'b1': Site('b1', 4, None),
    'rank3': Site('rank3', 10, None),
    'zero': Site('zero', 4, None),
    'maxn': Site('maxn', 4, None),
    'over_maxn': Site('over_maxn', 8, None),
    'ties_sort': Site('ties_sort', 4, None),
    'ties_edge': Site('ties_edge', 4, None),
    'attach_exit_64': Site('exit_64', 4, 80),                                                     # C (80 x 75) . A (75, 4, 160): 320 x 160
}


def site_operands(name, side):
    """(A (Dl, p, Dr), C or None) of a site as contiguous float64 arrays."""
    s = SITES[name]
    B = INPUTS[s.core].build()
    rows, n = B.shape
    assert rows % s.p == 0
    inner = rows // s.p
    g = _rng(99, sorted(SITES).index(name))
    if side == 0:
        return B.reshape(inner, s.p, n).copy(), None if s.kc is None else qx.spread_matrix(g, s.kc, inner)
    return np.ascontiguousarray(B.T).reshape(n, s.p, inner), None if s.kc is None else qx.spread_matrix(g, inner, s.kc)


def tie_rule(name, device_form):
    """The tie rule of the form that runs: the device form serves at most PIV_MAXN columns."""
    return 'device' if device_form and INPUTS[SITES[name].core].build().shape[1] <= PIV_MAXN else 'host'


# ------------------------------------------------------------------------------------------------------------------ per-process store
@functools.lru_cache(maxsize=None)
def _site_reference(name, side, ties):
    s = SITES[name]
    return pivoted_reference(qx.site_matrix(side, *site_operands(name, side)), INPUTS[s.core].rank_tol, ties)


def site_reference(name, side, ties):
    """pivoted_reference of a site.  Without an attach both sides factor one matrix, and without ties the two rules give one result
    (tests/test_qr_pivot_host.py): one evaluation serves them."""
    s = SITES[name]
    return _site_reference(name, side if s.kc is not None else 0, ties if s.core in TIES else 'host')


def lapack_deviation(ref, M64, kk):
    """How far float64 numpy.linalg.qr (signs fixed) of M64[:, ref.perm] lies from the reference on the leading kk columns:
    (max |dQ|, max_j ||dR[:kk, j]|| / ||M[:, j]||)."""
    Q, R = qx.fix_signs(*np.linalg.qr(M64[:, ref.perm]))
    cn = np.sqrt(np.asarray(ref.col2[ref.perm], dtype=np.float64))
    dR = np.asarray(R[:kk] - ref.R[:kk], dtype=np.float64)
    return float(np.abs(Q[:, :kk] - ref.Q[:, :kk]).max()), float((np.sqrt((dR * dR).sum(0)) / cn).max())
