"""Host references for the small helper kernels of the weighted first pass and of bond deflation (numpy / fractions, no GPU).

Each function restates the contract include/tnpeps.h gives the export of the same name:
- argsort_desc_ref: the stable descending order (NaN first, equal values -- +0.0 == -0.0 included -- by increasing index);
- weighted_sum_ref / weighted_sum_bound: the exact sum of the products and the error bound of the documented order (256 strided
  partial sums, then a binary tree over them);
- rows_norm2_ref / rows_norm2_bound: exact squared row norms and the bound of the kernel's summation depth;
- gram_weights_ref: the floored weights and max G_cc (bit-exact), and ||G / (d d^T)||_F^2 with the bound of its summation;
- gather_scale_rows_ref: both directions, with numpy's correctly rounded sqrt and division;
- bond_deflate_ref: the drop rule of csrc/site.hip (bond_deflate) on given squared norms;
- scale_phys_ref.
Bounds use gamma_D = D u / (1 - D u), u = 2^-53: a sum of N terms in which every term passes through at most D roundings is
within gamma_D sum |term| of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2).
"""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
EPS = 2.220446049250313e-16          # the eps of tn_bond_deflate's budget (DBL_EPSILON)


def gamma(d):
    """gamma_d as an exact fraction."""
    return d * U / (1 - d * U)


def _ratio(x):
    return Fraction(*float(x).as_integer_ratio())


def exact_sum(xs):
    """The exact sum of finite doubles (a Fraction)."""
    return sum((_ratio(x) for x in np.asarray(xs, dtype=np.float64).ravel()), Fraction(0))


def exact_dot(a, b):
    """(exact sum of a_i b_i, exact sum of |a_i b_i|) for finite doubles; integer arithmetic over a common power of two."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    num, den = [], []
    for x, y in zip(a.tolist(), b.tolist()):
        p, q = x.as_integer_ratio()
        r, s = y.as_integer_ratio()
        num.append(p * r)
        den.append(q * s)
    if not num:
        return Fraction(0), Fraction(0)
    D = max(den)                                          # every denominator is a power of two: D is a multiple of all
    tot = sum(n * (D // d) for n, d in zip(num, den))
    ab = sum(abs(n) * (D // d) for n, d in zip(num, den))
    return Fraction(tot, D), Fraction(ab, D)


def within(computed, exact, bound):
    """|computed - exact| <= bound, all compared exactly."""
    return abs(_ratio(computed) - exact) <= bound


# ---------------------------------------------------------------------------------------------------------- tn_argsort_desc
def argsort_desc_ref(w):
    """perm with w[perm] in descending order, NaN first, ties (+0.0 == -0.0) by increasing index."""
    w = np.asarray(w, dtype=np.float64).tolist()

    def key(i):
        x = w[i]
        return (0, 0.0) if x != x else (1, -x)
    return np.array(sorted(range(len(w)), key=key), dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------- tn_weighted_sum
def weighted_sum_ref(a, b):
    """(w = a * b as numpy computes it, exact sum of the EXACT products a_i b_i, exact sum of |a_i b_i|)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    s, t = exact_dot(a, b)
    return a * b, s, t


def weighted_sum_bound(n, abs_sum):
    """Bound of |sum_out - sum_i a_i b_i| for the documented order: thread t adds i = t, t + 256, ... (at most ceil(n/256) additions
    per product), then an 8-level binary tree over the 256 partials; one more rounding for the product itself (whether or not the
    compiler fuses it into the addition).  Measured against the exact products, so it holds for a fused and an unfused kernel."""
    d = -(-n // 256) + 8 + 1
    return gamma(d) * abs_sum


# ---------------------------------------------------------------------------------------------------------- tn_rows_norm2
def rows_norm2_ref(A):
    """Exact squared norms of the rows (Fractions)."""
    A = np.asarray(A, dtype=np.float64)
    return [exact_dot(r, r)[0] for r in A]


def rows_norm2_depth(cols):
    """Roundings a square can pass through in rows_norm2_kernel: its own (or the fused add), at most ceil(cols/256) additions in a
    thread's accumulator, s0 + s1, 6 shuffle levels inside a wave, 2 levels over the 4 waves."""
    return -(-cols // 256) + 1 + 1 + 6 + 2


def rows_norm2_bound(cols, exact):
    """All terms are non-negative: |out - exact| <= gamma_D exact."""
    return gamma(rows_norm2_depth(cols)) * exact


# ---------------------------------------------------------------------------------------------------------- tn_gram_weights
GW_PARTS = 64


def gram_weights_ref(G, floor_rel):
    """(d2, max G_cc) bit for bit: gmax = max(0, max_c G_cc), d2 = fmax(G_cc, gmax * floor_rel)."""
    G = np.asarray(G, dtype=np.float64)
    dg = np.diagonal(G).copy()
    gmax = max(0.0, float(np.fmax.reduce(dg)))
    fl = np.float64(gmax) * np.float64(floor_rel)
    return np.fmax(dg, fl), gmax


def gram_kfro_ref(G, d2):
    """||K||_F^2 = sum_ij G_ij^2 / (d2_i d2_j) for the d2 the kernel returned.  Evaluated in extended precision (x87 long double,
    64-bit significand: relative error below 40 * 2^-64 for n <= 65536, far below gram_kfro_bound) when numpy has it, exactly
    otherwise."""
    G = np.asarray(G, dtype=np.float64)
    d2 = np.asarray(d2, dtype=np.float64)
    if np.finfo(np.longdouble).nmant >= 63:
        dd = d2.astype(np.longdouble)
        tot = np.longdouble(0)
        for r0 in range(0, G.shape[0], 256):             # (blocks of rows: n = 4096 would need ~1 GB at once)
            g = G[r0:r0 + 256].astype(np.longdouble)
            tot += np.sum((g * g) / dd[r0:r0 + 256, None] / dd[None, :])
        return float(tot)
    n = G.shape[0]
    tot = Fraction(0)
    for i in range(n):
        for j in range(n):
            tot += _ratio(G[i, j]) ** 2 / (_ratio(d2[i]) * _ratio(d2[j]))
    return float(tot)


def gram_kfro_bound(n, kfro):
    """Bound of |sum_in_order(stats[0:64]) - ||K||_F^2|: a term G_ij^2 / (d2_i d2_j) is formed with 4 roundings (the square, 1/d2_i,
    the product, the division), is added into a thread's accumulator (at most ceil(n/64) rows x ceil(n/256) columns), passes an
    8-level tree and then the 63 in-order additions of the partials.  Terms are non-negative, so the bound is relative; the extra
    2^-50 relative covers the reference's own rounding and n^2 2^-1074 the terms that underflow."""
    rows_per = -(-n // GW_PARTS)
    d = 4 + rows_per * -(-n // 256) + 8 + (GW_PARTS - 1)
    return float(gamma(d) + Fraction(1, 2 ** 50)) * kfro + n * n * 2.0 ** -1074


# ---------------------------------------------------------------------------------------------------------- tn_gather_scale_rows
def gather_scale_rows_ref(A, perm, w2, inverse=False):
    """inverse=False: out[j] = sqrt(w2[perm[j]]) A[perm[j]];  inverse=True: out[perm[j]] = A[j] * (1 / sqrt(w2[perm[j]]))."""
    A = np.asarray(A, dtype=np.float64)
    perm = np.asarray(perm, dtype=np.int64)
    w2 = np.asarray(w2, dtype=np.float64)
    if not inverse:
        return np.sqrt(w2[perm])[:, None] * A[perm]
    out = np.empty_like(A)
    out[perm] = A * (1.0 / np.sqrt(w2[perm]))[:, None]
    return out


# ---------------------------------------------------------------------------------------------------------- tn_bond_deflate
def bond_norms2(side, C):
    """Squared norms of the bond slices of C: rows (side 0, C is k x n) or columns (side 1, C is n x k), rounded once from the exact
    value (inputs built from small integers times powers of two make them exact, so any summation order agrees)."""
    C = np.asarray(C, dtype=np.float64)
    S = C if side == 0 else C.T
    out = []
    for r in S:
        if not np.all(np.isfinite(r)):
            out.append(float(np.sum(r * r)))         # inf or NaN: only its class matters
        else:
            out.append(float(exact_dot(r, r)[0]))
    return np.array(out)


def bond_deflate_ref(h):
    """The rule of tn_bond_deflate on the squared norms h (k of them): (rc, kept indices, dropped2_rel).
    rc -2: a norm is NaN or above 1.7e308.  Nothing is dropped when k == 1 or max h == 0.  Otherwise the indices are visited in
    ascending order of h (equal h by increasing index) and dropped while the running sum of the dropped h stays <= eps^2 max h,
    at most k - 1 of them; the kept indices stay in their order."""
    h = [float(x) for x in h]
    k = len(h)
    for x in h:
        if not (x == x) or x > 1.7e308:
            return -2, None, None
    nmax = max([0.0] + h)
    if not (nmax > 0.0) or k == 1:
        return 0, list(range(k)), 0.0
    order = sorted(range(k), key=lambda i: (h[i], i))
    budget = EPS * EPS * nmax
    acc, drop = 0.0, set()
    for t in range(k - 1):
        v = h[order[t]]
        if not (acc + v <= budget):
            break
        acc += v
        drop.add(order[t])
    if not drop:
        return 0, list(range(k)), 0.0
    return 0, [i for i in range(k) if i not in drop], acc / nmax


def bond_deflate_apply(side, C, Q, kept):
    """(C_out, Q_out) gathered to the kept bond indices."""
    kept = np.asarray(kept, dtype=np.int64)
    if side == 0:
        return C[kept, :], Q[:, kept]
    return C[:, kept], Q[kept, :]


# ---------------------------------------------------------------------------------------------------------- tn_scale_phys
def scale_phys_ref(A, diag, inv=False):
    A = np.asarray(A, dtype=np.float64)
    d = np.asarray(diag, dtype=np.float64)[:A.shape[1]][None, :, None]
    return A / d if inv else A * d


def ulps(x, y):
    """Distance in units in the last place between two arrays of finite doubles of equal sign structure (elementwise)."""
    xi = np.asarray(x, dtype=np.float64).view(np.int64)
    yi = np.asarray(y, dtype=np.float64).view(np.int64)
    m = np.int64(0x7FFFFFFFFFFFFFFF)
    xi = np.where(xi < 0, -(xi & m), xi)
    yi = np.where(yi < 0, -(yi & m), yi)
    return np.abs(xi - yi)


def spread(rng, n, decades=100):
    """n random values with magnitudes spread over 10^-decades .. 10^decades and random signs."""
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-decades, decades, n)

