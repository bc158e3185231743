"""Host references for tn_pair_moments and tnac4o.calculate_overlap_correlations (numpy and Python integers, no GPU).

- make_group_rows / weight_sets: the inputs of the kernel tests (those of overlap_ref, for grouped rows).
- group_dists / pair_moments_ref: out[i][j] = sum_{a<b} w_a w_b d_i d_j by brute force, the sums in Python integers.
- correlations_ref: <q_g>, <Q_g Q_g'>, C and chi from all M^2 ordered pairs in float64, without condensing or quantisation.
- chi_ref: chi(k_m) by plain loops.
- exact_line_moments: E[Q_g Q_g'] and Var(Q_g Q_g') of two independent replicas of an enumerated Boltzmann law.
"""
import numpy as np

from overlap_ref import make_rows, unpack_rows, weight_sets  # noqa: F401 (the tests take weight_sets from here)


def make_group_rows(M, G, wpg, lanes16, seed):
    """(M, G wpg + 3) uint64: make_rows for rows of G wpg whole words, so d_g(0, M - 1) is the largest distance, (4 or 64) wpg, in
    every group."""
    return make_rows(M, G * wpg * (4 if lanes16 else 64), lanes16, seed)


def dmax_of(wpg, lanes16):
    return (4 if lanes16 else 64) * wpg


def wmax_of(wpg, lanes16):
    """The largest wmax tn_pair_moments takes: wmax dmax <= 2^32 - 1."""
    return (2 ** 32 - 1) // dmax_of(wpg, lanes16)


def group_dists(rows, G, wpg, lanes16):
    """(G, M, M) int64: the number of bits (lanes) in which rows a and b differ within group g = words [g wpg, (g+1) wpg)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    M = rows.shape[0]
    per = 4 if lanes16 else 64
    D = np.zeros((G, M, M), dtype=np.int64)
    for g in range(G):
        U = unpack_rows(rows[:, g * wpg:(g + 1) * wpg], wpg * per, lanes16)
        for a in range(M):
            D[g, a] = np.count_nonzero(U != U[a], axis=1)
    return D


def pair_moments_ref(rows, G, wpg, w=None, wmax=None, lanes16=False, dist=None):
    """(G+1) x (G+1) nested lists of Python integers: out[i][j] = sum_{a<b} p d_i d_j with p = min(w_a, wmax) min(w_b, wmax), d_G = 1.
    The sum over the pairs is a float64 matrix product made exact: p (below 2^64 / dmax^2) is cut into 12-bit digits, and with
    d_i d_j <= dmax^2 <= 2^22 every partial sum of a digit's product is an integer below pairs x 4095 x dmax^2 < 2^53 (asserted), so
    float64 holds it exactly whatever the order of the additions; the digits are put together in Python integers."""
    D = group_dists(rows, G, wpg, lanes16) if dist is None else dist
    M = D.shape[1]
    out = [[0] * (G + 1) for _ in range(G + 1)]
    if M < 2:
        return out
    ia, ib = np.triu_indices(M, 1)
    X = np.ones((G + 1, ia.size), dtype=np.float64)
    X[:G] = D[:, ia, ib]
    wi = np.ones(M, dtype=np.uint64) if w is None else np.asarray(w, dtype=np.uint64)
    if wmax is not None:
        wi = np.minimum(wi, np.uint64(wmax))
    dmax = dmax_of(wpg, lanes16)
    assert int(wi.max()) * dmax < 2 ** 32
    p = wi[ia] * wi[ib]                                                # below 2^64: uint64 holds it
    assert ia.size * 4095 * dmax * dmax < 2 ** 53
    for k in range(6):
        digit = ((p >> np.uint64(12 * k)) & np.uint64(0xfff)).astype(np.float64)
        if not digit.any():
            continue
        S = (X * digit) @ X.T
        assert np.array_equal(S, np.rint(S)) and S.max() < 2.0 ** 53
        for i in range(G + 1):
            for j in range(G + 1):
                out[i][j] += int(S[i, j]) << (12 * k)
    return out


def limbs3(out):
    """nested Python integers -> (G+1, G+1, 2) uint64 (lo, hi)."""
    mask = (1 << 64) - 1
    n = len(out)
    assert all(0 <= v < 1 << 128 for r in out for v in r)
    return np.array([[[v & mask, v >> 64] for v in r] for r in out], dtype=np.uint64).reshape(n, n, 2)


def chi_ref(QQ, N):
    """chi(k_m), m = 0 .. G // 2, by loops; the terms of a k are added up without rounding."""
    import math
    G = len(QQ)
    out = []
    for m in range(G // 2 + 1):
        terms = [float(QQ[g][h]) * float(np.cos(2.0 * np.pi * m * (g - h) / G)) for g in range(G) for h in range(G)]
        out.append(math.fsum(terms) / float(N))
    return np.array(out)


def line_overlaps(X, group, G, kind):
    """(G, M, M) float64: Q_g(a, b) = sum over the columns of group g of s_a s_b ('spin', X bits) or of [x_a == x_b] ('cell')."""
    X = np.asarray(X)
    M = X.shape[0]
    Q = np.zeros((G, M, M))
    for g in range(G):
        cols = np.flatnonzero(np.asarray(group) == g)
        if kind == 'cell':
            for k in cols:
                Q[g] += X[:, k][:, None] == X[:, k][None, :]
        else:
            S = 2.0 * X[:, cols].astype(np.float64) - 1.0
            Q[g] = S @ S.T
    return Q


def correlations_ref(X, group, G, w, kind):
    """dict(mean (G,) = <q_g>, QQ (G, G) = <Q_g Q_g'>, C (G, G) = <q_g q_g'>, chi): weighted means over all ordered pairs a != b in
    float64 straight from the (M, n) bits or cell states; nan where a group is empty."""
    Q = line_overlaps(X, group, G, kind)
    w = np.asarray(w, dtype=np.float64)
    WW = np.outer(w, w)
    np.fill_diagonal(WW, 0.0)
    tot = WW.sum()
    n = np.bincount(np.asarray(group), minlength=G).astype(np.float64)
    QW = Q * WW
    mean = QW.sum(axis=(1, 2)) / tot
    QQ = np.einsum('gab,hab->gh', QW, Q) / tot
    with np.errstate(divide='ignore', invalid='ignore'):
        return dict(mean=np.where(n > 0, mean / n, np.nan), QQ=QQ, C=np.where(np.outer(n, n) > 0, QQ / np.outer(n, n), np.nan),
                    chi=chi_ref(QQ, n.sum()), sizes=n)


def exact_line_moments(p, group, G):
    """(E (G, G), V (G, G)): mean and variance of Q_g Q_g' for two independent draws from the law p over the 2^n configurations of n
    <= 20 spins (index bit i = spin i = column i of spin_bits), Q_g = n_g - 2 popcount(z restricted to group g) with z the XOR of
    the two configurations, whose law r(z) = sum_x p(x) p(x ^ z) comes from a fast Walsh-Hadamard transform, left unbinned."""
    p = np.asarray(p, dtype=np.float64)
    n = int(p.size).bit_length() - 1
    assert p.size == 1 << n and n <= 20 and len(group) == n

    def fwht(a):
        a = a.copy()
        h = 1
        while h < a.size:
            a = a.reshape(-1, 2, h)
            a = np.stack([a[:, 0] + a[:, 1], a[:, 0] - a[:, 1]], axis=1).reshape(-1)
            h *= 2
        return a

    r = fwht(fwht(p) ** 2) / p.size
    r /= r.sum()
    z = np.arange(p.size, dtype=np.int64)
    Q = np.zeros((G, p.size))
    for i in range(n):
        Q[group[i]] += 1.0 - 2.0 * ((z >> i) & 1)
    E, V = np.zeros((G, G)), np.zeros((G, G))
    for g in range(G):
        for h in range(G):
            t = Q[g] * Q[h]
            E[g, h] = r @ t
            V[g, h] = r @ (t * t) - E[g, h] ** 2
    return E, V
