"""Host references for tn_spin_moments and tnac4o.calculate_sample_correlations (numpy and Python integers, no GPU).

- make_rows / weight_sets: the inputs of the kernel tests: random bits with junk in the padding words and behind nbits.
- spin_moments_slow / spin_moments_ref: out[i][j] = sum_a w_a [x_a,i != x_a,j] with the two pseudo-bits, by the definition in Python
  integers (small cases) and by exact int64 matrix products of 16-bit digits of the weights (the tests' reference).
- sample_ref: m, C and the pair estimator <q_i q_j> from loops over the samples and over all pairs of samples in float64, without
  condensing, quantisation or the identity the host side uses.
- pair_sums_int: sum_{a<b} w_a w_b q_i(ab) q_j(ab) in Python integers.
- chi2d_ref: chi_SG(k_x, k_y) by plain loops over the spins.
- exact_spin_law: <s_i>, <s_i s_j> of an enumerated Boltzmann law.
"""
import numpy as np

from overlap_ref import PAD, WMAX, unpack_rows


def make_rows(M, nbits, seed):
    """(M, ceil(nbits / 64) + 3) uint64 of random words: the padding words and the bits behind nbits in the last word are junk.  Row 1
    repeats row 0, row M // 2 repeats row 2 (duplicates); the last row is the complement of row 0 within nbits."""
    rng = np.random.default_rng(seed)
    nw = -(-nbits // 64)
    rows = rng.integers(0, 2 ** 64, (M, nw + PAD), dtype=np.uint64)
    if M >= 3:
        rows[1, :nw] = rows[0, :nw]
    if M >= 6:
        rows[M // 2, :nw] = rows[2, :nw]
    if M >= 2:
        rows[M - 1, :nw] = ~rows[0, :nw]
    return rows


def weight_sets(M, seed):
    """name -> (weights or None, wmax): no weights, ones, random ones under three values of wmax (some above wmax: clamped; some zero),
    and all at the largest."""
    rng = np.random.default_rng(seed)
    r32 = rng.integers(0, 2 ** 32, M, dtype=np.uint64)
    r32[rng.random(M) < 0.2] = 0
    small = rng.integers(0, 12, M, dtype=np.uint64)                    # about half of them above wmax = 5
    return {'none': (None, 1), 'none_wide': (None, WMAX), 'ones': (np.ones(M, dtype=np.uint64), WMAX), 'random': (r32, WMAX),
            'clamp1': (small, 1), 'clamp5': (small, 5), 'clamp5_wide': (r32, 5), 'max': (np.full(M, WMAX, dtype=np.uint64), WMAX),
            'mid': (rng.integers(0, 2 ** 20, M, dtype=np.uint64), 2 ** 20 - 1)}


def bits_with_pseudo(rows, nbits):
    """(M, nbits + 2) int64: the bits of the rows, then the constant 0 and the constant 1."""
    U = unpack_rows(rows, nbits, False).astype(np.int64)
    M = U.shape[0]
    return np.concatenate([U, np.zeros((M, 1), dtype=np.int64), np.ones((M, 1), dtype=np.int64)], axis=1)


def spin_moments_slow(rows, nbits, w=None, wmax=None):
    """The definition, in Python integers: nested lists (nbits + 2) x (nbits + 2)."""
    X = bits_with_pseudo(rows, nbits).tolist()
    M, n2 = len(X), nbits + 2
    wi = [1] * M if w is None else [min(int(v), int(wmax)) if wmax is not None else int(v) for v in w]
    out = [[0] * n2 for _ in range(n2)]
    for a in range(M):
        for i in range(n2):
            for j in range(n2):
                if X[a][i] != X[a][j]:
                    out[i][j] += wi[a]
    return out


def spin_moments_ref(rows, nbits, w=None, wmax=None):
    """(nbits + 2, nbits + 2) object array of Python integers.  The weights (clamped to wmax) are cut into 16-bit digits; per digit
    X^T diag(d) (1 - X) + (1 - X)^T diag(d) X in int64 is exact (below M 2^16 < 2^63); the digits are put together in Python integers."""
    X = bits_with_pseudo(rows, nbits)
    M, n2 = X.shape
    wi = np.ones(M, dtype=np.uint64) if w is None else np.asarray(w, dtype=np.uint64)
    if w is not None and wmax is not None:
        wi = np.minimum(wi, np.uint64(wmax))
    assert M < 2 ** 40
    out = np.zeros((n2, n2), dtype=object)
    for k in range(2):
        d = ((wi >> np.uint64(16 * k)) & np.uint64(0xffff)).astype(np.int64)
        if not d.any():
            continue
        A = (X * d[:, None]).T @ (1 - X)
        out = out + (A + A.T).astype(object) * (1 << (16 * k))
    return out


def to_ints(out):
    """int64 array holding unsigned 64-bit values -> object array of Python integers."""
    return np.ascontiguousarray(np.asarray(out)).astype(np.int64, copy=False).view(np.uint64).astype(object)


def sample_ref(bits, w, pairs=True):
    """dict(m (n,), C (n, n), QQ (n, n) or None): sigma = 2 bit - 1; m and C are weighted means over the samples, QQ the weighted mean
    of q_i(ab) q_j(ab), q_i(ab) = sigma_i^a sigma_i^b, over all pairs a != b (a loop over a; the pairs with b = a get weight 0).
    float64."""
    S = 2.0 * np.asarray(bits, dtype=np.float64) - 1.0
    w = np.asarray(w, dtype=np.float64)
    M, n = S.shape
    m = (w @ S) / w.sum()
    C = (S.T * w) @ S / w.sum()
    QQ = None
    if pairs:
        acc, tot = np.zeros((n, n)), 0.0
        for a in range(M):
            if w[a] == 0:
                continue
            p = w[a] * w
            p[a] = 0.0
            Q = S * S[a]
            acc += (Q.T * p) @ Q
            tot += p.sum()
        QQ = acc / tot
    return dict(m=m, C=C, QQ=QQ)


def pair_sums_int(bits, w):
    """(num (n, n) object array, den): num_ij = sum_{a<b} w_a w_b q_i(ab) q_j(ab), den = sum_{a<b} w_a w_b, Python integers."""
    S = (2 * np.asarray(bits, dtype=np.int64) - 1)
    M, n = S.shape
    wi = [int(v) for v in w]
    num, den = np.zeros((n, n), dtype=object), 0
    for a in range(M):
        for b in range(a + 1, M):
            q = S[a] * S[b]
            num = num + np.outer(q, q).astype(object) * (wi[a] * wi[b])
            den += wi[a] * wi[b]
    return num, den


def chi2d_ref(QQ, gx, gy, Nx, Ny):
    """chi(k_x, k_y) = (1 / N) sum_ij QQ_ij cos(k_x (x_i - x_j) + k_y (y_i - y_j)), k = 2 pi (m_x / Nx, m_y / Ny): (Nx, Ny), the
    terms of a wave vector added without rounding."""
    import math
    QQ = np.asarray(QQ, dtype=np.float64)
    gx, gy = np.asarray(gx, dtype=np.float64), np.asarray(gy, dtype=np.float64)
    dx, dy = gx[:, None] - gx[None, :], gy[:, None] - gy[None, :]
    out = np.zeros((Nx, Ny))
    for mx in range(Nx):
        for my in range(Ny):
            out[mx, my] = math.fsum((QQ * np.cos(2.0 * np.pi * (mx * dx / Nx + my * dy / Ny))).ravel()) / QQ.shape[0]
    return out


def exact_spin_law(J, beta, L, act):
    """(m (n,), C (n, n), p): <sigma_i> and <sigma_i sigma_j> over the active spins `act` (sorted) of the Boltzmann law of J at beta,
    sigma = +1 where the bit is 1, by enumeration of the 2^n configurations (n <= 20)."""
    from tnac4o_amd import auxx
    n = len(act)
    assert n <= 20
    binary = np.zeros((2 ** n, L), dtype=np.int8)
    binary[:, act] = (np.arange(2 ** n)[:, None] >> np.arange(n)[None, :]) & 1
    E = auxx.energy_Jij(J, binary)
    p = np.exp(-beta * (E - E.min()))
    p /= p.sum()
    S = 2.0 * binary[:, act].astype(np.float64) - 1.0
    return p @ S, (S.T * p) @ S, p
