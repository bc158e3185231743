"""Host references for tn_pair_hist and tnac4o.calculate_overlap_distribution (numpy and Python integers, no GPU).

- pair_dist_ref / pair_hist_ref: the pair histogram by brute force, the sums in Python integers.
- distribution_ref: P over the distances from all M^2 ordered pairs in float64, without condensing and without quantisation.
- exact_spin_overlap_law: the exact overlap law of two independent replicas of an enumerated Boltzmann law.
"""
import numpy as np


def unpack_rows(rows, nbits, lanes16):
    """(M, nbits) array of the bits (uint8) or 16-bit lanes (uint16) of packed rows (M, ld) uint64; what lies beyond nbits is cut."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    M = rows.shape[0]
    by = rows.astype('<u8').view(np.uint8).reshape(M, -1)
    if lanes16:
        return np.ascontiguousarray(by).view('<u2').reshape(M, -1)[:, :nbits].copy()
    return np.unpackbits(by, axis=1, bitorder='little')[:, :nbits].copy()


def pair_dist_ref(rows, nbits, lanes16):
    """(M, M) int64: the number of bits (lanes) in which rows a and b differ."""
    U = unpack_rows(rows, nbits, lanes16)
    M = U.shape[0]
    D = np.zeros((M, M), dtype=np.int64)
    for a in range(M):
        D[a] = np.count_nonzero(U != U[a], axis=1)
    return D


def pair_hist_ref(rows, nbits, w=None, lanes16=False, dist=None):
    """[sum_{a<b} w_a w_b [dist(a, b) = d] for d = 0 .. nbits] as Python integers.  w: None (all 1) or M integers."""
    D = pair_dist_ref(rows, nbits, lanes16) if dist is None else dist
    M = D.shape[0]
    wi = [1] * M if w is None else [int(x) for x in w]
    hist = [0] * (nbits + 1)
    for a in range(M):
        wa = wi[a]
        if wa == 0:
            continue
        row = D[a]
        for b in range(a + 1, M):
            hist[row[b]] += wa * wi[b]
    return hist


def limbs(hist):
    """Python integers -> (nbins, 2) uint64 (lo, hi)."""
    mask = (1 << 64) - 1
    assert all(0 <= h < 1 << 128 for h in hist)
    return np.array([[h & mask, h >> 64] for h in hist], dtype=np.uint64).reshape(len(hist), 2)


def distribution_ref(bits_or_states, w, kind):
    """(values, P): P[d] = sum_{a != b} w_a w_b [dist(a, b) = d] / sum_{a != b} w_a w_b over all ordered pairs in float64, straight
    from the (M, n) bits ('spin', 'link': Hamming distance, value 1 - 2 d / n) or cell states ('cell': cells that differ, value
    1 - d / n)."""
    X = np.asarray(bits_or_states)
    M, n = X.shape
    w = np.asarray(w, dtype=np.float64)
    if kind == 'cell':
        D = np.zeros((M, M), dtype=np.int64)
        for k in range(n):
            D += X[:, k][:, None] != X[:, k][None, :]
        values = 1.0 - np.arange(n + 1) / n
    else:
        S = 2.0 * X.astype(np.float64) - 1.0
        D = np.rint((n - S @ S.T) / 2.0).astype(np.int64)
        values = 1.0 - 2.0 * np.arange(n + 1) / n
    WW = np.outer(w, w)
    np.fill_diagonal(WW, 0.0)
    H = np.bincount(D.ravel(), weights=WW.ravel(), minlength=n + 1)
    return values, H / H.sum()


def exact_spin_overlap_law(p):
    """P over d = 0 .. n of the Hamming distance between two independent draws from the law p over the 2^n configurations of n <= 20
    spins (index bit i = spin i): r(z) = sum_x p(x) p(x ^ z) by a fast Walsh-Hadamard transform, binned by popcount(z).  The overlap
    at distance d is 1 - 2 d / n."""
    p = np.asarray(p, dtype=np.float64)
    n = int(p.size).bit_length() - 1
    assert p.size == 1 << n and n <= 20

    def fwht(a):
        a = a.copy()
        h = 1
        while h < a.size:
            a = a.reshape(-1, 2, h)
            a = np.stack([a[:, 0] + a[:, 1], a[:, 0] - a[:, 1]], axis=1).reshape(-1)
            h *= 2
        return a

    r = fwht(fwht(p) ** 2) / p.size
    z = np.arange(p.size, dtype=np.int64)
    pop = np.zeros(p.size, dtype=np.int64)
    for i in range(n):
        pop += (z >> i) & 1
    P = np.bincount(pop, weights=r, minlength=n + 1)
    return P / P.sum()
