"""Host references for tn_pair_hist and tnac4o.calculate_overlap_distribution (numpy and Python integers, no GPU).

- pair_dist_ref / pair_hist_ref: the pair histogram by brute force, the sums in Python integers.
- distribution_ref: P over the distances from all M^2 ordered pairs in float64, without condensing and without quantisation.
- exact_spin_overlap_law: the exact overlap law of two independent replicas of an enumerated Boltzmann law.
- what the tests of tn_pair_hist, tn_pair_moments and tn_spin_moments share: the small solvers, states_with_duplicates and source for
  the pipeline tests, make_rows / weight_sets for the kernel tests, last_error, first_diffs.
"""
import numpy as np

PAD = 3                                                                # words of random padding behind a row
WMAX = 2 ** 32 - 1


def droplet(beta=3.0):
    import golden_inputs as gi
    import tnac4o_amd
    return tnac4o_amd.tnac4o(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=beta)


def ising3x3(beta=1.0):
    import marginals_ref as mr
    import tnac4o_amd
    return tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=beta)


def rmf(beta=1.0):
    import tnac4o_amd
    from tnac4o_amd import auxx
    return tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=3, J=auxx.synthetic_rmf(3, 3, 3, 17), beta=beta)


def states_with_duplicates(M, rng, distinct):
    """(M, 16) cell states of the droplet lattice drawn from `distinct` configurations that differ from one another in a few cells."""
    base = rng.integers(0, 256, 16)
    pool = np.tile(base, (distinct, 1))
    for k in range(distinct):
        cells = rng.integers(0, 16, rng.integers(0, 5))
        pool[k, cells] = rng.integers(0, 256, cells.size)
    return pool[rng.integers(0, distinct, M)]


def source(s, kind, unsigned=False):
    """(M, n) of what `kind` compares in the states of solver s: the spin or link bits, or the cell states as int64 -- as they are stored
    (int8 states above 127 negative), or, unsigned, in 0 .. 255."""
    from tnac4o_amd import overlap
    if kind == 'cell':
        st = np.asarray(s.states).astype(np.int64)
        return st & 0xff if unsigned else st
    return {'spin': overlap.spin_bits, 'link': overlap.link_bits}[kind](s)


def last_error(L):
    import ctypes as ct
    buf = ct.create_string_buffer(512)
    L.tn_last_error(buf, 512)
    return buf.value.decode()


def first_diffs(got, want):
    """The first four entries in which two square tables (nested lists or arrays) differ: (i, j, got, want)."""
    return [(i, j, got[i][j], want[i][j]) for i in range(len(want)) for j in range(len(want)) if got[i][j] != want[i][j]][:4]


def make_rows(M, nbits, lanes16, seed):
    """(M, ld) uint64 with ld = nwords + 3: random rows, random words in the padding, random bits (lanes) beyond nbits in the last
    word; row 1 repeats row 0 and M // 2 repeats row 2 (duplicates), the last row differs from row 0 everywhere (bin nbits)."""
    rng = np.random.default_rng(seed)
    per = 4 if lanes16 else 64
    nwords = -(-nbits // per)
    if lanes16:
        U = rng.integers(0, 32768, (M, nwords * 4)).astype('<u2')
        if M >= 2:
            U[M - 1] = (U[0] + 1 + rng.integers(0, 32766, nwords * 4)) % 32768
        body = U.view('<u8').astype(np.uint64)
    else:
        body = rng.integers(0, 2 ** 64, (M, nwords), dtype=np.uint64)
        if M >= 2:
            body[M - 1] = ~body[0]
    rows = rng.integers(0, 2 ** 64, (M, nwords + PAD), dtype=np.uint64)
    rows[:, :nwords] = body
    if M >= 3:
        rows[1, :nwords] = rows[0, :nwords]
    if M >= 6:
        rows[M // 2, :nwords] = rows[2, :nwords]
    if nbits % per:                                                    # what lies beyond nbits in the last word differs from row to row
        cut = (nbits % per) * (16 if lanes16 else 1)
        junk = rng.integers(0, 2 ** 64, M, dtype=np.uint64) << np.uint64(cut)
        keep = np.uint64((1 << cut) - 1)
        rows[:, nwords - 1] = (rows[:, nwords - 1] & keep) | junk
    return rows


def weight_sets(M, wmax, seed):
    rng = np.random.default_rng(seed)
    some_zero = rng.integers(0, wmax + 1, M, dtype=np.uint64)
    some_zero[rng.random(M) < 0.3] = 0
    if M >= 2:
        some_zero[0] = 0
    return {'none': None, 'random': rng.integers(0, wmax + 1, M, dtype=np.uint64), 'max': np.full(M, wmax, dtype=np.uint64), 'zeros': some_zero}


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
