"""Host reference of tn_cluster_exchange and tnac4o.exchange_clusters (Python integers and numpy, no GPU).

- reach / seed_bit / move: the move on masks held as Python integers -- breadth-first search over the CSR with the library's clamping
  and skipping rules, the seed rule r = min(floor(u cnt), cnt - 1).
- run: one library call on packed rows (M, ld) uint64: (rows, size_out, diff_out).
- the graphs and the shared case table of tests/test_gpu_exchange.py.
- pair_chain: the exact transition table of the chain of a PAIR of replicas on a small model.
"""
import numpy as np

PAD = 3                                                                # words of poisoned padding behind a row
SIZES = (1, 63, 64, 65, 130, 4096, 4097)                               # nbits: word edges, the last one-wave row and the first workgroup row
U_MAX = float(np.nextafter(1.0, 0.0))


# ---------------------------------------------------------------------------------------------- the move on masks
def arcs(i, rowptr, cols):
    """The neighbours the library reads for bit i: the range clamped to [0, nnz] (empty when that is none)."""
    beg, end = max(int(rowptr[i]), 0), min(int(rowptr[i + 1]), len(cols))
    return cols[beg:end] if beg < end else cols[:0]


def reach(D, seed, nbits, rowptr, cols):
    """The bits reachable from `seed` along listed arcs through bits of the mask D (a Python integer), the seed included; a neighbour
    outside [0, nbits) is skipped."""
    C = 1 << seed
    todo = [seed]
    while todo:
        i = todo.pop()
        for j in arcs(i, rowptr, cols):
            j = int(j)
            if 0 <= j < nbits and (D >> j) & 1 and not (C >> j) & 1:
                C |= 1 << j
                todo.append(j)
    return C


def seed_bit(D, u):
    """The r-th set bit of D in ascending index, r = min(floor(u cnt), cnt - 1): one IEEE multiplication and a floor."""
    cnt = bin(D).count('1')
    r = min(int(np.floor(np.float64(u) * np.float64(cnt))), cnt - 1)
    for _ in range(r):
        D &= D - 1
    return (D & -D).bit_length() - 1


def move(a, b, u, nbits, rowptr, cols):
    """(a ^ C, b ^ C, |C|, cnt) for two rows held as Python integers of nbits bits."""
    D = (a ^ b) & ((1 << nbits) - 1)
    cnt = bin(D).count('1')
    if cnt == 0:
        return a, b, 0, 0
    C = reach(D, seed_bit(D, u), nbits, rowptr, cols)
    return a ^ C, b ^ C, bin(C).count('1'), cnt


def row_int(words):
    return sum(int(w) << (64 * k) for k, w in enumerate(words))


def row_words(value, nwords):
    return [(value >> (64 * k)) & (2 ** 64 - 1) for k in range(nwords)]


def run(rows, nbits, rowptr, cols, pairs, uniforms):
    """One call of tn_cluster_exchange: rows (M, ld) uint64 -> (new rows, size_out (P,), diff_out (P,)) int64.  Words behind the row and
    bits beyond nbits stay as they are; a pair with an index outside [0, M) gives -1, -1 and touches nothing."""
    rows = np.array(rows, dtype=np.uint64)
    M, nwords = rows.shape[0], -(-nbits // 64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    size, diff = np.zeros(len(pairs), dtype=np.int64), np.zeros(len(pairs), dtype=np.int64)
    for p, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        if not (0 <= a < M and 0 <= b < M):
            size[p] = diff[p] = -1
            continue
        if a == b:
            continue
        ra, rb = row_int(rows[a, :nwords]), row_int(rows[b, :nwords])
        na, nb, size[p], diff[p] = move(ra, rb, uniforms[p], nbits, rowptr, cols)
        rows[a, :nwords] = np.array(row_words(na, nwords), dtype=np.uint64)
        rows[b, :nwords] = np.array(row_words(nb, nwords), dtype=np.uint64)
    return rows, size, diff


def popcounts(rows, nbits):
    """(M,) set bits of the first nbits bits of packed rows."""
    mask = (1 << nbits) - 1
    nwords = -(-nbits // 64)
    return np.array([bin(row_int(r[:nwords]) & mask).count('1') for r in np.asarray(rows, dtype=np.uint64)], dtype=np.int64)


# ---------------------------------------------------------------------------------------------- graphs
def csr(n, edges, both=True):
    """(rowptr (n + 1,), cols) int32 of the arcs i -> j of `edges` (and j -> i with both), the neighbours of a vertex ascending."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if both:
        e = np.concatenate([e, e[:, ::-1]])
    e = e[np.lexsort((e[:, 1], e[:, 0]))]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=n), out=rowptr[1:])
    return rowptr.astype(np.int32), e[:, 1].astype(np.int32)


def path_edges(n):
    return [(i, i + 1) for i in range(n - 1)]


def star_edges(n):
    return [(0, i) for i in range(1, n)]


def clique_edges(n):
    """Two cliques of k = min(8, n // 2) vertices at both ends of the range, joined by one arc; what lies between them is isolated."""
    k = min(8, n // 2)
    left, right = list(range(k)), list(range(n - k, n))
    e = [(i, j) for g in (left, right) for i in g for j in g if i < j]
    return e + ([(left[-1], right[0])] if k else [])


def random_edges(n, rng, degree=3):
    m = (n * degree) // 2
    e = rng.integers(0, n, (m, 2))
    return [tuple(x) for x in e if x[0] != x[1]]


def chimera_edges(Ny, Nx):
    """Cells of 8 spins, spin 8 (ny Nx + nx) + k: K_4,4 inside a cell, k < 4 coupled to the cell below, k >= 4 to the cell on the right."""
    e = []
    for ny in range(Ny):
        for nx in range(Nx):
            c = 8 * (ny * Nx + nx)
            e += [(c + i, c + 4 + j) for i in range(4) for j in range(4)]
            if ny + 1 < Ny:
                e += [(c + k, c + 8 * Nx + k) for k in range(4)]
            if nx + 1 < Nx:
                e += [(c + k, c + 8 + k) for k in range(4, 8)]
    return e


# ---------------------------------------------------------------------------------------------- rows
def poison(body, nbits, rng):
    """(M, nwords) -> (M, nwords + PAD): random words behind the row, random bits beyond nbits in the last word."""
    M, nwords = body.shape
    rows = rng.integers(0, 2 ** 64, (M, nwords + PAD), dtype=np.uint64)
    rows[:, :nwords] = body
    if nbits % 64:
        keep = np.uint64((1 << (nbits % 64)) - 1)
        junk = rng.integers(0, 2 ** 64, M, dtype=np.uint64) << np.uint64(nbits % 64)
        rows[:, nwords - 1] = (rows[:, nwords - 1] & keep) | junk
    return rows


def rows_from_masks(base, masks, nbits, rng):
    """Rows 2k, 2k + 1 = a random row and the same row with the bits of masks[k] (a Python integer) flipped, poisoned."""
    nwords = -(-nbits // 64)
    body = np.zeros((2 * len(masks), nwords), dtype=np.uint64)
    for k, m in enumerate(masks):
        a = row_int(rng.integers(0, 2 ** 64, nwords, dtype=np.uint64)) if base is None else base
        body[2 * k] = row_words(a, nwords)
        body[2 * k + 1] = row_words(a ^ m, nwords)
    return poison(body, nbits, rng)


def random_rows(M, nbits, rng):
    return poison(rng.integers(0, 2 ** 64, (M, -(-nbits // 64)), dtype=np.uint64), nbits, rng)


def in_order_pairs(M):
    return np.arange(2 * (M // 2), dtype=np.int32).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------- the shared cases
FAMILIES = ('path-full', 'path-gap', 'star', 'cliques', 'isolated', 'random', 'one-way', 'bad-neighbour', 'bad-rowptr', 'pow2')
CASES = [(f, n) for f in FAMILIES for n in SIZES] + [('chimera', 128)]


def case_inputs(case):
    """dict(nbits, rowptr, cols, rows (M, nwords + PAD) uint64, pairs (P, 2) int32, uniforms (P,)) of a case (family, nbits)."""
    family, n = case
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + n if family in FAMILIES else 7)
    full = (1 << n) - 1
    few = 12 if n <= 130 else 4                                          # pairs of random rows
    if family == 'path-full':                                            # every bit differs, the seed at one end: n - 1 growth steps
        rowptr, cols = csr(n, path_edges(n))
        rows, u = rows_from_masks(None, [full], n, rng), [0.0]
    elif family == 'path-gap':                                           # the middle spin equal: the cluster stops at the gap, from either end
        rowptr, cols = csr(n, path_edges(n))
        gap = full & ~(1 << (n // 2))
        rows, u = rows_from_masks(None, [gap, gap], n, rng), [0.0, U_MAX]
    elif family == 'star':                                               # one CSR row of n - 1 arcs; seeds at the centre, at a leaf, anywhere
        rowptr, cols = csr(n, star_edges(n))
        masks = [full, full, full & ~1] + [row_int(rng.integers(0, 2 ** 64, -(-n // 64), dtype=np.uint64)) & full for _ in range(few)]
        rows, u = rows_from_masks(None, masks, n, rng), [0.0, U_MAX, 0.5] + list(rng.random(few))
    elif family == 'cliques':
        rowptr, cols = csr(n, clique_edges(n))
        k = min(8, n // 2)
        masks = [full, full, full & ~(1 << max(k - 1, 0)), full & ~(1 << (n - k))] + \
                [row_int(rng.integers(0, 2 ** 64, -(-n // 64), dtype=np.uint64)) & full for _ in range(few)]
        rows, u = rows_from_masks(None, masks, n, rng), [0.0, U_MAX, 0.0, 0.0] + list(rng.random(few))
    elif family == 'isolated':                                           # no arc at all (nnz = 0): the cluster is the seed
        rowptr, cols = csr(n, [])
        rows = random_rows(2 * few, n, rng)
        u = [0.0, U_MAX] + list(rng.random(few - 2))
    elif family in ('random', 'one-way'):                                # one-way: arcs in one direction only, directed reachability
        rowptr, cols = csr(n, random_edges(n, rng) if n > 1 else [], both=family == 'random')
        rows = random_rows(2 * few + 1, n, rng)                         # (odd M: the last row has no partner)
        u = list(rng.random(few))
    elif family == 'bad-neighbour':                                      # neighbours outside [0, n) among the arcs: skipped
        e = np.array(random_edges(n, rng) + path_edges(n), dtype=np.int64).reshape(-1, 2)
        rowptr, cols = csr(n, e)
        cols = cols.copy()
        bad = np.array([-1, n, n + 63, 2 ** 31 - 1, -2 ** 31, 65536], dtype=np.int64)
        if cols.size:
            where = rng.choice(cols.size, max(1, cols.size // 4), replace=False)
            cols[where] = bad[rng.integers(0, bad.size, where.size)].astype(np.int32)
        else:
            rowptr, cols = np.array([0, 3], dtype=np.int32), np.array([-1, 1, 2 ** 31 - 1], dtype=np.int32)
        rows = random_rows(2 * few, n, rng)
        u = list(rng.random(few))
    elif family == 'bad-rowptr':                                         # entries beyond nnz, below 0 and out of order: clamped ranges
        rowptr, cols = csr(n, random_edges(n, rng) + path_edges(n))
        rowptr = rowptr.copy()
        nnz = cols.size
        bad = np.array([nnz + 1, nnz + 1000, 2 ** 31 - 1, -1, -2 ** 31, 0, nnz], dtype=np.int64)
        where = rng.choice(n + 1, min(max(1, (n + 1) // 5), 12), replace=False)    # (few: a clamped range can span every arc)
        rowptr[where] = bad[rng.integers(0, bad.size, where.size)].astype(np.int32)
        rows = random_rows(2 * few, n, rng)
        u = list(rng.random(few))
    elif family == 'pow2':                                               # cnt a power of two, u = k / cnt: the products are integers
        rowptr, cols = csr(n, [])
        cnt = 1 << min(3, n.bit_length() - 1)
        mask = sum(1 << int(i) for i in rng.choice(n, cnt, replace=False))
        rows, u = rows_from_masks(None, [mask] * cnt, n, rng), [k / cnt for k in range(cnt)]
    else:                                                                # chimera 4 x 4, Nc = 8: 128 spins, 64 random rows
        rowptr, cols = csr(128, chimera_edges(4, 4))
        rows = random_rows(64, 128, rng)
        u = list(rng.random(32))
    return dict(nbits=n, rowptr=rowptr, cols=cols, rows=rows, pairs=in_order_pairs(rows.shape[0]), uniforms=np.array(u, dtype=np.float64))


_REFERENCE = {}


def case_reference(case):
    """(rows, size, diff) of run() on a case, computed once."""
    if case not in _REFERENCE:
        c = case_inputs(case)
        _REFERENCE[case] = run(c['rows'], c['nbits'], c['rowptr'], c['cols'], c['pairs'], c['uniforms'])
    return _REFERENCE[case]


# ---------------------------------------------------------------------------------------------- the chain of a pair of replicas
def small_model(seed=5):
    """6 spins with integer couplings and fields: a triangle 0-1-2, 2-3, the pendant spin 4 on 3, the isolated spin 5.
    (n, edges, J per edge, h (n,))."""
    rng = np.random.default_rng(seed)
    edges = [(0, 1), (1, 2), (0, 2), (2, 3), (3, 4)]
    J = rng.choice([-3, -2, -1, 1, 2, 3], len(edges))
    h = rng.choice([-2, -1, 1, 2], 6)
    return 6, edges, J, h


def model_energies(n, edges, J, h):
    """(2^n,) int64: E(x) = sum J_ij s_i s_j + sum h_i s_i with s_i = 2 bit_i(x) - 1."""
    x = np.arange(1 << n)
    s = 2 * ((x[:, None] >> np.arange(n)[None, :]) & 1) - 1
    E = s @ np.asarray(h, dtype=np.int64)
    for (i, j), v in zip(edges, J):
        E = E + int(v) * s[:, i] * s[:, j]
    return E.astype(np.int64)


def pair_chain(n, edges):
    """The chain of the move on a pair (a, b) of configurations of n spins: (src, dst, num, den), one entry per (pair state, seed):
    the pair state src = a 2^n + b goes to dst with probability num / den, den = the number of differing spins (a pair of equal
    configurations stays with probability 1 / 1).  The seed k of cnt is picked through the library's rule with u = (k + 0.5) / cnt."""
    rowptr, cols = csr(n, edges)
    src, dst, den = [], [], []
    for a in range(1 << n):
        for b in range(1 << n):
            cnt = bin(a ^ b).count('1')
            for k in range(max(cnt, 1)):
                na, nb, _, _ = move(a, b, (k + 0.5) / max(cnt, 1), n, rowptr, cols)
                src.append((a << n) | b)
                dst.append((na << n) | nb)
                den.append(max(cnt, 1))
    return np.array(src), np.array(dst), np.ones(len(src), dtype=np.int64), np.array(den)
