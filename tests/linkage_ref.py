"""Reference of tn_state_linkage and tnac4o.calculate_state_linkage, numpy only: dense distances with fold and lanes, Kruskal under the
total order key(a, b) = (d(a, b), min(a, b), max(a, b)), the nearest other row, labels at a threshold, the cluster counts and the
scipy-format matrix; and the rows of the test cases."""
import numpy as np


# ---------------------------------------------------------------------------------------------- distances
def entries(rows, nbits, lanes16):
    """(M, nbits) entries of packed rows (M, ld) uint64: the bits, or the 16-bit lanes; whatever lies behind them is dropped."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    M = rows.shape[0]
    if lanes16:
        return rows.view('<u2').reshape(M, 4 * rows.shape[1])[:, :nbits].astype(np.int64)
    return np.unpackbits(rows.view(np.uint8).reshape(M, 8 * rows.shape[1]), axis=1, bitorder='little')[:, :nbits].astype(np.int64)


def dense(rows, nbits, lanes16=False, fold=False):
    """(M, M) int64: d(a, b) = the entries that differ; fold: min(d, nbits - d)."""
    X = entries(rows, nbits, lanes16)
    D = np.zeros((X.shape[0], X.shape[0]), dtype=np.int64)
    for a in range(X.shape[0]):
        D[a] = np.count_nonzero(X != X[a][None, :], axis=1)
    return np.minimum(D, nbits - D) if fold else D


# ---------------------------------------------------------------------------------------------- the tree
def find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def kruskal(D):
    """(pairs (M - 1, 2) int64 with lo < hi, dist (M - 1,) int64): the minimum spanning tree under (d, lo, hi), in ascending order."""
    M = D.shape[0]
    lo, hi = np.triu_indices(M, 1)
    order = np.lexsort((hi, lo, D[lo, hi]))
    parent = list(range(M))
    pairs, dist = [], []
    for e in order:
        a, b = find(parent, int(lo[e])), find(parent, int(hi[e]))
        if a != b:
            parent[max(a, b)] = min(a, b)
            pairs.append((int(lo[e]), int(hi[e])))
            dist.append(int(D[lo[e], hi[e]]))
            if len(pairs) == M - 1:
                break
    return np.array(pairs, dtype=np.int64).reshape(-1, 2), np.array(dist, dtype=np.int64)


def prim(D):
    """The same tree by Prim from row 0, brute force: in every step the smallest key (d, lo, hi) among all edges that leave the tree;
    returned sorted by key."""
    M = D.shape[0]
    inside = [0] if M else []
    edges = []
    while len(inside) < M:
        best = None
        for a in inside:
            for b in range(M):
                if b not in inside:
                    k = (int(D[a, b]), min(a, b), max(a, b))
                    if best is None or k < best:
                        best = k
        edges.append(best)
        inside.append(best[1] if best[1] not in inside else best[2])
    edges.sort()
    return np.array([(lo, hi) for _, lo, hi in edges], dtype=np.int64).reshape(-1, 2), np.array([d for d, _, _ in edges], dtype=np.int64)


def boruvka_rounds(D):
    """The rounds of a plain Boruvka under the same order (every component takes its smallest leaving edge, all are joined)."""
    M = D.shape[0]
    parent = list(range(M))
    rounds = 0
    while True:
        comp = [find(parent, a) for a in range(M)]
        if len(set(comp)) <= 1:
            return rounds
        rounds += 1
        best = {}
        for a in range(M):
            for b in range(M):
                if comp[a] != comp[b]:
                    k = (int(D[a, b]), min(a, b), max(a, b))
                    if comp[a] not in best or k < best[comp[a]]:
                        best[comp[a]] = k
        for _, lo, hi in best.values():
            a, b = find(parent, lo), find(parent, hi)
            parent[max(a, b)] = min(a, b)


def nearest(D):
    """(index (M,), distance (M,)) int64 of the b != a that minimises (d(a, b), b); -1, -1 for a single row."""
    M = D.shape[0]
    if M < 2:
        return np.full(M, -1, dtype=np.int64), np.full(M, -1, dtype=np.int64)
    big = D.astype(np.int64) * M + np.arange(M)[None, :]
    big[np.arange(M), np.arange(M)] = np.iinfo(np.int64).max
    idx = np.argmin(big, axis=1)
    return idx.astype(np.int64), D[np.arange(M), idx].astype(np.int64)


def run(rows, nbits, lanes16=False, fold=False):
    """The dict tn_state_linkage is compared with: edge_lo, edge_hi, edge_dist, nn_index, nn_dist (int64)."""
    D = dense(rows, nbits, lanes16, fold)
    pairs, dist = kruskal(D)
    nn, nd = nearest(D)
    return dict(edge_lo=pairs[:, 0], edge_hi=pairs[:, 1], edge_dist=dist, nn_index=nn, nn_dist=nd)


# ---------------------------------------------------------------------------------------------- from the tree
def canonical(labels):
    """Labels renumbered by the ascending smallest member of each set."""
    labels = np.asarray(labels)
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[np.asarray(inv).reshape(-1)].astype(np.int64)


def labels_at(pairs, dist, M, t):
    """The clusters of the tree's edges with d <= t, numbered by their ascending smallest member."""
    parent = list(range(M))
    for (a, b), d in zip(pairs.tolist(), dist.tolist()):
        if d <= t:
            a, b = find(parent, a), find(parent, b)
            parent[max(a, b)] = min(a, b)
    return canonical([find(parent, a) for a in range(M)])


def threshold_components(D, t):
    """The connected components of the explicit graph {a, b: d(a, b) <= t}, by search from every unvisited row in ascending order:
    labels numbered by ascending smallest member."""
    M = D.shape[0]
    labels = np.full(M, -1, dtype=np.int64)
    k = 0
    for s in range(M):
        if labels[s] >= 0:
            continue
        labels[s] = k
        todo = [s]
        while todo:
            a = todo.pop()
            for b in np.flatnonzero((D[a] <= t) & (labels < 0)):
                labels[b] = k
                todo.append(int(b))
        k += 1
    return labels


def cluster_counts(dist, M, n):
    return np.array([M - int(np.count_nonzero(dist <= t)) for t in range(n + 1)], dtype=np.int64)


def linkage_matrix(pairs, dist, M):
    """scipy's format from the sorted edges: merge i creates cluster M + i, the smaller id first."""
    ident = {a: (a, 1) for a in range(M)}                               # root -> (cluster id, size)
    parent = list(range(M))
    Z = np.zeros((max(M - 1, 0), 4))
    for i, ((a, b), d) in enumerate(zip(pairs.tolist(), dist.tolist())):
        ra, rb = find(parent, a), find(parent, b)
        (ia, sa), (ib, sb) = ident[ra], ident[rb]
        Z[i] = (min(ia, ib), max(ia, ib), d, sa + sb)
        parent[rb] = ra
        ident[ra] = (M + i, sa + sb)
    return Z


def same_partition(a, b):
    return np.array_equal(canonical(a), canonical(b))


# ---------------------------------------------------------------------------------------------- rows of the cases
PAD = 1                                                                 # words behind a row (ldr = nwords + 1), poisoned


def nwords_of(nbits, lanes16):
    return -(-nbits // (4 if lanes16 else 64))


def frame(rows, nbits, lanes16, seed):
    """(M, nwords + PAD) uint64: the rows (M, nwords) with random words behind them and random bits beyond nbits in the last word."""
    rng = np.random.default_rng(seed)
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    M, nw = rows.shape
    out = rng.integers(0, 2 ** 63, (M, nw + PAD), dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    out[:, :nw] = rows
    per, width = (4, 16) if lanes16 else (64, 1)
    used = (nbits - (nw - 1) * per) * width
    if used < 64 and M:
        junk = rng.integers(0, 2 ** 62, M, dtype=np.int64).astype(np.uint64) << np.uint64(used)
        keep = np.uint64((1 << used) - 1)
        out[:, nw - 1] = (out[:, nw - 1] & keep) | junk
    return out


def pack(X, lanes16):
    """(M, n) entries -> packed rows (M, nwords) uint64 (the layout of tnac4o_amd/overlap.py)."""
    X = np.asarray(X, dtype=np.int64)
    M, n = X.shape
    nw = nwords_of(n, lanes16)
    if lanes16:
        la = np.zeros((M, nw * 4), dtype='<u2')
        la[:, :n] = X
        return la.view('<u8').astype(np.uint64).reshape(M, nw)
    by = np.zeros((M, nw * 8), dtype=np.uint8)
    pk = np.packbits(X.astype(np.uint8), axis=1, bitorder='little')
    by[:, :pk.shape[1]] = pk
    return by.view('<u8').astype(np.uint64).reshape(M, nw)


def random_rows(M, nbits, seed, lanes16=False, alphabet=2):
    rng = np.random.default_rng(seed)
    return frame(pack(rng.integers(0, alphabet, (M, nbits)), lanes16), nbits, lanes16, seed + 1)


def ruler_rows(M):
    """The ruler path: row i differs from row i - 1 in r(i) = 1 + (the exponent of 2 in i) fresh bits, so that distances add along the
    path and the tree is the path (i - 1, i).  Returns (packed rows (M, nwords), nbits)."""
    r = [1 + ((i & -i).bit_length() - 1) for i in range(1, M)]
    nbits = int(sum(r))
    X = np.zeros((M, max(nbits, 1)), dtype=np.int64)
    at = 0
    for i in range(1, M):
        X[i] = X[i - 1]
        X[i, at:at + r[i - 1]] = 1
        at += r[i - 1]
    return pack(X, False), max(nbits, 1)


def folded_rows(M, nbits, seed):
    """Random rows; every third row is the complement of the row before it (distance 0 under fold)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 2, (M, nbits))
    for a in range(2, M, 3):
        X[a] = 1 - X[a - 1]
    return frame(pack(X, False), nbits, False, seed + 1)


def two_groups(nbits, seed):
    """Two far groups with duplicates inside: 40 rows near one random centre, 37 near its complement (each a copy of the centre with at
    most two bits flipped, many of them equal).  One long edge joins the groups, and it comes last."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2, nbits)
    X = np.array([c] * 40 + [1 - c] * 37)
    for a in range(X.shape[0]):
        if a % 3:
            X[a, rng.integers(0, nbits, a % 3)] ^= 1
    return frame(pack(X, False), nbits, False, seed + 1)
