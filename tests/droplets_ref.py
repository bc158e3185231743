"""Host reference of tn_droplets and tnac4o.calculate_droplets (Python integers, math.fsum and numpy, no GPU).

- row_droplets: the droplets of one row held as a Python integer -- roots ascending, the growth of exchange_ref.reach through what is
  left of D, the energy terms of the library's rule (a neighbour in D adds nothing, one outside adds -J g_i g_j, the field -h g_i), each
  energy the correctly rounded exact sum of its terms, and the bound (t + 1) 2^-52 sum |terms| of a sum of t terms in any order.
- run: one library call on packed rows: every output, and the bounds.
- the graphs with couplings and the shared case table of tests/test_gpu_droplets.py.
- brute_force: components by union-find and energies by two calls of auxx.energy_Jij, for small models.
- model_graph / public_reference: tnac4o.calculate_droplets from solver.J0 alone.
"""
import math

import numpy as np

import exchange_ref as xr

PAD = xr.PAD
SIZES = (1, 63, 64, 65, 128, 4096, 4097)                               # nbits: word edges, the last one-wave row and the first workgroup row
EPS = 2.0 ** -52


# ---------------------------------------------------------------------------------------------- one row
def row_droplets(x, g, nbits, rowptr, cols, vals, field):
    """[(root, size, C, terms)] of the row x against the reference g (Python integers), roots ascending; terms: the numbers whose sum is
    dE_C / 2, as Python floats, each a coupling or a field times +-1."""
    D = (x ^ g) & ((1 << nbits) - 1)
    rem, out = D, []
    while rem:
        root = (rem & -rem).bit_length() - 1
        C = xr.reach(rem, root, nbits, rowptr, cols)
        terms, c = [], C
        while c:
            i = (c & -c).bit_length() - 1
            c &= c - 1
            gi = 1.0 if (g >> i) & 1 else -1.0
            if field is not None:
                terms.append(-float(field[i]) * gi)
            beg, end = max(int(rowptr[i]), 0), min(int(rowptr[i + 1]), len(cols))
            for e in range(beg, end):
                j = int(cols[e])
                if 0 <= j < nbits and not (D >> j) & 1:
                    terms.append(-float(vals[e]) * gi * (1.0 if (g >> j) & 1 else -1.0))
        out.append((root, bin(C).count('1'), C, terms))
        rem &= ~C
    return out


def energy_and_bound(terms):
    """(2 fsum(terms) + 0.0, (t + 1) 2^-52 sum |2 terms|): the correctly rounded energy and what a sum of its t terms in any order, with the
    final sums of the kernel on top, may miss it by."""
    return 2.0 * math.fsum(terms) + 0.0, (len(terms) + 1) * EPS * 2.0 * math.fsum(abs(t) for t in terms)


def run(rows, ref, nbits, rowptr, cols, vals, field, K, M=None):
    """One call of tn_droplets: rows (M, ld) uint64, ref (>= nwords,) uint64 -> dict(count, diff, largest (M,) int64, de_total (M,), root,
    size (M, K) int64, de (M, K), size_hist (nbits + 1,) int64, labels (M, nbits) int32, de_bound (M, K), de_total_bound (M,), nterms (M,)
    = the terms of all droplets of a row, abs_sum (M,) = the sum of their magnitudes as they enter de_total)."""
    rows = np.asarray(rows, dtype=np.uint64)
    M = rows.shape[0] if M is None else M
    nwords = -(-nbits // 64)
    g = xr.row_int(np.asarray(ref, dtype=np.uint64)[:nwords])
    out = dict(count=np.zeros(M, dtype=np.int64), diff=np.zeros(M, dtype=np.int64), largest=np.zeros(M, dtype=np.int64), de_total=np.zeros(M),
               root=np.full((M, K), -1, dtype=np.int64), size=np.zeros((M, K), dtype=np.int64), de=np.zeros((M, K)),
               size_hist=np.zeros(nbits + 1, dtype=np.int64), labels=np.full((M, nbits), -1, dtype=np.int32), de_bound=np.zeros((M, K)),
               de_total_bound=np.zeros(M), nterms=np.zeros(M, dtype=np.int64), abs_sum=np.zeros(M))
    for m in range(M):
        drops = row_droplets(xr.row_int(rows[m, :nwords]), g, nbits, rowptr, cols, vals, field)
        every = []
        for k, (root, size, C, terms) in enumerate(drops):
            every += terms
            out['size_hist'][size] += 1
            if k < K:
                out['root'][m, k], out['size'][m, k] = root, size
                out['de'][m, k], out['de_bound'][m, k] = energy_and_bound(terms)
            while C:
                out['labels'][m, (C & -C).bit_length() - 1] = k
                C &= C - 1
        out['count'][m] = len(drops)
        out['diff'][m] = sum(d[1] for d in drops)
        out['largest'][m] = max([d[1] for d in drops] + [0])
        out['de_total'][m], out['de_total_bound'][m] = energy_and_bound(every)
        out['nterms'][m], out['abs_sum'][m] = len(every), 2.0 * math.fsum(abs(t) for t in every)
    return out


# ---------------------------------------------------------------------------------------------- graphs with couplings
def wcsr(n, edges, J, both=True):
    """(rowptr, cols, vals): exchange_ref.csr with the coupling J[k] of edge k on its arcs."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    v = np.asarray(J, dtype=np.float64).reshape(-1)
    if both:
        e, v = np.concatenate([e, e[:, ::-1]]), np.concatenate([v, v])
    order = np.lexsort((e[:, 1], e[:, 0]))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(e[:, 0], minlength=n), out=rowptr[1:])
    return rowptr.astype(np.int32), e[order, 1].astype(np.int32), np.ascontiguousarray(v[order])


def integer_J(count, rng):
    return rng.choice([-4.0, -2.0, -1.0, 1.0, 2.0, 4.0], count)


def flipped(ref_int, masks, nbits, rng):
    """(len(masks), nwords + PAD) uint64: the reference with the bits of each mask flipped, poisoned behind the row and beyond nbits."""
    nwords = -(-nbits // 64)
    body = np.array([xr.row_words(ref_int ^ m, nwords) for m in masks], dtype=np.uint64).reshape(len(masks), nwords)
    return xr.poison(body, nbits, rng)


def sparse_mask(n, count, rng):
    return sum(1 << int(i) for i in rng.choice(n, min(count, n), replace=False))


# ---------------------------------------------------------------------------------------------- the shared cases
FAMILIES = ('path-full', 'path-gap', 'star', 'cliques', 'isolated', 'random', 'real', 'one-way', 'bad-neighbour', 'bad-rowptr', 'alternating')
CASES = [(f, n) for f in FAMILIES for n in SIZES] + [('chimera', 128)]
K_DEFAULT = 6


def case_inputs(case):
    """dict(nbits, rowptr, cols, vals, field (or None), ref (nwords,) uint64 with random bits beyond nbits, rows (M, nwords + PAD) uint64,
    K, exact) of a case (family, nbits).  Row 0 equals the reference, row 1 is its complement.  exact: every coupling and field is a
    small integer, the energies have no rounding."""
    family, n = case
    rng = np.random.default_rng(5000 + 1000 * FAMILIES.index(family) + n if family in FAMILIES else 11)
    nwords = -(-n // 64)
    full = (1 << n) - 1
    ref = xr.poison(rng.integers(0, 2 ** 64, (1, nwords), dtype=np.uint64), n, rng)[0, :nwords]
    g = xr.row_int(ref) & full
    few = 6 if n <= 128 else 3
    masks = [0, full]
    field = rng.integers(-3, 4, n).astype(np.float64)
    exact, K = True, K_DEFAULT
    rand = [xr.row_int(rng.integers(0, 2 ** 64, nwords, dtype=np.uint64)) & full for _ in range(few)]
    thin = [sparse_mask(n, 9, rng) for _ in range(few)]
    if family == 'path-full':                                            # the complement is one droplet that takes n - 1 growth steps
        e = xr.path_edges(n)
        graph = wcsr(n, e, integer_J(len(e), rng))
    elif family == 'path-gap':                                           # one spin equal: two droplets that share it as a neighbour
        e = xr.path_edges(n)
        graph = wcsr(n, e, integer_J(len(e), rng))
        masks += [full & ~(1 << (n // 2)), full & ~(1 << (n // 2)) & ~1, full & ~(1 << (n - 1))]
        field = None
    elif family == 'star':
        e = xr.star_edges(n)
        graph = wcsr(n, e, integer_J(len(e), rng))
        masks += [full & ~1, 1] + rand + thin                            # without the centre: n - 1 single spins; the centre alone
    elif family == 'cliques':
        e = xr.clique_edges(n)
        graph = wcsr(n, e, integer_J(len(e), rng))
        k = min(8, n // 2)
        masks += [full & ~(1 << max(k - 1, 0)), full & ~(1 << (n - k))] + rand + thin
    elif family == 'isolated':                                           # no arc at all (nnz = 0): every droplet one spin, its energy the field's
        graph = wcsr(n, [], [])
        masks += rand + thin
    elif family in ('random', 'real', 'one-way'):                        # one-way: arcs in one direction only
        e = xr.random_edges(n, rng) if n > 1 else []
        J = rng.normal(size=len(e)) if family == 'real' else integer_J(len(e), rng)
        graph = wcsr(n, e, J, both=family != 'one-way')
        masks += rand + thin
        if family == 'real':
            field, exact = rng.normal(size=n), False
        if family == 'random':
            field = None
    elif family == 'bad-neighbour':                                      # neighbours outside [0, n) among the arcs: skipped
        e = np.array(xr.random_edges(n, rng) + xr.path_edges(n), dtype=np.int64).reshape(-1, 2)
        rowptr, cols, vals = wcsr(n, e, integer_J(len(e), rng))
        cols = cols.copy()
        bad = np.array([-1, n, n + 63, 2 ** 31 - 1, -2 ** 31, 65536], dtype=np.int64)
        if cols.size:
            where = rng.choice(cols.size, max(1, cols.size // 4), replace=False)
            cols[where] = bad[rng.integers(0, bad.size, where.size)].astype(np.int32)
        else:
            rowptr, cols, vals = np.array([0, 3], dtype=np.int32), np.array([-1, 1, 2 ** 31 - 1], dtype=np.int32), np.array([1.0, 2.0, 4.0])
        graph = (rowptr, cols, vals)
        masks += rand + thin
    elif family == 'bad-rowptr':                                         # entries beyond nnz, below 0 and out of order: clamped ranges
        e = xr.random_edges(n, rng) + xr.path_edges(n)
        rowptr, cols, vals = wcsr(n, e, integer_J(len(e), rng))
        rowptr = rowptr.copy()
        nnz = cols.size
        bad = np.array([nnz + 1, nnz + 1000, 2 ** 31 - 1, -1, -2 ** 31, 0, nnz], dtype=np.int64)
        where = rng.choice(n + 1, min(max(1, (n + 1) // 5), 12), replace=False)
        rowptr[where] = bad[rng.integers(0, bad.size, where.size)].astype(np.int32)
        graph = (rowptr, cols, vals)
        masks += thin                                                   # (few bits: a clamped range can span every arc)
    elif family == 'alternating':                                        # every second spin of a path: ceil(n / 2) droplets, far more than K
        e = xr.path_edges(n)
        graph = wcsr(n, e, integer_J(len(e), rng))
        masks += [sum(1 << i for i in range(0, n, 2)), sum(1 << i for i in range(1, n, 2))]
        K = 3
    else:                                                                # chimera 4 x 4, Nc = 8: 128 spins, 62 random and thin rows
        e = xr.chimera_edges(4, 4)
        graph = wcsr(128, e, integer_J(len(e), rng))
        masks += [xr.row_int(rng.integers(0, 2 ** 64, 2, dtype=np.uint64)) for _ in range(30)] + [sparse_mask(128, 12, rng) for _ in range(32)]
        K = 16
    rowptr, cols, vals = graph
    return dict(nbits=n, rowptr=rowptr, cols=cols, vals=vals, field=field, ref=ref, rows=flipped(g, masks, n, rng), K=K, exact=exact)


_REFERENCE = {}


def case_reference(case):
    """run() on a case, computed once."""
    if case not in _REFERENCE:
        c = case_inputs(case)
        _REFERENCE[case] = run(c['rows'], c['ref'], c['nbits'], c['rowptr'], c['cols'], c['vals'], c['field'], c['K'])
    return _REFERENCE[case]


# ---------------------------------------------------------------------------------------------- brute force on small models
def brute_force(n, edges, J, h, x, g):
    """[(root, size, dE)] of the bit tuples x against g on n spins: components of the subgraph induced on x != g by union-find, roots
    ascending; dE = energy_Jij(g with the component flipped) - energy_Jij(g), two calls."""
    from tnac4o_amd.auxx import energy_Jij
    x, g = np.asarray(x), np.asarray(g)
    D = x != g
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, j in edges:
        if D[i] and D[j]:
            a, b = find(i), find(j)
            parent[max(a, b)] = min(a, b)
    triples = [(int(i), int(j), float(v)) for (i, j), v in zip(edges, J)] + [(i, i, float(h[i])) for i in range(n)]
    out = []
    for r in range(n):
        if D[r] and find(r) == r:
            C = np.array([D[i] and find(i) == r for i in range(n)])
            out.append((r, int(C.sum()), float(energy_Jij(triples, np.where(C, 1 - g, g)[None, :])[0] - energy_Jij(triples, g[None, :])[0])))
    return out


# ---------------------------------------------------------------------------------------------- the public call from J0 alone
def model_graph(solver):
    """(act, rowptr, cols, vals, field) of an Ising solver from solver.J0 and solver.ind0: the graph over the active spins in model order."""
    J0 = np.asarray(solver.J0, dtype=np.float64)
    act = np.sort(np.concatenate([np.asarray(a, dtype=np.int64) for row in solver.ind0 for a in row]))
    pos = {int(v): k for k, v in enumerate(act)}
    links = [(i, j) for i in range(J0.shape[0]) for j in range(i + 1, J0.shape[0]) if J0[i, j] != 0]
    rowptr, cols, vals = wcsr(act.size, [(pos[i], pos[j]) for i, j in links], [J0[i, j] for i, j in links])
    return act, rowptr, cols, vals, J0.diagonal()[act].copy()


def public_reference(solver, bits, ref_bits, K):
    """What calculate_droplets stores for the states with the bits `bits` (M, L) and the reference ref_bits (L,), rows of binary_states():
    run()'s dict with the roots as model spins and the labels as (M, L)."""
    act, rowptr, cols, vals, field = model_graph(solver)
    pack = lambda b: np.array([xr.row_words(sum(int(v) << k for k, v in enumerate(r)), -(-act.size // 64)) for r in b], dtype=np.uint64)
    out = run(pack(np.asarray(bits)[:, act]), pack(np.asarray(ref_bits)[None, act])[0], act.size, rowptr, cols, vals, field, K)
    out['root'] = np.where(out['root'] >= 0, act[np.maximum(out['root'], 0)], -1)
    labels = np.full((len(bits), len(ref_bits)), -1, dtype=np.int32)
    labels[:, act] = out['labels']
    out['labels'] = labels
    return out
