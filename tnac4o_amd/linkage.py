"""Driver of tnac4o.calculate_state_linkage: single-linkage clusters of configurations by Hamming distance, with the library's
tn_state_linkage (csrc/linkage.hip).

Rows.  A state is a row of n bits (kind 'spin': the active spins in model order, d(a, b) = popcount(a XOR b)) or of n cell states
(kind 'cell': d = the number of cells that differ).  Fold (symmetric, 'spin' only): d'(a, b) = min(d, n - d), so that a state and its
global spin flip are the same point.  Edge order: key(a, b) = (d(a, b), min(a, b), max(a, b)), compared lexicographically, a strict
total order.  The tree is the unique minimum spanning tree of the complete graph on the M states under that order, its M - 1 edges in
ascending key order; cut at height t it gives the connected components of "differ in at most t".  The nearest other state of a is the
b != a that minimises (d(a, b), b).

The device computes the edges and the nearest states; everything derived from the edges (labels at a threshold, cluster counts, the
scipy-format matrix, representatives) and every argument check is plain numpy and runs without a GPU."""
import numpy as np

from .overlap import active_spins, cell_states, pack_bits, pack_lanes16, spin_bits
from .sampler import check_states

MAX_ENTRIES = 65534              # spins or cells per state: a distance takes 16 bits of an edge's key (include/tnpeps.h)
MAX_STATES = 2 ** 24             # a state index takes 24 bits of an edge's key
KINDS = ('spin', 'cell')


# ---------------------------------------------------------------------------------------------- from the sorted edges, on the host
class _Forest:
    """Union-find over M points that keeps the smallest member of every set."""

    def __init__(self, M):
        self.parent = np.arange(M, dtype=np.int64)

    def find(self, a):
        p = self.parent
        r = a
        while p[r] != r:
            r = p[r]
        while p[a] != r:
            p[a], a = r, p[a]
        return r

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)
        return min(a, b)


def labels_at(pairs, dist, M, threshold):
    """Labels (M,) int64 of the clusters when all pairs at distance <= threshold are joined -- the components of the tree's edges with
    d <= threshold --, numbered by their ascending smallest member."""
    pairs, dist = np.asarray(pairs, dtype=np.int64).reshape(-1, 2), np.asarray(dist, dtype=np.int64)
    f = _Forest(M)
    for (a, b), d in zip(pairs.tolist(), dist.tolist()):
        if d <= threshold:
            f.union(a, b)
    roots = np.array([f.find(a) for a in range(M)], dtype=np.int64)     # the smallest member of the cluster of a
    firsts = np.unique(roots)
    return np.searchsorted(firsts, roots).astype(np.int64)


def cluster_counts(dist, M, n):
    """(n + 1,) int64: entry t = the number of clusters when all pairs at distance <= t are joined = M - #{edges with d <= t}."""
    dist = np.asarray(dist, dtype=np.int64)
    return M - np.cumsum(np.bincount(dist, minlength=n + 1)[:n + 1]).astype(np.int64)


def linkage_matrix(pairs, dist, M):
    """(M - 1, 4) float64 in the format of scipy.cluster.hierarchy.linkage, from the edges in ascending order: merge i joins the
    clusters that hold the two ends of edge i, creates cluster M + i and lists the smaller id first; columns: the two ids, the height,
    the size of the new cluster."""
    pairs, dist = np.asarray(pairs, dtype=np.int64).reshape(-1, 2), np.asarray(dist, dtype=np.int64)
    Z = np.zeros((max(M - 1, 0), 4), dtype=np.float64)
    f = _Forest(M)
    ident = np.arange(M, dtype=np.int64)                                # the cluster id of a set, kept at its root
    size = np.ones(M, dtype=np.int64)
    for i, ((a, b), d) in enumerate(zip(pairs.tolist(), dist.tolist())):
        ra, rb = f.find(a), f.find(b)
        if ra == rb:
            raise ValueError('edge %d closes a cycle: the edges are not a tree' % i)
        Z[i] = (min(ident[ra], ident[rb]), max(ident[ra], ident[rb]), d, size[ra] + size[rb])
        r = f.union(ra, rb)
        ident[r], size[r] = M + i, size[ra] + size[rb]
    return Z


def cluster_summary(labels, energy=None):
    """(sizes, first, representative, energy_min) of the clusters of `labels`: the members, the smallest member, and -- with one energy
    per state -- the member of lowest energy (the first on ties) and that energy; without, None and None."""
    labels = np.asarray(labels, dtype=np.int64)
    K = int(labels.max(initial=-1)) + 1
    sizes = np.bincount(labels, minlength=K).astype(np.int64)
    first = np.full(K, labels.size, dtype=np.int64)
    np.minimum.at(first, labels, np.arange(labels.size, dtype=np.int64))
    if energy is None:
        return sizes, first, None, None
    energy = np.asarray(energy, dtype=np.float64)
    order = np.lexsort((np.arange(labels.size), energy, labels))        # by cluster, then energy, then index
    rep = order[np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)] if K else np.zeros(0, dtype=np.int64)
    return sizes, first, rep.astype(np.int64), energy[rep]


# ---------------------------------------------------------------------------------------------- driver
def _stored(solver):
    st = getattr(solver, 'states', None)
    st = np.asarray(st) if st is not None else np.zeros(0)
    return st if st.ndim == 2 and st.shape[0] >= 1 else None


def check_arguments(solver, threshold, kind, symmetric, states):
    """Everything calculate_state_linkage can refuse before any device work.  Returns (kind, symmetric, packed rows (M, nwords) uint64, n,
    lanes16)."""
    if kind is None:
        kind = 'spin' if solver.mode == 'Ising' else 'cell'
    if kind not in KINDS:
        raise ValueError("kind must be 'spin', 'cell' or None")
    if kind == 'spin' and solver.mode != 'Ising':
        raise ValueError("kind 'spin' is defined for mode 'Ising' only")
    if symmetric is None:
        symmetric = bool(kind == 'spin' and not np.any(np.asarray(solver.J0).diagonal() != 0))
    if not isinstance(symmetric, (bool, np.bool_)):
        raise ValueError('symmetric must be True, False or None')
    if symmetric and kind != 'spin':
        raise ValueError("symmetric folds the Hamming distance of spins: it is defined for kind 'spin' only")
    if threshold is not None and (isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, np.integer)) or threshold < 0):
        raise ValueError('threshold must be None or an integer >= 0')
    if states is None:
        if _stored(solver) is None:
            raise ValueError('calculate_state_linkage needs stored states (run sample_boltzmann, gibbs_sampling, a search or '
                             'decode_low_energy_states first) or states=')
        given = None
    else:
        given = check_states(states, solver._cell_sizes()[solver.order])
    if kind == 'cell':
        st = cell_states(solver) if given is None else given
        n, M = int(st.shape[1]), int(st.shape[0])
    else:
        n, M = int(active_spins(solver).size), int((_stored(solver) if given is None else given).shape[0])
    if n < 1:
        raise ValueError("kind '%s': the model has nothing to compare" % kind)
    if n > MAX_ENTRIES:
        raise NotImplementedError("kind '%s' compares %d %s per state; tn_state_linkage takes at most %d; there is no host fallback"
                                  % (kind, n, 'cells' if kind == 'cell' else 'spins', MAX_ENTRIES))
    if M > MAX_STATES:
        raise NotImplementedError('%d states; tn_state_linkage takes at most 2^24 = %d; there is no host fallback' % (M, MAX_STATES))
    if kind == 'cell':
        if st.size and int(st.max()) >= 32768:
            raise NotImplementedError('a cell has more than 32768 states; tn_state_linkage compares 16-bit lanes')
        return kind, bool(symmetric), pack_lanes16(st), n, True
    if given is None:
        bits = spin_bits(solver)
    else:
        from .droplets_of_states import state_bits
        bits = state_bits(solver, given)
    return kind, bool(symmetric), pack_bits(bits), n, False


def linkage_native(rows, n, lanes16, fold):
    """tn_state_linkage on packed rows (M, nwords) uint64: (pairs (M - 1, 2) int64, dist (M - 1,) int64, nearest (M,) int64, nearest
    distance (M,) int64, rounds)."""
    import torch
    from . import ops
    dev = torch.device('cuda', torch.cuda.current_device())
    got = ops.state_linkage(torch.as_tensor(np.ascontiguousarray(rows).view(np.int64)).to(dev), n, lanes16, fold)
    host = {k: v.cpu().numpy().astype(np.int64) for k, v in got.items()}
    return np.stack([host['edge_lo'], host['edge_hi']], axis=1), host['edge_dist'], host['nn_index'], host['nn_dist'], int(host['rounds'][0])


def store(solver, kind, symmetric, n, pairs, dist, nearest, nearest_dist, rounds, threshold, per_state_energy):
    """The attributes of calculate_state_linkage from the edges (host only)."""
    M = int(nearest.shape[0])
    solver.linkage_pairs, solver.linkage_distance = pairs, dist
    solver.nearest_state, solver.nearest_distance = nearest, nearest_dist
    solver.linkage_cluster_counts = cluster_counts(dist, M, n)
    solver.linkage_matrix = linkage_matrix(pairs, dist, M)
    solver.linkage_kind, solver.linkage_symmetric, solver.linkage_rounds = kind, symmetric, rounds
    solver.state_cluster_labels = solver.state_cluster_sizes = solver.state_cluster_first = None
    solver.state_cluster_representative = solver.state_cluster_energy_min = None
    if threshold is not None:
        labels = labels_at(pairs, dist, M, int(threshold))
        sizes, first, rep, emin = cluster_summary(labels, per_state_energy)
        solver.state_cluster_labels, solver.state_cluster_sizes, solver.state_cluster_first = labels, sizes, first
        solver.state_cluster_representative, solver.state_cluster_energy_min = rep, emin
    return solver.linkage_distance


def state_linkage(solver, threshold=None, kind=None, symmetric=None, states=None):
    """calculate_state_linkage of tnac4o (documented there)."""
    kind, symmetric, rows, n, lanes16 = check_arguments(solver, threshold, kind, symmetric, states)
    M = int(rows.shape[0])
    E = getattr(solver, 'energy', None)
    E = np.asarray(E, dtype=np.float64) if E is not None else np.zeros(0)
    per_state_energy = E if E.shape == (M,) and not np.any(np.isnan(E)) else None       # (with states=: of the GIVEN states when it has M entries)
    pairs, dist, nearest, nearest_dist, rounds = linkage_native(rows, n, lanes16, symmetric)
    return store(solver, kind, symmetric, n, pairs, dist, nearest, nearest_dist, rounds, threshold, per_state_energy)
