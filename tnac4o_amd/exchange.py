"""Driver of tnac4o.exchange_clusters: isoenergetic cluster moves (Houdayer's move in its form for arbitrary graphs: Zhu, Ochoa,
Katzgraber) on pairs of the stored configurations with the library's tn_cluster_exchange (csrc/exchange.hip).

For two replicas a, b the spins in which they differ (q_i = s_i^a s_i^b = -1) form a subgraph of the coupling graph; one of them is picked
at random, and the connected cluster of differing spins around it is flipped in BOTH replicas.  A coupling inside the cluster or
outside it keeps its energy in each replica; across the border of the cluster one end differs and the other does not, so what replica a
gains there replica b loses, and a field term of a cluster spin moves from one replica to the other: E_a + E_b is conserved.  The set
of differing spins is the same after the move, so the move is its own inverse, picked with the same probability: it leaves the product
law pi x pi of two replicas at one temperature invariant, without a rejection.

The host part (the bits of the states, the coupling graph as a CSR, the pairings, every argument check) is plain numpy and runs
without a GPU."""
import numpy as np

from .overlap import MAX_SPIN_BITS, _ising, active_spins, link_pairs, pack_bits, spin_bits


def coupling_csr(solver):
    """The coupling graph of an Ising model over the bits of spin_bits(solver): (rowptr (n + 1,), cols (nnz,)) int32, vertex k = active
    spin k in model order, every coupling of link_pairs(solver.J0) listed in both directions, the neighbours of a vertex ascending.  A
    coupling that touches a spin outside the cells is a ValueError."""
    _ising(solver, 'coupling_csr')
    act = active_spins(solver)
    n = int(act.size)
    links = link_pairs(solver.J0)
    pos = np.full(int(np.asarray(solver.J0).shape[0]), -1, dtype=np.int64)
    pos[act] = np.arange(n)
    ends = pos[links]                                                    # (nlinks, 2) positions, -1 = inactive
    if ends.size and ends.min() < 0:
        i, j = links[np.argwhere(ends.min(axis=1) < 0)[0, 0]]
        raise ValueError('the coupling (%d, %d) touches a spin that no cell lists' % (i, j))
    src = np.concatenate([ends[:, 0], ends[:, 1]])
    dst = np.concatenate([ends[:, 1], ends[:, 0]])
    order = np.lexsort((dst, src))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=rowptr[1:])
    return rowptr.astype(np.int32), dst[order].astype(np.int32)


def weighted_coupling_csr(solver):
    """coupling_csr with the numbers of the energy E(s) = sum_{i<j} J_ij s_i s_j + sum_i J_ii s_i of auxx.energy_Jij on it: (rowptr, cols,
    vals (nnz,) float64, field (n,) float64) -- vals[e] = the coupling J0[i, j], i < j, of the arc e, which both of its directions carry;
    field[k] = J0[i, i] of the active spin i at position k.  (tn_droplets reads them: droplets_of_states.py.)"""
    rowptr, cols = coupling_csr(solver)
    act = active_spins(solver)
    J0 = np.asarray(solver.J0, dtype=np.float64)
    a, b = act[np.repeat(np.arange(act.size), np.diff(rowptr))], act[cols]
    return rowptr, cols, np.ascontiguousarray(J0[np.minimum(a, b), np.maximum(a, b)]), np.ascontiguousarray(J0.diagonal()[act])


def check_pairs(pairs, rounds, M):
    """The pairings of `rounds` rounds over M rows: None -> for each round np.random.permutation(M)[:2 P].reshape(P, 2), P = M // 2, from
    numpy's global generator; else an integer numpy array (rounds, P, 2) with every entry in [0, M) and no index twice within a round.
    Returns them as int32 (rounds, P, 2); anything else: ValueError."""
    rounds, M = int(rounds), int(M)
    if pairs is None:
        P = M // 2
        return np.array([np.random.permutation(M)[:2 * P].reshape(P, 2) for _ in range(rounds)], dtype=np.int32).reshape(rounds, P, 2)
    if not isinstance(pairs, np.ndarray) or pairs.dtype.kind not in 'iu':
        raise ValueError('pairs must be None or an integer numpy array of shape (rounds, P, 2)')
    if pairs.ndim != 3 or pairs.shape[0] != rounds or pairs.shape[2] != 2:
        raise ValueError('pairs must have shape (rounds, P, 2) = (%d, P, 2), got %s' % (rounds, tuple(pairs.shape)))
    if pairs.size and (pairs.min() < 0 or pairs.max() >= M):
        raise ValueError('pairs: an index lies outside [0, %d), the stored states' % M)
    for k in range(rounds):
        if np.unique(pairs[k]).size != pairs[k].size:
            raise ValueError('pairs: an index appears twice in round %d (a state is in at most one pair of a round)' % k)
    return np.ascontiguousarray(pairs, dtype=np.int32)


def check_round_uniforms(uniforms, rounds, P):
    """The uniform numbers of the seeds: None -> np.random.rand(rounds, P) from numpy's global generator; else a (rounds, P) float64 numpy
    array or torch tensor of numbers in [0, 1), which is returned as it is.  Anything else: ValueError (the rules of
    sampler.check_uniforms)."""
    shape = (int(rounds), int(P))
    if uniforms is None:
        return np.random.rand(*shape)
    is_np = isinstance(uniforms, np.ndarray)
    if not is_np:
        import torch
        if not isinstance(uniforms, torch.Tensor):
            raise ValueError('uniforms must be None, a numpy array or a torch tensor (got %s)' % type(uniforms).__name__)
    if tuple(uniforms.shape) != shape:
        raise ValueError('uniforms must have shape (rounds, P) = %s, got %s' % (shape, tuple(uniforms.shape)))
    if is_np:
        if uniforms.dtype != np.float64:
            raise ValueError('uniforms must be float64, got %s' % uniforms.dtype)
        ok = bool(np.all((uniforms >= 0.0) & (uniforms < 1.0)))
    else:
        import torch
        if uniforms.dtype != torch.float64:
            raise ValueError('uniforms must be float64, got %s' % uniforms.dtype)
        ok = bool(((uniforms >= 0.0) & (uniforms < 1.0)).all().item())
    if not ok:                                            # (a NaN fails both comparisons)
        raise ValueError('uniforms must lie in [0, 1) (no NaN)')
    return uniforms


def check_arguments(solver, rounds, pairs, uniforms, seed=None):
    """Everything exchange_clusters can refuse before any device work.  Returns (rounds, pairs (rounds, P, 2) int32, uniforms (rounds, P));
    every pairing is drawn before any uniform.  With a seed (rng.check_seed; not together with uniforms) nothing is drawn from numpy's
    generator: pairs=None gives the pairings of the seed's keys, and the uniforms returned are None -- they are filled on the device."""
    from . import rng
    _ising(solver, 'exchange_clusters')
    if int(rounds) != rounds or rounds < 0:
        raise ValueError('rounds must be a non-negative integer')
    seed = rng.check_seed_alone(seed, uniforms)
    st = np.asarray(solver.states)
    M = int(st.shape[0]) if st.ndim == 2 else 0
    if M < 2:
        raise ValueError('exchange_clusters needs at least two stored states (run sample_boltzmann, gibbs_sampling, a search or '
                         'decode_low_energy_states first)')
    if seed is not None:
        pairs = rng.draw_pairs(seed, rng.EXCHANGE_PAIRING, int(rounds), M) if pairs is None else check_pairs(pairs, rounds, M)
        return int(rounds), pairs, None
    pairs = check_pairs(pairs, rounds, M)
    return int(rounds), pairs, check_round_uniforms(uniforms, rounds, pairs.shape[1])


def unpack_bits(rows, n):
    """(M, >= ceil(n / 64)) uint64 -> (M, n) uint8 of 0 / 1: the inverse of overlap.pack_bits."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    by = rows.astype('<u8').view(np.uint8).reshape(rows.shape[0], -1)
    return np.unpackbits(by, axis=1, bitorder='little')[:, :n]


def exchange_native(rows, nbits, rowptr, cols, pairs, uniforms, seed=None):
    """The device loop: rows (M, nwords) uint64 go up once, every round is one tn_cluster_exchange on them, they come back once.
    uniforms None and seed an integer: the (rounds, P) numbers are filled on the device (rng.EXCHANGE_SEED: row = round, index = pair).
    Returns (rows, cluster sizes (rounds, P) int64, differing bits (rounds, P) int64)."""
    import torch
    from . import ops, rng
    dev = torch.device('cuda', torch.cuda.current_device())
    rounds, P = pairs.shape[0], pairs.shape[1]
    d_rows = torch.as_tensor(np.ascontiguousarray(rows).view(np.int64)).to(dev)
    d_rowptr, d_cols = torch.as_tensor(rowptr).to(dev), torch.as_tensor(cols).to(dev)
    d_pairs = torch.as_tensor(pairs).to(dev)
    if seed is not None:
        d_u = rng.fill(seed, rng.EXCHANGE_SEED, 0, (rounds, P), dev=dev)
    else:
        d_u = (torch.as_tensor(uniforms) if isinstance(uniforms, np.ndarray) else uniforms).to(dev).contiguous()
    out = [ops.cluster_exchange(d_rows, nbits, d_rowptr, d_cols, d_pairs[k], d_u[k]) for k in range(rounds)]
    sizes = np.array([s.cpu().numpy() for s, _ in out], dtype=np.int64).reshape(rounds, P)
    diff = np.array([d.cpu().numpy() for _, d in out], dtype=np.int64).reshape(rounds, P)
    return d_rows.cpu().numpy().view(np.uint64), sizes, diff


def exchange_clusters(solver, rounds=1, pairs=None, uniforms=None, seed=None):
    """exchange_clusters of tnac4o (documented there)."""
    from .rng import check_seed
    rounds, pairs, uniforms = check_arguments(solver, rounds, pairs, uniforms, seed)
    seed = check_seed(seed)
    act = active_spins(solver)
    n = int(act.size)
    if n < 1:
        raise ValueError('the model has no active spin')
    if n > MAX_SPIN_BITS:
        raise NotImplementedError('the model has %d active spins; tn_cluster_exchange takes at most %d; there is no host fallback' % (n, MAX_SPIN_BITS))
    rowptr, cols = coupling_csr(solver)
    old = np.asarray(solver.states)
    M = old.shape[0]
    rows, sizes, diff = exchange_native(pack_bits(spin_bits(solver)), n, rowptr, cols, pairs, uniforms, seed)
    bits = np.zeros((M, int(solver.L)), dtype=np.int8)
    bits[:, act] = unpack_bits(rows, n)
    new = solver.states_from_binary(bits)
    # the energies before and after, in the bits relax_samples and scored_energy produce: no sweep, one call over both sets
    from . import relax, sampler
    both = np.concatenate([sampler.check_states(old, solver._cell_sizes()[solver.order]), new])
    rot = np.empty_like(both)
    rot[:, solver.order] = both                                         # the inverse of _store_result's states[:, order]
    energy = relax.relax_native(solver, rot, 1, float(solver.beta), 0)[1]
    solver.states = new
    solver.energy, solver.exchange_energy_before = energy[M:].copy(), energy[:M].copy()
    solver.exchange_pairs = pairs.astype(np.int64)
    solver.exchange_cluster_sizes, solver.exchange_differing = sizes, diff
    solver.probability = solver.sample_log2Z = solver.log2Z_lower = solver.log2Z_estimate = None
    return sizes
