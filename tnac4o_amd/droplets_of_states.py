"""Driver of tnac4o.calculate_droplets: the droplets of configurations relative to a reference state, with the library's tn_droplets
(csrc/droplets.hip).  (The droplets the branch-and-bound search keeps are another matter: droplets.py.)

For a state x and a reference g the spins in which they differ, D = x XOR g, form a subgraph of the coupling graph; its connected
components are the droplets of x, numbered by ascending root (the smallest spin of a droplet).  The excitation energy of a droplet C
is dE_C = E(g with C flipped) - E(g) = -2 (sum_{i in C, j not in C} J_ij g_i g_j + sum_{i in C} J_ii g_i) in the convention of
auxx.energy_Jij.  A neighbour of C that lies in D is in C, so every coupling that leaves C ends outside D and a coupling between two
droplets does not exist: the droplets flip independently, sum_C dE_C = E(x) - E(g).

The host part (the bits of the states and of the reference, the weighted CSR, every argument check) is plain numpy and runs without a
GPU."""
import numpy as np

from .exchange import weighted_coupling_csr
from .overlap import MAX_SPIN_BITS, _ising, active_spins, pack_bits, spin_bits
from .sampler import check_states, chunk_slices, plan_chunk


def state_bits(solver, states):
    """binary_states() of the configurations `states` ((M, Nx*Ny) int64 in model cell order, every entry inside its cell) restricted to
    the active spins, in model order: (M, n) uint8 of 0 / 1 -- spin_bits for states that are not the stored ones."""
    from .tnac4o import _bits
    out = np.zeros((states.shape[0], int(solver.L)), dtype=np.uint8)
    k = -1
    for ny in range(solver.Ny_model):
        for nx in range(solver.Nx_model):
            k += 1
            act = solver.ind0[ny][nx]
            out[:, act] = (1 - _bits(len(act)))[states[:, k]]
    return out[:, active_spins(solver)]


def reference_energy(J0, bits):
    """E(s) = sum_{i<j} J0[i, j] s_i s_j + sum_i J0[i, i] s_i with s = 2 bits - 1: auxx.energy_Jij's formula on the dense upper triangle."""
    J0 = np.asarray(J0, dtype=np.float64)
    s = 2.0 * np.asarray(bits, dtype=np.float64) - 1.0
    return float(np.sum((s @ np.triu(J0, 1)) * s) + s @ J0.diagonal())


def _stored(solver):
    st = getattr(solver, 'states', None)
    st = np.asarray(st) if st is not None else np.zeros(0)
    return st if st.ndim == 2 and st.shape[0] >= 1 else None


def check_reference(solver, reference):
    """The reference as (L,) uint8 bits of 0 / 1 (0 at the inactive spins): None -> the stored state of lowest solver.energy, the first
    on ties; an integer -> that stored state; an integer array of length L -> 0 / 1 at every active spin, the form of a row of
    binary_states() (what the inactive spins hold is ignored).  Anything else: ValueError."""
    L = int(solver.L)
    act = active_spins(solver)
    if reference is None or (isinstance(reference, (int, np.integer)) and not isinstance(reference, (bool, np.bool_))):
        st = _stored(solver)
        if st is None:
            raise ValueError('reference: there are no stored states to take it from (run sample_boltzmann, gibbs_sampling, a search or '
                             'decode_low_energy_states first, or give the reference as bits)')
        if reference is None:
            E = getattr(solver, 'energy', None)
            E = np.asarray(E, dtype=np.float64) if E is not None else np.zeros(0)
            if E.shape != (st.shape[0],) or np.all(np.isnan(E)):
                raise ValueError('reference=None takes the stored state of lowest energy: there is no energy for each of the %d stored states'
                                 % st.shape[0])
            reference = int(np.nanargmin(E))
        if not 0 <= int(reference) < st.shape[0]:
            raise ValueError('reference: the index %d lies outside [0, %d), the stored states' % (int(reference), st.shape[0]))
        bits = np.zeros(L, dtype=np.uint8)
        bits[act] = spin_bits(solver)[int(reference)]
        return bits
    if not isinstance(reference, np.ndarray) or reference.dtype.kind not in 'iub':
        raise ValueError('reference must be None, an index into the stored states or an integer numpy array of %d bits' % L)
    if reference.shape != (L,):
        raise ValueError('reference: bits of shape (L,) = (%d,) expected, got %s' % (L, tuple(reference.shape)))
    b = reference[act].astype(np.int64)
    if np.any((b != 0) & (b != 1)):
        raise ValueError('reference: the bit of an active spin is neither 0 nor 1')
    bits = np.zeros(L, dtype=np.uint8)
    bits[act] = b
    return bits


def check_arguments(solver, reference, max_droplets, labels, states, chunk):
    """Everything calculate_droplets can refuse before any device work.  Returns (reference bits (L,) uint8, the bits of the states (M, n)
    uint8 over the active spins, K)."""
    _ising(solver, 'calculate_droplets')
    if isinstance(max_droplets, (bool, np.bool_)) or not isinstance(max_droplets, (int, np.integer)) or not 0 <= max_droplets < 2 ** 31:
        raise ValueError('max_droplets must be an integer in [0, 2^31)')
    if not isinstance(labels, (bool, np.bool_)):
        raise ValueError('labels must be True or False')
    if chunk is not None:
        chunk_slices(1, chunk)
    if states is None:
        if _stored(solver) is None:
            raise ValueError('calculate_droplets needs stored states (run sample_boltzmann, gibbs_sampling, a search or '
                             'decode_low_energy_states first) or states=')
        bits = None
    else:
        bits = state_bits(solver, check_states(states, solver._cell_sizes()[solver.order]))
    ref = check_reference(solver, reference)
    return ref, spin_bits(solver) if bits is None else bits, int(max_droplets)


def droplets_native(rows, ref_row, nbits, rowptr, cols, vals, field, K, labels=False, chunk=None):
    """tn_droplets over the packed rows (M, nwords) uint64 in row slices of at most `chunk` (None: what fits half of the free device
    memory, sampler.plan_chunk); the graph and the reference go up once, the size counts accumulate on the device over the slices.
    Returns a dict of numpy arrays: count, diff, largest (M,) int64, de_total (M,), root, size (M, K) int64, de (M, K), size_hist
    (nbits + 1,) int64, labels (M, nbits) int32 or None."""
    import torch
    from . import ops
    dev = torch.device('cuda', torch.cuda.current_device())
    M, nwords = int(rows.shape[0]), -(-nbits // 64)
    if chunk is not None:
        chunk_slices(M, chunk)                            # (validates chunk before any device work)
    else:
        chunk = plan_chunk(M, lambda m: m * (nwords * 8 + 20 + K * 16 + (nbits * 4 if labels else 0)), torch.cuda.mem_get_info(dev)[0] // 2)
    d_ref = torch.as_tensor(np.ascontiguousarray(ref_row).view(np.int64)).to(dev)
    d_rowptr, d_cols, d_vals, d_field = (torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in (rowptr, cols, vals, field))
    d_hist = torch.zeros(nbits + 1, dtype=torch.int64, device=dev)
    out = dict(count=np.empty(M, dtype=np.int64), diff=np.empty(M, dtype=np.int64), largest=np.empty(M, dtype=np.int64), de_total=np.empty(M),
               root=np.empty((M, K), dtype=np.int64), size=np.empty((M, K), dtype=np.int64), de=np.empty((M, K)),
               labels=np.empty((M, nbits), dtype=np.int32) if labels else None)
    rows = np.ascontiguousarray(rows).view(np.int64)
    for lo, hi in chunk_slices(M, chunk):
        got = ops.droplets(torch.as_tensor(rows[lo:hi]).to(dev), nbits, d_ref, d_rowptr, d_cols, d_vals, d_field, K, d_hist, labels)
        for k, v in out.items():
            if v is not None:
                v[lo:hi] = got[k].cpu().numpy()
    out['size_hist'] = d_hist.cpu().numpy()
    return out


def droplets_of_states(solver, reference=None, max_droplets=64, labels=False, states=None, chunk=None):
    """calculate_droplets of tnac4o (documented there)."""
    ref, bits, K = check_arguments(solver, reference, max_droplets, labels, states, chunk)
    act = active_spins(solver)
    n, M = int(act.size), int(bits.shape[0])
    if n < 1:
        raise ValueError('the model has no active spin')
    if n > MAX_SPIN_BITS:
        raise NotImplementedError('the model has %d active spins; tn_droplets takes at most %d; there is no host fallback' % (n, MAX_SPIN_BITS))
    rowptr, cols, vals, field = weighted_coupling_csr(solver)
    out = droplets_native(pack_bits(bits), pack_bits(ref[act][None, :])[0], n, rowptr, cols, vals, field, K, bool(labels), chunk)
    solver.droplet_count = out['count']
    solver.droplet_hamming, solver.droplet_largest, solver.droplet_energy_total = out['diff'], out['largest'], out['de_total']
    solver.droplet_roots = np.where(out['root'] >= 0, act[np.maximum(out['root'], 0)], -1)
    solver.droplet_sizes, solver.droplet_energies = out['size'], out['de']
    solver.droplet_size_counts = out['size_hist']
    solver.droplet_truncated = np.flatnonzero(out['count'] > K)
    solver.droplet_reference = ref
    solver.droplet_reference_energy = reference_energy(solver.J0, ref)
    solver.droplet_labels = None
    if labels:
        solver.droplet_labels = np.full((M, int(solver.L)), -1, dtype=np.int32)
        solver.droplet_labels[:, act] = out['labels']
    return solver.droplet_count
