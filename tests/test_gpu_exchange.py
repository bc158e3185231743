"""tn_cluster_exchange and tnac4o.exchange_clusters on the GPU against the reference of tests/exchange_ref.py.  Every comparison is exact:
the move has no rounding in it.  The kernel on the shared cases (word edges, the last one-wave row and the first workgroup row; paths
that need nbits - 1 growth steps, a gap, a star, cliques, isolated spins, one-way arcs, neighbours and arc ranges out of range, uniforms
whose products are integers; poisoned padding and bits beyond nbits), the pairs (none, a == b, indices out of range, an unpaired row),
slicing, the invariants of the move from the device's own output, and the public call on the small Ising solvers."""
import ctypes as ct

import numpy as np
import pytest

import exchange_ref as xr
import golden_inputs as gi
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_sampling import droplet, dv, small      # noqa: E402  (helpers only, no test is imported)

CASE_IDS = ['%s-%d' % c for c in xr.CASES]
CHIMERA = ('chimera', 128)


# ---------------------------------------------------------------------------------------------- helpers
def _last_error():
    from tnac4o_amd import _lib
    buf = ct.create_string_buffer(512)
    _lib.lib().tn_last_error(buf, 512)
    return buf.value.decode()


def _framed(dtype, array, seed):
    """A numpy array on the device between guards."""
    array = np.ascontiguousarray(array)
    g = Guarded.of(dtype, array.shape, 0x55, seed=seed)
    if array.size:
        g.tensor().copy_(dv(array))
    return g


def exchange_device(rows, nbits, rowptr, cols, pairs, uniforms, M=None, want_rc=0):
    """One call of tn_cluster_exchange with every buffer between guards: (rows (M, ld) uint64, size_out, diff_out (P,) int64).  The
    outputs start as 0x55 bytes: an entry the call left alone shows."""
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    P = pairs.shape[0]
    g_rows = _framed(torch.int64, rows.view(np.int64), 1)
    g_ptr, g_cols = _framed(torch.int32, np.asarray(rowptr, dtype=np.int32), 2), _framed(torch.int32, np.asarray(cols, dtype=np.int32), 3)
    g_pairs, g_u = _framed(torch.int32, pairs, 4), _framed(torch.float64, np.asarray(uniforms, dtype=np.float64).reshape(P), 5)
    g_size, g_diff = Guarded.of(torch.int32, (P,), 0x55, seed=6), Guarded.of(torch.int32, (P,), 0x55, seed=7)
    rc = L.tn_cluster_exchange(g_rows.ptr, rows.shape[0] if M is None else M, nbits, rows.shape[1], g_ptr.ptr, g_cols.ptr, len(cols), g_pairs.ptr, P,
                               g_u.ptr, g_size.ptr, g_diff.ptr, ops._stream())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _last_error())
    for g in (g_rows, g_ptr, g_cols, g_pairs, g_u, g_size, g_diff):
        assert g.intact()
    return g_rows.host().view(np.uint64), g_size.host().astype(np.int64), g_diff.host().astype(np.int64)


def run_case(c, **kw):
    args = dict(rows=c['rows'], nbits=c['nbits'], rowptr=c['rowptr'], cols=c['cols'], pairs=c['pairs'], uniforms=c['uniforms'])
    args.update(kw)
    return exchange_device(**args)


def masks_of(rows, nbits):
    nwords = -(-nbits // 64)
    return [xr.row_int(r[:nwords]) & ((1 << nbits) - 1) for r in rows]


# ---------------------------------------------------------------------------------------------- 1. kernel against the reference
@pytest.mark.parametrize('case', xr.CASES, ids=CASE_IDS)
def test_kernel_against_the_reference(case):
    """Rows (padding and the bits beyond nbits included), size_out and diff_out equal the reference's; and from the device's own output,
    for every pair: the differing bits are the same set as before and diff_out counts them, the flipped cluster is the same in both rows,
    lies inside them and has size_out bits, and the same call with the seed forced into the cluster restores the input."""
    c = xr.case_inputs(case)
    n = c['nbits']
    rows, size, diff = run_case(c)
    ref_rows, ref_size, ref_diff = xr.case_reference(case)
    assert np.array_equal(size, ref_size) and np.array_equal(diff, ref_diff)
    assert np.array_equal(rows, ref_rows)
    old, new = masks_of(c['rows'], n), masks_of(rows, n)
    symmetric = case[0] not in ('one-way', 'bad-neighbour', 'bad-rowptr')      # (with one-way arcs only the SAME seed finds the cluster again)
    back = np.array(c['uniforms'])
    for p, (a, b) in enumerate(c['pairs']):
        D, C = old[a] ^ old[b], old[a] ^ new[a]
        assert new[a] ^ new[b] == D and bin(D).count('1') == diff[p]
        assert old[b] ^ new[b] == C and C & ~D == 0 and bin(C).count('1') == size[p]
        assert (size[p] == 0) == (diff[p] == 0)
        if C and symmetric:                                             # the lowest bit of the cluster as the seed
            low = (C & -C).bit_length() - 1
            back[p] = (bin(D & ((1 << low) - 1)).count('1') + 0.5) / diff[p]
    again, size2, diff2 = run_case(c, rows=rows, uniforms=back)
    assert np.array_equal(again, c['rows']) and np.array_equal(size2, size) and np.array_equal(diff2, diff)


# ---------------------------------------------------------------------------------------------- 2. the pairs
def test_no_pair_is_a_no_op():
    c = xr.case_inputs(CHIMERA)
    rows, size, diff = run_case(c, pairs=np.zeros((0, 2), dtype=np.int32), uniforms=np.zeros(0))
    assert np.array_equal(rows, c['rows']) and size.size == 0 and diff.size == 0


def test_pairs_that_move_nothing_and_the_unpaired_row():
    """a == b, equal rows, an index of -1 and of M (-1 in both outputs, nothing touched), among pairs that move; 65 rows: the last has
    no partner and is bit-identical afterwards."""
    c = xr.case_inputs(CHIMERA)
    rng = np.random.default_rng(3)
    rows = np.concatenate([c['rows'], xr.random_rows(1, 128, rng)])
    rows[11, :2] = rows[10, :2]                                         # equal rows (their padding differs)
    M = rows.shape[0]
    pairs = np.array([[0, 1], [2, 2], [3, -1], [M, 4], [-1, M], [5, 6], [10, 11], [2 ** 31 - 1, 7], [8, -2 ** 31], [12, 13]], dtype=np.int32)
    u = rng.random(len(pairs))
    got_rows, size, diff = exchange_device(rows, 128, c['rowptr'], c['cols'], pairs, u)
    ref_rows, ref_size, ref_diff = xr.run(rows, 128, c['rowptr'], c['cols'], pairs, u)
    assert np.array_equal(size, ref_size) and np.array_equal(diff, ref_diff) and np.array_equal(got_rows, ref_rows)
    assert size.tolist()[1:5] == [0, -1, -1, -1] and diff.tolist()[1:5] == [0, -1, -1, -1]
    assert size[6] == 0 and diff[6] == 0 and list(size[7:9]) == [-1, -1] and size[0] > 0 and size[5] > 0 and size[9] > 0
    moved = [0, 1, 5, 6, 12, 13]
    still = [k for k in range(M) if k not in moved]
    assert np.array_equal(got_rows[still], rows[still]) and not np.array_equal(got_rows[moved], rows[moved])
    # M below the rows that are there: indices at and beyond it are outside
    _, size, diff = exchange_device(rows, 128, c['rowptr'], c['cols'], np.array([[0, 1], [2, 20]], dtype=np.int32), u[:2], M=20)
    assert size[1] == -1 and diff[1] == -1 and size[0] == ref_size[0]


# ---------------------------------------------------------------------------------------------- 3. slicing
@pytest.mark.parametrize('case', [CHIMERA, ('random', 130), ('random', 4097)], ids=['chimera-128', 'random-130', 'random-4097'])
def test_slicing(case):
    """The same pairs in one call, in two calls and in reversed order: the same bits."""
    c = xr.case_inputs(case)
    whole = run_case(c)
    ref = xr.case_reference(case)
    assert all(np.array_equal(x, y) for x, y in zip(whole, ref))
    P = len(c['pairs'])
    h = P // 2 + 1
    first = run_case(c, pairs=c['pairs'][:h], uniforms=c['uniforms'][:h])
    second = run_case(c, rows=first[0], pairs=c['pairs'][h:], uniforms=c['uniforms'][h:])
    assert np.array_equal(second[0], whole[0])
    assert np.array_equal(np.concatenate([first[1], second[1]]), whole[1]) and np.array_equal(np.concatenate([first[2], second[2]]), whole[2])
    rev = run_case(c, pairs=c['pairs'][::-1], uniforms=c['uniforms'][::-1])
    assert np.array_equal(rev[0], whole[0]) and np.array_equal(rev[1][::-1], whole[1]) and np.array_equal(rev[2][::-1], whole[2])
    swapped = run_case(c, pairs=c['pairs'][:, ::-1])                    # (b, a) for (a, b)
    assert all(np.array_equal(x, y) for x, y in zip(swapped, whole))


def test_wrapper():
    """ops.cluster_exchange on plain device tensors, rows with a stride; its refusals."""
    from tnac4o_amd import ops
    c = xr.case_inputs(CHIMERA)
    d_rows = dv(c['rows'].view(np.int64))
    size, diff = ops.cluster_exchange(d_rows, 128, dv(c['rowptr']), dv(c['cols']), dv(c['pairs']), dv(c['uniforms']))
    ref = xr.case_reference(CHIMERA)
    assert size.dtype == torch.int32 and diff.dtype == torch.int32
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64), ref[0]) and np.array_equal(size.cpu().numpy(), ref[1]) and np.array_equal(diff.cpu().numpy(), ref[2])
    size, diff = ops.cluster_exchange(d_rows, 128, dv(c['rowptr']), dv(c['cols']), dv(np.zeros((0, 2), dtype=np.int32)), dv(np.zeros(0)))
    assert size.numel() == 0 and diff.numel() == 0
    with pytest.raises(RuntimeError):
        ops.cluster_exchange(d_rows.cpu(), 128, dv(c['rowptr']), dv(c['cols']), dv(c['pairs']), dv(c['uniforms']))
    with pytest.raises(TypeError):
        ops.cluster_exchange(d_rows, 128, dv(c['rowptr'][:-1]), dv(c['cols']), dv(c['pairs']), dv(c['uniforms']))
    with pytest.raises(TypeError):
        ops.cluster_exchange(d_rows, 128, dv(c['rowptr']), dv(c['cols']), dv(c['pairs'].astype(np.int64)), dv(c['uniforms']))
    with pytest.raises(TypeError):
        ops.cluster_exchange(d_rows, 128, dv(c['rowptr']), dv(c['cols']), dv(c['pairs']), dv(c['uniforms'][:-1]))
    with pytest.raises(ValueError):
        ops.cluster_exchange(d_rows, 64 * d_rows.shape[1] + 1, dv(c['rowptr']), dv(c['cols']), dv(c['pairs']), dv(c['uniforms']))


# ---------------------------------------------------------------------------------------------- 4. the public call
def make(name):
    if name.startswith('droplet'):
        return droplet(int(name[-1]), beta=1.0)
    if name == 'j124':
        import tnac4o_amd
        return tnac4o_amd.tnac4o(mode='Ising', Nx=8, Ny=8, Nc=8, J=gi.j124_J(1), beta=1.0)
    return small(name, 1.0)


def random_states(ins, M, seed):
    qs = ins._cell_sizes()[ins.order]                                    # model order
    return np.random.default_rng(seed).integers(0, qs[None, :], size=(M, qs.size))


def reference_call(ins, pairs, uniforms):
    """(states, sizes, differing) of exchange_clusters on ins.states from the reference, round by round on the packed spin bits."""
    from tnac4o_amd import exchange as ex
    from tnac4o_amd import overlap as ov
    act = ov.active_spins(ins)
    rowptr, cols = ex.coupling_csr(ins)
    rows = ov.pack_bits(ov.spin_bits(ins))
    sizes, differing = [], []
    for k in range(len(pairs)):
        rows, s, d = xr.run(rows, act.size, rowptr, cols, pairs[k], uniforms[k])
        sizes.append(s)
        differing.append(d)
    bits = np.zeros((rows.shape[0], ins.L), dtype=np.int8)
    bits[:, act] = ex.unpack_bits(rows, act.size)
    return ins.states_from_binary(bits), np.array(sizes), np.array(differing)


def energies_of(name, states):
    other = make(name)
    return other.relax_samples(sweeps=0, mode='quench', states=states)


@pytest.mark.parametrize('name', ['ising3x3', 'chimera2x2', 'droplet0', 'droplet1'])
def test_public_call(name):
    """33 random states, two rounds with given pairs and uniforms: the reference's states, cluster sizes and distances; the energies
    in the bits of relax_samples(sweeps=0, mode='quench'); what is stored and what is left alone; uniforms on the device and the
    other rotation give the same result."""
    from tnac4o_amd import overlap as ov
    ins = make(name)                                                     # a fresh solver: no contraction has run
    M, P = 33, 16
    ins.states = random_states(ins, M, 21)
    start = np.copy(ins.states)
    rng = np.random.default_rng(22)
    pairs = np.array([rng.permutation(M)[:2 * P].reshape(P, 2) for _ in range(2)])
    u = rng.random((2, P))
    want_states, want_sizes, want_diff = reference_call(ins, pairs, u)
    bits = ov.spin_bits(ins).astype(np.int64)
    hamming = np.array([np.count_nonzero(bits[a] != bits[b]) for a, b in pairs[0]])
    ins.degeneracy = 5
    ins.probability = np.zeros(M)
    sizes = ins.exchange_clusters(rounds=2, pairs=pairs, uniforms=u)
    assert not hasattr(ins, 'rhoT') and ins.degeneracy == 5
    assert sizes is ins.exchange_cluster_sizes and sizes.shape == (2, P) and np.array_equal(sizes, want_sizes)
    assert np.array_equal(ins.exchange_differing, want_diff) and np.array_equal(ins.exchange_differing[0], hamming)
    assert np.array_equal(ins.exchange_pairs, pairs)
    assert np.array_equal(ins.states, want_states) and not np.array_equal(ins.states, start)
    assert same_bits(ins.energy, energies_of(name, ins.states)) and same_bits(ins.exchange_energy_before, energies_of(name, start))
    assert ins.probability is None and ins.sample_log2Z is None and ins.log2Z_lower is None and ins.log2Z_estimate is None
    unpaired = [k for k in range(M) if k not in pairs[0] and k not in pairs[1]]
    assert np.array_equal(ins.states[unpaired], start[unpaired])
    other = make('droplet1' if name == 'droplet0' else name)            # (the droplet: in the other rotation)
    other.states = np.copy(start)
    other.exchange_clusters(rounds=2, pairs=pairs, uniforms=torch.as_tensor(u).cuda())
    assert np.array_equal(other.states, ins.states) and np.array_equal(other.exchange_cluster_sizes, sizes)
    if name != 'droplet0':
        assert same_bits(other.energy, ins.energy)
    # no round: nothing moves, the energies are there
    ins.exchange_clusters(rounds=0)
    assert np.array_equal(ins.states, want_states) and ins.exchange_cluster_sizes.shape == (0, P) and same_bits(ins.energy, ins.exchange_energy_before)


def test_public_call_draws_from_the_global_generator():
    ins = make('droplet0')
    ins.states = random_states(ins, 12, 5)
    start = np.copy(ins.states)
    np.random.seed(17)
    ins.exchange_clusters(rounds=3)
    np.random.seed(17)
    pairs = np.array([np.random.permutation(12).reshape(6, 2) for _ in range(3)])
    u = np.random.rand(3, 6)
    assert np.array_equal(ins.exchange_pairs, pairs)
    other = make('droplet0')
    other.states = start.astype(other.indtype)                          # (as the searches store them: 256 states of a cell in int8)
    other.exchange_clusters(rounds=3, pairs=pairs, uniforms=u)
    assert np.array_equal(other.states, ins.states) and np.array_equal(other.exchange_cluster_sizes, ins.exchange_cluster_sizes)


def test_energy_is_conserved_pair_by_pair_and_the_quench_pipeline_runs():
    """C8_J124_001 (512 spins, integer couplings): energy[a] + energy[b] is exactly what it was for every pair of a round; then, from
    quenched states, exchange_clusters() and a quench until nothing moves: the pipeline runs and ends converged."""
    ins = make('j124')
    ins.states = random_states(ins, 32, 9)
    np.random.seed(4)
    sizes = ins.exchange_clusters()
    a, b = ins.exchange_pairs[0, :, 0], ins.exchange_pairs[0, :, 1]
    assert np.all(ins.energy == np.rint(ins.energy))
    assert np.array_equal(ins.energy[a] + ins.energy[b], ins.exchange_energy_before[a] + ins.exchange_energy_before[b])
    assert np.any(ins.energy != ins.exchange_energy_before) and np.all(sizes > 0)
    ins.relax_samples(mode='quench', sweeps=None)
    assert np.all(ins.relax_converged)
    quenched = np.copy(ins.energy)
    ins.exchange_clusters()
    assert same_bits(ins.exchange_energy_before, quenched)
    ins.relax_samples(mode='quench', sweeps=None)
    assert np.all(ins.relax_converged) and np.all(ins.energy <= ins.relax_energy_before)
