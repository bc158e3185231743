"""tn_uniforms and seed= of the five Monte Carlo calls on the GPU against the scalar reference of tests/rng_ref.py: the kernel bit for
bit on every store form with a sentinel in every padding element, the split of a fill, and each public call with seed=s against the
same call with uniforms= (and pairs=) built by the reference -- chunked, cut into calls, on a prefix, and seed=None as it was."""
import numpy as np
import pytest

import rng_ref as rf
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SEED = 20260004
SENTINEL = 0x55
M70 = 70                                                                 # no multiple of 64
CHUNK = 33                                                               # chunks begin at odd indices


# ---------------------------------------------------------------------------------------------- 1. the kernel
# (seed, stream0, first, rows, cols, ld, byte offset of the base from a 16-byte boundary)
FILLS = {
    '1x1': (SEED, 7, 0, 1, 1, 1, 0),
    '1x2': (SEED, 7, 0, 1, 2, 2, 0),
    '3x5-ld8': (SEED, 7, 0, 3, 5, 8, 0),
    '2x129-odd-first': (SEED, 7, 1, 2, 129, 129, 0),
    '257x3': (SEED, 7, 0, 257, 3, 3, 0),
    '1x65537-odd-first': (SEED, 7, 3, 1, 65537, 65537, 0),
    'carry-2^33': (SEED, 7, 2 ** 33 - 3, 2, 8, 8, 0),
    'top-of-the-counter': (SEED, 7, 2 ** 64 - 8, 2, 8, 8, 0),
    'stream-carry': (SEED, 11 * 2 ** 56 + 2 ** 32 - 1, 0, 3, 4, 4, 0),
    'wide-seed': (0xa4093822299f31d0, 7, 0, 2, 4, 6, 0),
    'zero-vector': (0, 0, 0, 1, 2, 2, 0),
    'base-offset-8': (SEED, 7, 0, 3, 6, 7, 8),
}


def fill_device(seed, stream0, first, rows, cols, ld, offset):
    """One tn_uniforms into a buffer of sentinel bytes between guards; returns the (rows, ld) doubles as they are afterwards."""
    from tnac4o_amd import _lib, ops
    n = rows * ld
    g = Guarded(offset + 8 * n, SENTINEL, seed=1)
    assert g.ptr % 16 == 0
    rc = _lib.lib().tn_uniforms(seed, stream0, first, rows, cols, g.ptr + offset, ld, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert g.intact() and bool(g.body[:offset].eq(SENTINEL).all())
    return g.body[offset:].cpu().numpy().view(np.float64).reshape(rows, ld)


@pytest.mark.parametrize('case', list(FILLS), ids=list(FILLS))
def test_fill_against_the_reference(case):
    """Bit-identical to the reference; every element c >= cols of a row, the bytes before an offset base and the guards keep their bytes."""
    seed, stream0, first, rows, cols, ld, offset = FILLS[case]
    got = fill_device(seed, stream0, first, rows, cols, ld, offset)
    want = rf.fill(seed, stream0, first, rows, cols)
    assert same_bits(np.ascontiguousarray(got[:, :cols]), want)
    assert np.all(np.ascontiguousarray(got[:, cols:]).view(np.uint8) == SENTINEL)
    assert want.min() >= 0.0 and want.max() < 1.0
    if case == 'zero-vector':
        x = rf.KAT[0][2]
        assert got[0].tolist() == [float((x[0] + (x[1] << 32)) >> 11) * 2.0 ** -53, float((x[2] + (x[3] << 32)) >> 11) * 2.0 ** -53]


def test_store_form_changes_no_bit():
    """The same numbers through 16-byte stores (even first, aligned base) and through 8-byte stores (base offset by 8; an odd ld)."""
    a = fill_device(SEED, 9, 4, 4, 64, 64, 0)
    b = fill_device(SEED, 9, 4, 4, 64, 64, 8)
    c = fill_device(SEED, 9, 4, 4, 64, 65, 0)
    assert same_bits(a, b) and same_bits(a, np.ascontiguousarray(c[:, :64]))


def test_a_fill_equals_its_two_parts():
    """[0, n) against [0, a) and [a, n) with a odd; rows of a strided tensor; zero sizes; the wrapper's own refusals."""
    from tnac4o_amd import ops
    rows, n, a = 3, 1001, 333
    whole = ops.uniforms(SEED, 40, 0, rows, n)
    assert whole.shape == (rows, n) and whole.dtype == torch.float64 and whole.is_cuda
    parts = torch.full((rows, n + 4), -1.0, dtype=torch.float64, device='cuda')
    assert ops.uniforms(SEED, 40, 0, rows, a, out=parts[:, :a]).data_ptr() == parts.data_ptr()
    ops.uniforms(SEED, 40, a, rows, n - a, out=parts[:, a:n])
    assert torch.equal(parts[:, :n], whole) and bool((parts[:, n:] == -1.0).all())
    assert same_bits(whole[1].cpu().numpy(), rf.fill(SEED, 41, 0, 1, n)[0])
    assert ops.uniforms(SEED, 0, 0, 0, 5).shape == (0, 5) and ops.uniforms(SEED, 0, 0, 5, 0).shape == (5, 0)
    with pytest.raises(RuntimeError):
        ops.uniforms(SEED, 0, 0, 1, 2, out=torch.zeros(1, 2, dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.uniforms(SEED, 0, 0, 2, 2, out=torch.zeros(2, 2, dtype=torch.float64, device='cuda').t())
    with pytest.raises(ValueError):
        ops.uniforms(2 ** 64, 0, 0, 1, 1)


# ---------------------------------------------------------------------------------------------- 2. the public calls
INSTANCES = ['chimera', 'ising3x3', 'rmf2x2']
ISING = ['chimera', 'ising3x3']


def solver(name, beta=1.0):
    import tnac4o_amd
    from tnac4o_amd import auxx
    import marginals_ref as mr
    if name == 'chimera':                                                # 32 spins, 2 x 2 cells of q = 256
        return tnac4o_amd.tnac4o(mode='Ising', Nx=2, Ny=2, Nc=8, J=auxx.synthetic_chimera(2, 2, 29), beta=beta)
    if name == 'ising3x3':
        return tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=beta)
    return tnac4o_amd.tnac4o(mode='RMF', Nx=2, Ny=2, J=auxx.synthetic_rmf(2, 2, 4, 17), beta=beta)


def with_states(name, M=M70, seed=50):
    ins = solver(name)
    qs = ins._cell_sizes()[ins.order]                                    # model order
    ins.states = np.random.default_rng(seed).integers(0, qs[None, :], size=(M, qs.size))
    return ins


def assert_same(a, b, names):
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(x, np.ndarray):
            assert same_bits(x, np.asarray(y)), k
        else:
            assert x == y, k


@pytest.mark.parametrize('name', INSTANCES)
def test_sample_boltzmann(name):
    ncell = 9 if name == 'ising3x3' else 4
    a, b, c = solver(name), solver(name), solver(name)
    a.sample_boltzmann(M=M70, Dmax=8, seed=SEED, chunk=CHUNK)
    b.sample_boltzmann(M=M70, Dmax=8, uniforms=rf.walk(SEED, ncell, M70))
    c.sample_boltzmann(M=M70, Dmax=8, seed=SEED)
    names = ('states', 'energy', 'probability', 'sample_log2Z', 'log2Z_lower', 'log2Z_estimate', 'negative_probability')
    assert_same(a, b, names)
    assert_same(c, b, names)
    assert len({tuple(r) for r in a.states.tolist()}) > 1


@pytest.mark.parametrize('name', INSTANCES)
def test_relax_samples(name):
    """seed= against the reference's uniforms; chunked against unchunked; the first 31 of 70 states alone give the first 31 rows."""
    ncell = 9 if name == 'ising3x3' else 4
    a, b, c, d = (with_states(name) for _ in range(4))
    start = np.copy(a.states)
    a.relax_samples(sweeps=2, seed=SEED, chunk=CHUNK)
    b.relax_samples(sweeps=2, uniforms=rf.relax_sweep(SEED, 2, ncell, M70))
    c.relax_samples(sweeps=2, seed=SEED)
    names = ('states', 'energy', 'relax_energy_before', 'relax_moves', 'relax_converged', 'relax_sweeps')
    assert_same(a, b, names)
    assert_same(c, b, names)
    assert not np.array_equal(a.states, start)
    d.relax_samples(sweeps=2, seed=SEED, states=start[:31])
    assert np.array_equal(d.states, a.states[:31]) and same_bits(d.energy, a.energy[:31]) and np.array_equal(d.relax_moves, a.relax_moves[:31])
    d.relax_samples(sweeps=2, seed=SEED + 1, states=start)               # another seed: other numbers
    assert not np.array_equal(d.states, a.states)


@pytest.mark.parametrize('name', ISING)
def test_exchange_clusters(name):
    rounds, P = 3, M70 // 2
    a, b, c = (with_states(name) for _ in range(3))
    pairs, u = rf.exchange_pairs(SEED, rounds, M70), rf.exchange_seeds(SEED, rounds, P)
    state = np.random.get_state()[1].copy()
    a.exchange_clusters(rounds=rounds, seed=SEED)
    assert np.array_equal(np.random.get_state()[1], state)               # numpy's global generator is not touched
    b.exchange_clusters(rounds=rounds, pairs=pairs, uniforms=u)
    names = ('states', 'energy', 'exchange_energy_before', 'exchange_pairs', 'exchange_cluster_sizes', 'exchange_differing')
    assert_same(a, b, names)
    assert a.exchange_cluster_sizes.max() > 0
    other = pairs[:, ::-1, ::-1].copy()                                  # explicit pairs with a seed: only the uniforms come from it
    a2, b2 = with_states(name), with_states(name)
    a2.exchange_clusters(rounds=rounds, pairs=other, seed=SEED)
    b2.exchange_clusters(rounds=rounds, pairs=other, uniforms=u)
    assert_same(a2, b2, names)
    assert c.exchange_clusters(rounds=0, seed=SEED).shape == (0, P)


TEMPER_ATTRS = ('states', 'energy', 'temper_betas', 'temper_index', 'temper_beta', 'temper_swap_accepted', 'temper_swap_attempted',
                'temper_energy_trace', 'temper_cluster_sizes', 'temper_cluster_differing')


@pytest.mark.parametrize('name', INSTANCES)
def test_temper_samples(name):
    """seed= against the reference's uniforms and pairs (cluster moves on the Ising instances); rounds_per_call 1 against None."""
    ncell = 9 if name == 'ising3x3' else 4
    betas = [0.3, 0.6, 0.9, 1.3, 1.8]
    T, rounds, sweeps = 5, 3, 2
    R = M70 // T
    cluster = name in ISING
    Tc, Pc = (T, R // 2) if cluster else (0, 0)
    u = rf.temper_uniforms(SEED, rounds, sweeps, ncell, M70, T, Tc, Pc)
    pairs = rf.temper_pairs(SEED, rounds, R) if cluster else None
    a, b, c = (with_states(name) for _ in range(3))
    a.temper_samples(betas, rounds=rounds, sweeps=sweeps, cluster_moves=cluster, seed=SEED, record=True, rounds_per_call=1)
    b.temper_samples(betas, rounds=rounds, sweeps=sweeps, cluster_moves=cluster, pairs=pairs, uniforms=u, record=True)
    c.temper_samples(betas, rounds=rounds, sweeps=sweeps, cluster_moves=cluster, seed=SEED, record=True)
    assert_same(a, b, TEMPER_ATTRS)
    assert_same(c, b, TEMPER_ATTRS)
    assert a.temper_swap_accepted.sum() > 0
    if cluster:                                                          # explicit pairs with a seed
        other = pairs[:, ::-1, ::-1].copy()
        a.temper_samples(betas, rounds=rounds, sweeps=sweeps, pairs=other, seed=SEED, record=True)
        b.temper_samples(betas, rounds=rounds, sweeps=sweeps, pairs=other, uniforms=u, record=True)
        assert_same(a, b, TEMPER_ATTRS)


ANNEAL_ATTRS = ('states', 'energy', 'anneal_betas', 'anneal_log2Z', 'anneal_free_energy', 'anneal_energy_mean', 'anneal_heat_capacity', 'anneal_ess',
                'anneal_survivors', 'anneal_family', 'anneal_rho_t', 'anneal_family_entropy', 'anneal_energy_trace', 'anneal_parent_trace')


@pytest.mark.parametrize('name', INSTANCES)
@pytest.mark.parametrize('fresh', [False, True], ids=['stored', 'fresh'])
def test_anneal_population(name, fresh):
    """seed= against the reference's uniforms, on the stored states and on a population drawn on the device; steps_per_call 1, 2, None."""
    ncell = 9 if name == 'ising3x3' else 4
    betas = [0.0, 0.4, 0.8, 1.2, 1.7] if fresh else [0.2, 0.5, 0.9, 1.4, 2.0]
    K, sweeps = 5, 2
    u = rf.anneal_uniforms(SEED, K, sweeps, ncell, M70, fresh)
    make = (lambda: solver(name)) if fresh else (lambda: with_states(name))
    kw = dict(sweeps=sweeps, M=M70 if fresh else None, record=True)
    b = make()
    b.anneal_population(betas, uniforms=u, **kw)
    assert np.unique(b.anneal_family).size < M70
    for per in (1, 2, None):
        a = make()
        a.anneal_population(betas, seed=SEED, steps_per_call=per, **kw)
        assert_same(a, b, ANNEAL_ATTRS)


def test_seed_none_is_the_parent():
    """seed=None with numpy's generator seeded: the numbers the call drew before, in the same order."""
    a, b = with_states('chimera'), with_states('chimera')
    np.random.seed(5)
    a.relax_samples(sweeps=2)
    np.random.seed(5)
    u = np.random.rand(2, 4, M70)
    after = np.random.rand()
    b.relax_samples(sweeps=2, uniforms=u)
    assert_same(a, b, ('states', 'energy', 'relax_moves'))
    np.random.seed(5)
    a.relax_samples(sweeps=2, seed=None)
    assert np.random.rand() == after
    np.random.seed(5)
    a.relax_samples(sweeps=2, seed=SEED)                                 # a seed leaves numpy's generator where it is
    assert np.random.rand() == np.random.RandomState(5).rand()
