"""Host side of the counter-based generator (tnac4o_amd/rng.py): the published known answers, uniforms_host against the scalar
reference of tests/rng_ref.py, the distribution, the stream ids and the kind table, the seed= rules of the five Monte Carlo calls, and
the argument errors of tn_uniforms.  No GPU."""
import ctypes as ct

import numpy as np
import pytest

import rng_ref as rf
from overlap_ref import last_error
from rng_ref import same_bits
from tnac4o_amd import rng


# ---------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize('counter,key,want', rf.KAT, ids=['zero', 'ones', 'pi'])
def test_known_answer_vectors(counter, key, want):
    assert rf.philox(counter, key) == want
    got = rng.philox4x32_10([np.array([c], dtype=np.uint32) for c in counter], [np.array([k], dtype=np.uint32) for k in key])
    assert tuple(int(x[0]) for x in got) == want
    # ... and through U: the counter words are (b lo, b hi, stream lo, stream hi), the key is the seed
    b, stream, seed = counter[0] + (counter[1] << 32), counter[2] + (counter[3] << 32), key[0] + (key[1] << 32)
    if b < 1 << 63:
        u = [float((want[2 * h] + (want[2 * h + 1] << 32)) >> 11) * 2.0 ** -53 for h in (0, 1)]
        assert [rf.U(seed, stream, 2 * b + h) for h in (0, 1)] == u
        assert rng.uniforms_host(seed, stream, 2 * b, 2).tolist() == u


def test_known_numbers():
    seed, stream, raw, u0, u1 = rf.KNOWN
    assert rf.block(seed, stream, 0) == raw
    assert (rf.U(seed, stream, 0), rf.U(seed, stream, 1)) == (u0, u1)
    assert rng.uniforms_host(seed, stream, 0, 2).tolist() == [u0, u1]


# ---------------------------------------------------------------------------------------------- the host function against the reference
@pytest.mark.parametrize('seed,stream,first,n', [(20260004, 7, 1, 9), (20260004, 7, 0, 8), (5, 3, 2 ** 33 - 3, 8), (5, 3, 2 ** 64 - 8, 8),
                                                 (0xa4093822299f31d0, 11 * 2 ** 56 + 2 ** 32 - 1, 5, 6), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 3, 3),
                                                 (1, 2, 3, 0)],
                         ids=['odd-first', 'even-first', 'carry-2^33', 'top', 'wide-seed-stream', 'all-top', 'empty'])
def test_host_function_against_the_reference(seed, stream, first, n):
    got = rng.uniforms_host(seed, stream, first, n)
    want = np.array([rf.U(seed, stream, first + c) for c in range(n)], dtype=np.float64)
    assert got.dtype == np.float64 and same_bits(got, want)
    if n > 2:
        assert len(set(got.tolist())) == n


def test_host_function_refuses():
    for args in ((-1, 0, 0, 1), (2 ** 64, 0, 0, 1), (0, 2 ** 64, 0, 1), (0, 0, 2 ** 64, 0), (0, 0, 2 ** 64 - 1, 2), (0, 0, 0, -1)):
        with pytest.raises(ValueError):
            rng.uniforms_host(*args)


def test_distribution():
    """2^20 numbers lie in [0, 1); their mean is within 5 standard deviations 1 / sqrt(12 n) of 1/2."""
    n = 2 ** 20
    u = rng.uniforms_host(20260004, 7, 0, n)
    assert u.min() >= 0.0 and u.max() < 1.0
    dev = (u.mean() - 0.5) * np.sqrt(12.0 * n)
    print('mean deviates by %.2f standard deviations' % dev)
    assert abs(dev) <= 5.0


# ---------------------------------------------------------------------------------------------- stream ids, kind table
def test_stream_id_limits():
    assert rng.stream_id(0, 0) == 0 and rng.stream_id(11, 5) == 11 * 2 ** 56 + 5 == rf.stream_id(11, 5)
    assert rng.stream_id(255, 2 ** 56 - 1) == 2 ** 64 - 1
    for kind, row in ((1, 2 ** 56), (1, -1), (256, 0), (-1, 0)):
        with pytest.raises(ValueError):
            rng.stream_id(kind, row)
    assert [rng.WALK, rng.RELAX_SWEEP, rng.EXCHANGE_SEED, rng.EXCHANGE_PAIRING, rng.TEMPER_SWEEP, rng.TEMPER_CLUSTER, rng.TEMPER_SWAP, rng.TEMPER_PAIRING,
            rng.ANNEAL_INIT, rng.ANNEAL_RESAMPLE, rng.ANNEAL_SWEEP] == list(range(1, 12))


def _logical(seed, kind, shape, row0=0, first=0):
    """The package's rule: row = the C-order index over all dimensions but the last, i = the last index."""
    rows = int(np.prod(shape[:-1], dtype=np.int64)) if len(shape) > 1 else 1
    return rng.rows_host(seed, kind, row0, rows, first, shape[-1]).reshape(shape)


def test_kind_table_against_the_builders():
    s = 20260004
    ncell, M, sweeps, rounds, T, Tc, Pc, K = 4, 7, 2, 3, 2, 1, 1, 4
    assert same_bits(_logical(s, rng.WALK, (ncell, M)), rf.walk(s, ncell, M))
    assert same_bits(_logical(s, rng.RELAX_SWEEP, (sweeps, ncell, M)), rf.relax_sweep(s, sweeps, ncell, M))
    assert same_bits(_logical(s, rng.EXCHANGE_SEED, (rounds, 3)), rf.exchange_seeds(s, rounds, 3))
    assert np.array_equal(rng.draw_pairs(s, rng.EXCHANGE_PAIRING, rounds, M), rf.exchange_pairs(s, rounds, M))
    M = 6
    R = M // T
    t = rf.temper_uniforms(s, rounds, sweeps, ncell, M, T, Tc, Pc)
    assert same_bits(_logical(s, rng.TEMPER_SWEEP, (rounds, sweeps, ncell, M)), t['sweep'])
    assert same_bits(_logical(s, rng.TEMPER_CLUSTER, (rounds, Tc, Pc)), t['cluster'])
    assert same_bits(_logical(s, rng.TEMPER_SWAP, (rounds, R, T - 1)), t['swap'])
    assert np.array_equal(rng.draw_pairs(s, rng.TEMPER_PAIRING, rounds, R), rf.temper_pairs(s, rounds, R))
    a = rf.anneal_uniforms(s, K, sweeps, ncell, M, True)
    assert same_bits(_logical(s, rng.ANNEAL_INIT, (M, ncell)), a['init'])
    assert same_bits(_logical(s, rng.ANNEAL_RESAMPLE, (K - 1,)), a['resample'])
    assert same_bits(_logical(s, rng.ANNEAL_SWEEP, (K - 1, sweeps, ncell, M)), a['sweep'])
    # a block of rounds / steps and a slice of samples: the GLOBAL row and the logical first
    assert same_bits(_logical(s, rng.TEMPER_SWEEP, (1, sweeps, ncell, 3), row0=2 * sweeps * ncell, first=2), t['sweep'][2:, :, :, 2:5])
    assert same_bits(_logical(s, rng.ANNEAL_RESAMPLE, (2,), first=1), a['resample'][1:])
    # the numbers of sample m do not depend on M
    assert same_bits(rf.relax_sweep(s, sweeps, ncell, 3), rf.relax_sweep(s, sweeps, ncell, 7)[:, :, :3])
    assert same_bits(rf.anneal_uniforms(s, 2, 1, ncell, 3, True)['init'], a['init'][:3])


def test_pairing_rule():
    keys = np.array([0.5, 0.25, 0.5, 0.125, 0.75])
    assert rng.pairs_from_keys(keys).tolist() == [[3, 1], [0, 2]] == rf.pairs_from_keys(keys.tolist()).tolist()
    p = rng.draw_pairs(9, rng.EXCHANGE_PAIRING, 4, 9)
    assert p.shape == (4, 4, 2) and p.dtype == np.int32 and all(np.unique(p[r]).size == 8 for r in range(4))
    assert len({p[r].tobytes() for r in range(4)}) == 4


# ---------------------------------------------------------------------------------------------- the seed argument of the five calls
def _solver():
    import tnac4o_amd
    from tnac4o_amd import auxx
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=2, Ny=2, Nc=8, J=auxx.synthetic_chimera(2, 2, 29), beta=1.0)
    ins.states = np.random.default_rng(3).integers(0, 256, size=(6, 4))
    return ins


BAD_SEEDS = [True, False, np.True_, -1, 2 ** 64, 1.5, '7', (3,)]


def test_check_seed():
    assert rng.check_seed(None) is None and rng.check_seed(0) == 0 and rng.check_seed(2 ** 64 - 1) == 2 ** 64 - 1
    s = rng.check_seed(np.uint64(2 ** 63 + 1))
    assert type(s) is int and s == 2 ** 63 + 1
    for bad in BAD_SEEDS:
        with pytest.raises(ValueError, match='seed'):
            rng.check_seed(bad)


@pytest.mark.parametrize('call', ['sample', 'relax', 'exchange', 'temper', 'anneal', 'anneal_fresh'])
def test_seed_errors_come_before_device_work(call, monkeypatch):
    """A seed that is no integer in [0, 2^64), a bool, a seed together with uniforms, and a seed with a quench: ValueError, nothing on the
    device and nothing from numpy's generator (the ctypes binding and numpy.random.rand are replaced by a trap)."""
    from tnac4o_amd import _lib

    def trap(*a, **k):
        raise AssertionError('device or generator work before the seed was checked')

    ins = _solver()
    monkeypatch.setattr(_lib, 'lib', trap)
    monkeypatch.setattr(np.random, 'rand', trap)
    monkeypatch.setattr(np.random, 'permutation', trap)
    monkeypatch.setattr(ins, '_setup_rhoT', trap)
    u = np.full((1, 1), 0.5)                                             # (its shape is never looked at)
    run = {'sample': lambda **k: ins.sample_boltzmann(M=4, **k),
           'relax': lambda **k: ins.relax_samples(sweeps=1, **k),
           'exchange': lambda **k: ins.exchange_clusters(rounds=1, **k),
           'temper': lambda **k: ins.temper_samples([0.5, 1.0], rounds=1, **k),
           'anneal': lambda **k: ins.anneal_population([0.5, 1.0], **k),
           'anneal_fresh': lambda **k: ins.anneal_population([0.0, 1.0], M=4, **k)}[call]
    for bad in BAD_SEEDS:
        with pytest.raises(ValueError, match='seed'):
            run(seed=bad)
    with pytest.raises(ValueError, match='seed'):
        run(seed=5, uniforms={'sweep': u} if call in ('temper', 'anneal', 'anneal_fresh') else u)
    if call == 'relax':
        with pytest.raises(ValueError, match='seed'):
            run(seed=5, mode='quench')
        with pytest.raises(ValueError, match='seed'):
            ins.relax_samples(sweeps=None, mode='quench', seed=5)


def test_seeded_pairings_leave_the_global_generator_alone():
    from tnac4o_amd import exchange, temper
    ins = _solver()
    np.random.seed(4)
    want = np.random.rand(3)
    np.random.seed(4)
    rounds, pairs, u = exchange.check_arguments(ins, 2, None, None, seed=12)
    assert u is None and np.array_equal(pairs, rf.exchange_pairs(12, 2, 6)) and pairs.dtype == np.int32
    a = temper.check_arguments(ins, [0.5, 1.0], 3, 1, True, None, None, None, None, None, seed=12)
    assert a['seed'] == 12 and a['uniforms'] is None and np.array_equal(a['pairs'], rf.temper_pairs(12, 3, 3))
    given = np.array([[[2, 0]]] * 3)
    a = temper.check_arguments(ins, [0.5, 1.0], 3, 1, True, None, given, None, None, None, seed=12)
    assert np.array_equal(a['pairs'], given)                             # explicit pairs with a seed are allowed
    assert np.array_equal(np.random.rand(3), want)


# ---------------------------------------------------------------------------------------------- the export
def test_uniforms_argument_errors():
    """rc = -1 with a message that starts with tn_uniforms and names the limit, nothing launched: the pointers below are not device memory,
    they are never followed.  rows = 0 and cols = 0 are valid no-ops."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    p = 4096                                                             # stands for a non-null device pointer

    def call(seed=1, stream0=2, first=3, rows=2, cols=5, out=p, ld=8):
        return L.tn_uniforms(seed, stream0, first, rows, cols, out, ld, None)

    for kw, word in ((dict(out=None), 'null'), (dict(out=p + 4), 'aligned'), (dict(rows=-1), 'negative'), (dict(cols=-1), 'negative'), (dict(ld=4), 'ld < cols'),
                     (dict(rows=2 ** 31, ld=2 ** 31), '2^62'), (dict(rows=1, cols=1, ld=2 ** 62), '2^62'), (dict(first=2 ** 64 - 4), 'first + cols'),
                     (dict(first=2 ** 64 - 1, cols=2), 'first + cols'), (dict(stream0=2 ** 64 - 1), 'stream0 + rows'),
                     (dict(rows=0, first=2 ** 64 - 4), 'first + cols'), (dict(cols=0, ld=0, stream0=2 ** 64 - 1), 'stream0 + rows')):
        assert call(**kw) == -1, kw
        msg = last_error(L)
        assert msg.startswith('tn_uniforms') and word in msg, (kw, msg)
    assert call(rows=0) == 0 and call(cols=0) == 0 and call(rows=0, cols=0, out=None, ld=0) == 0
    assert call(rows=0, stream0=2 ** 64 - 1) == 0 and call(cols=0, first=2 ** 64 - 1) == 0
