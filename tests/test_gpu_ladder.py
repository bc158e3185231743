"""tn_ladder_measure and tnac4o.temper_samples(measure=) on the GPU against the numpy reference of tests/ladder_ref.py: direct calls over
the word boundaries, chain counts, splits and link counts; accumulation into pre-filled 64-bit counters; the skip rules; independence
of the grid; refusals; tn_pair_hist on the same rows; the public call against temper_ref.run walked round by round, in both rotations,
and a static chain.  Every comparison is exact; every buffer of a library call lies between guards."""
import ctypes as ct

import numpy as np
import pytest

import ladder_ref as lr
import temper_ref as tr
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_relax import DeviceCells, solver_cells                    # noqa: E402  (helpers only, no test is imported)
from test_gpu_sampling import dv, small                                 # noqa: E402
from test_gpu_temper import _framed, _last_error, _random_states        # noqa: E402


# ---------------------------------------------------------------------------------------------- helpers
LAT = tr.ising_lattice()
QS = np.array([c['q'] for c in LAT['cells']])
NSPIN = np.array([int(q).bit_length() - 1 for q in QS])


def _cells():
    if not hasattr(_cells, 'dc'):
        _cells.dc = DeviceCells(LAT['cells'])
    return _cells.dc


def make_case(nbits, R, T, nlinks, seed):
    """Random inputs on the synthetic Ising lattice: states inside their cells, slot with the labels of every chain permuted as swaps
    leave them, a bitcell table of nbits random (cell, bit) entries, nlinks random links (i != j allowed to coincide), energies."""
    rng = np.random.default_rng(seed)
    M = R * T
    k = rng.integers(0, 16, nbits)
    bitcell = np.stack([k, rng.integers(0, NSPIN[k])], axis=1).astype(np.int32)
    return dict(nbits=nbits, R=R, T=T, M=M, states=rng.integers(0, QS[None, :], size=(M, 16)), bitcell=bitcell,
                slot=np.array([c * T + rng.permutation(T) for c in range(R)], dtype=np.int32).reshape(R, T),
                links=rng.integers(0, nbits, (nlinks, 2)).astype(np.int32), energy=rng.normal(size=M) * 10.0)


def measure_device(c, split=0, spin0=None, link0=None, esums0=None, null=(), want_rc=0, ws_short=0, calls=1, **over):
    """`calls` calls of tn_ladder_measure on a case with every buffer between guards.  spin0 / link0 / esums0: what the accumulators hold
    before (None: zeros); null: names among 'cells', 'states', 'slot', 'bitcell', 'links', 'energy', 'spin', 'link', 'esums', 'ws' passed
    as NULL; over: nbits / nlinks / M / T as the call sees them (the buffers keep the case's sizes).  Returns dict(rc, spin, link
    (uint64), esums)."""
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    nbits, R, T, M = c['nbits'], c['R'], c['T'], c['M']
    nlinks = c['links'].shape[0]
    a_nbits, a_nlinks, a_M, a_T = over.get('nbits', nbits), over.get('nlinks', nlinks), over.get('M', M), over.get('T', T)
    need = int(L.tn_ladder_measure_ws_bytes(4, 4, a_M, a_T, a_nbits, a_nlinks))       # (0 for a shape the call refuses)
    assert need > 0 or want_rc == -1
    ws = Guarded(max(need - ws_short, 0) if need else 64, 'random', seed=1)
    g_st = _framed(torch.int16, c['states'].astype(np.int16), 2)
    g_slot = _framed(torch.int32, c['slot'], 3)
    g_bc = _framed(torch.int32, c['bitcell'], 4)
    g_ln = _framed(torch.int32, c['links'], 5)
    g_E = _framed(torch.float64, c['energy'], 6)
    z = lambda n: np.zeros((T, n), dtype=np.uint64)                     # noqa: E731
    g_sh = _framed(torch.int64, (z(nbits + 1) if spin0 is None else np.asarray(spin0, dtype=np.uint64)).view(np.int64), 7)
    g_lh = _framed(torch.int64, (z(nlinks + 1) if link0 is None else np.asarray(link0, dtype=np.uint64)).view(np.int64), 8)
    g_es = _framed(torch.float64, np.zeros((T, 3)) if esums0 is None else np.asarray(esums0, dtype=np.float64), 9)
    p = dict(cells=_cells().ptr, states=g_st.ptr, slot=g_slot.ptr, bitcell=g_bc.ptr, links=g_ln.ptr if nlinks else None, energy=g_E.ptr, spin=g_sh.ptr,
             link=g_lh.ptr, esums=g_es.ptr, ws=ws.ptr)
    for name in null:
        p[name] = None
    rc = 0
    for _ in range(calls):
        rc = L.tn_ladder_measure(4, 4, p['cells'], a_M, a_T, p['states'], p['slot'], a_nbits, p['bitcell'], p['links'], a_nlinks, over.get('split', split),
                                 p['energy'], p['spin'], p['link'], p['esums'], p['ws'], max(need - ws_short, 0), ops._stream())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _last_error())
    for g in (ws, g_st, g_slot, g_bc, g_ln, g_E, g_sh, g_lh, g_es):
        assert g.intact()
    assert np.array_equal(g_st.host(), c['states']) and np.array_equal(g_slot.host(), c['slot']) and same_bits(g_E.host(), c['energy'])
    return dict(rc=rc, spin=g_sh.host().view(np.uint64), link=g_lh.host().view(np.uint64), esums=g_es.host())


def reference(c, split=0, spin0=None, link0=None, esums0=None, calls=1, links=True, energy=True):
    """What measure_device must leave: the accumulators plus `calls` times the increments of ladder_ref."""
    T, M = c['T'], c['M']
    nlinks = c['links'].shape[0]
    hs, hl = lr.measure(LAT['cells'], c['states'], c['slot'], c['nbits'], c['bitcell'], c['links'] if nlinks and links else None, split)
    spin = np.zeros((T, c['nbits'] + 1), dtype=np.uint64) if spin0 is None else np.asarray(spin0, dtype=np.uint64)
    link = np.zeros((T, nlinks + 1), dtype=np.uint64) if link0 is None else np.asarray(link0, dtype=np.uint64)
    es = np.zeros((T, 3)) if esums0 is None else np.asarray(esums0, dtype=np.float64)
    for _ in range(calls):
        spin = lr.add_hist(spin, hs)
        if hl is not None:
            link = lr.add_hist(link, hl)
        if energy:
            es = lr.add_esums(es, c['slot'], c['energy'], M)
    return dict(spin=spin, link=link, esums=es)


def assert_same(got, ref):
    assert np.array_equal(got['spin'], ref['spin']) and np.array_equal(got['link'], ref['link']) and same_bits(got['esums'], ref['esums'])


# ---------------------------------------------------------------------------------------------- 1. direct calls against the reference
@pytest.mark.parametrize('nbits', [1, 63, 64, 65, 130])
def test_direct_call_against_the_reference(nbits):
    """R in {1, 2, 3, 17} x T in {1, 3} with permuted labels, every split of {0, 1, R // 2, R} and nlinks cycling through {0, 1, 64, 200}
    (nlinks > nbits occurs at every nbits): the histograms as integers, esums in the reference's bits, the inputs and the frames
    untouched."""
    seen = set()
    for i, (R, T) in enumerate((R, T) for R in (1, 2, 3, 17) for T in (1, 3)):
        for j, split in enumerate(sorted({0, 1, R // 2, R})):
            nlinks = (0, 1, 64, 200)[(i + j + nbits) % 4]
            seen.add(nlinks)
            c = make_case(nbits, R, T, nlinks, 100 * nbits + 10 * i + j)
            got = measure_device(c, split)
            ref = reference(c, split)
            assert_same(got, ref)
            pairs = len(lr.counted_pairs(R, split))
            assert got['spin'].sum(axis=1).tolist() == [pairs] * T and got['esums'][:, 0].tolist() == [1.0] * T
            if nlinks:
                assert got['link'].sum(axis=1).tolist() == [pairs] * T
    assert seen == {0, 1, 64, 200}


def test_optional_operands_null_in_turn():
    """link_hist, energy and esums NULL in turn: what belongs to the missing operand is left alone, the rest is the reference's."""
    c = make_case(65, 17, 3, 200, 7)
    ref = reference(c, 0)
    got = measure_device(c, null=('link',))
    assert np.array_equal(got['spin'], ref['spin']) and not got['link'].any() and same_bits(got['esums'], ref['esums'])
    for name in ('energy', 'esums'):
        got = measure_device(c, null=(name,))
        assert np.array_equal(got['spin'], ref['spin']) and np.array_equal(got['link'], ref['link']) and not got['esums'].any()
    got = measure_device(c, null=('links',), nlinks=0)                   # no link overlap by nlinks = 0
    assert np.array_equal(got['spin'], ref['spin']) and not got['link'].any()


def test_more_tiles_than_one_and_the_largest_row():
    """R = 50: four blocks of 16 chains, ten tiles of the folded triangle and the rectangles of two splits, tiles g, g + G, ... of one
    workgroup.  nbits = nlinks = 38815, the limit: the largest histogram the 160 KiB of LDS take."""
    c = make_case(70, 50, 2, 64, 21)
    for split in (0, 16, 33):
        assert_same(measure_device(c, split), reference(c, split))
    big = make_case(lr.MAX_NBITS, 2, 1, lr.MAX_NBITS, 22)
    assert_same(measure_device(big), reference(big))


# ---------------------------------------------------------------------------------------------- 2. accumulation
def test_accumulation_is_a_64_bit_add():
    """Accumulators pre-filled with random values, some >= 2^32, and some 2^64 - 1 minus the expected increment (a carry out of the low
    32 bits that a split add would lose; the sum lands on 2^64 - 1 exactly); two consecutive calls equal the sum of two references; a
    pre-filled esums continues in the kernel's order."""
    c = make_case(130, 17, 3, 200, 31)
    rng = np.random.default_rng(32)
    inc = reference(c, 0)
    spin0 = rng.integers(0, 2 ** 31, inc['spin'].shape).astype(np.uint64)
    link0 = rng.integers(0, 2 ** 31, inc['link'].shape).astype(np.uint64)
    spin0[:, ::3] += np.uint64(2 ** 32) * rng.integers(1, 2 ** 20, spin0[:, ::3].shape).astype(np.uint64)
    link0[:, 1::2] = np.uint64(2 ** 32) - np.uint64(1)                   # the next count carries into the upper half
    hot = inc['spin'] > 0
    spin0[hot] = np.uint64(2 ** 64 - 1) - inc['spin'][hot]
    assert hot.any() and (spin0 >= 2 ** 32).any()
    esums0 = rng.normal(size=(3, 3)) * 1e3
    got = measure_device(c, 0, spin0, link0, esums0)
    ref = reference(c, 0, spin0, link0, esums0)
    assert_same(got, ref)
    assert np.all(got['spin'][hot] == np.uint64(2 ** 64 - 1)) and np.array_equal(got['link'], link0 + inc['link'])
    assert np.any((link0 < 2 ** 32) & (got['link'] >= 2 ** 32))
    two = measure_device(c, 0, spin0 * 0 + 5, link0, esums0, calls=2)
    assert_same(two, reference(c, 0, spin0 * 0 + 5, link0, esums0, calls=2))
    assert np.array_equal(two['spin'], np.uint64(5) + np.uint64(2) * inc['spin'])


# ---------------------------------------------------------------------------------------------- 3. skip rules and the conversion
def test_skip_rules_and_conversion():
    """slot entries -1 and M take their chain's pairs at that temperature out (never an index: guards intact); links entries -1 and
    nbits give link bit 0; bitcell entries out of range leave the bit 0; states -1 and q are read as 0."""
    c = make_case(65, 5, 3, 64, 41)
    M, T = c['M'], c['T']
    c['slot'][1, 0], c['slot'][3, 2], c['slot'][4, 2] = -1, M, 2 ** 31 - 1
    c['links'][0], c['links'][5], c['links'][63] = (-1, 3), (2, 65), (-2 ** 31, 2 ** 31 - 1)
    c['bitcell'][0], c['bitcell'][7], c['bitcell'][64], c['bitcell'][20] = (-1, 0), (16, 0), (3, 15), (2, -1)
    for m, k, v in ((0, 3, 256), (2, 0, -1), (5, 2, 32), (7, 5, 32767), (9, 15, 300), (11, 1, 8), (14, 7, -32768)):
        c['states'][m, k] = v
    for split in (0, 2):
        got = measure_device(c, split)
        assert_same(got, reference(c, split))
    got = measure_device(c, 0)
    assert got['spin'].sum(axis=1).tolist() == [6, 10, 3] and got['link'].sum(axis=1).tolist() == [6, 10, 3]
    E = c['energy']                                                      # the skipped rows contribute no energy either
    assert got['esums'][0].tolist() == [1.0, ((E[c['slot'][0, 0]] + E[c['slot'][2, 0]]) + E[c['slot'][3, 0]]) + E[c['slot'][4, 0]],
                                        lr.add_esums(np.zeros((T, 3)), c['slot'], E, M)[0, 2]]
    rows = tr.to_bits(LAT['cells'], c['states'], 65, c['bitcell'])       # what the reference makes of the bad table entries: bit 0
    assert all(((v >> 0) & 1, (v >> 7) & 1, (v >> 64) & 1, (v >> 20) & 1) == (0, 0, 0, 0) for v in rows)


# ---------------------------------------------------------------------------------------------- 4. grid independence
@pytest.mark.parametrize('R,T', [(17, 1), (17, 3), (50, 2)])
def test_grid_independence(R, T, monkeypatch):
    """TN_LADDER_WGS in {1, 3, 7, default}: identical bits, and the workspace the query asks for follows the knob (read per call)."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    c = make_case(130, R, T, 200, 51)
    ref = reference(c, 0)
    monkeypatch.delenv('TN_LADDER_WGS', raising=False)
    dflt = int(L.tn_ladder_measure_ws_bytes(4, 4, c['M'], T, 130, 200))
    assert_same(measure_device(c), ref)
    sizes = {}
    for wgs in (1, 3, 7):
        monkeypatch.setenv('TN_LADDER_WGS', str(wgs))
        sizes[wgs] = int(L.tn_ladder_measure_ws_bytes(4, 4, c['M'], T, 130, 200))
        assert_same(measure_device(c), ref)
        assert_same(measure_device(c, R // 2), reference(c, R // 2))
    if R == 17:                                                          # 3 tiles of 16 x 16 chains: never more workgroups than tiles
        assert sizes[1] < sizes[3] == sizes[7] == dflt
    else:                                                                # 10 tiles
        assert sizes[1] < sizes[3] < sizes[7] < dflt


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_accumulators():
    """rc = -1 for nbits = 0, nbits or nlinks one above the limit, M no multiple of T, a null operand, a split outside 0 .. R; rc = -3 for
    a workspace one byte short; the message starts with tn_ladder_measure and names the limit; the accumulators keep their bits."""
    from tnac4o_amd import _lib
    L = _lib.lib()
    c = make_case(65, 4, 3, 64, 61)
    rng = np.random.default_rng(62)
    spin0 = rng.integers(0, 2 ** 63, (3, 66)).astype(np.uint64)
    link0 = rng.integers(0, 2 ** 63, (3, 65)).astype(np.uint64)
    esums0 = rng.normal(size=(3, 3))

    def refused(word, want_rc=-1, **kw):
        got = measure_device(c, kw.pop('split', 0), spin0, link0, esums0, want_rc=want_rc, **kw)
        msg = _last_error()
        assert msg.startswith('tn_ladder_measure') and word in msg, (kw, msg)
        assert np.array_equal(got['spin'], spin0) and np.array_equal(got['link'], link0) and same_bits(got['esums'], esums0)

    refused('38815', nbits=0)
    refused('38815', nbits=lr.MAX_NBITS + 1)
    refused('38815', nlinks=lr.MAX_NBITS + 1)
    refused('multiple', M=11)
    refused('multiple', T=0)
    refused('split', split=5)
    refused('split', split=-1)
    for name, word in (('cells', 'cells'), ('states', 'states'), ('slot', 'slot'), ('bitcell', 'bitcell'), ('spin', 'spin_hist'), ('links', 'links'),
                       ('ws', 'ws')):
        refused(word, null=(name,))
    need = int(L.tn_ladder_measure_ws_bytes(4, 4, 12, 3, 65, 64))
    refused(str(need), want_rc=-3, ws_short=1)
    for shape in ((0, 4, 12, 3, 65, 64), (4, 4, -1, 3, 65, 64), (4, 4, 2 ** 31, 1, 65, 64), (4, 4, 12, 0, 65, 64), (4, 4, 11, 3, 65, 64), (4, 4, 12, 3, 0, 64),
                  (4, 4, 12, 3, lr.MAX_NBITS + 1, 64), (4, 4, 12, 3, 65, -1), (4, 4, 12, 3, 65, lr.MAX_NBITS + 1), (4, 4, 65537, 1, 65, 0)):
        assert int(L.tn_ladder_measure_ws_bytes(*shape)) == 0, shape
    assert int(L.tn_ladder_measure_ws_bytes(4, 4, 0, 3, 65, 0)) > 0 and int(L.tn_ladder_measure_ws_bytes(4, 4, 65536, 1, 65, 0)) > 0
    assert_same(measure_device(c, 0, spin0, link0, esums0), reference(c, 0, spin0, link0, esums0))      # and the call they refused goes through


# ---------------------------------------------------------------------------------------------- 6. the existing kernel on the same rows
def test_cross_check_with_pair_hist():
    """T = 1, R = 33, nbits = 130: one measurement equals the low limbs of tn_pair_hist on the same packed rows with unit weights (the
    high limbs are zero)."""
    from tnac4o_amd import ops
    c = make_case(130, 33, 1, 0, 71)
    got = measure_device(c)
    rows = tr.to_bits(LAT['cells'], c['states'], 130, c['bitcell'])
    words = np.array([[(v >> (64 * w)) & (2 ** 64 - 1) for w in range(3)] for v in rows], dtype=np.uint64)
    limbs = ops.pair_hist(dv(words.view(np.int64)), 130).cpu().numpy().view(np.uint64)
    assert not limbs[:, 1].any() and np.array_equal(got['spin'][0], limbs[:, 0]) and got['spin'].sum() == 33 * 32 // 2


# ---------------------------------------------------------------------------------------------- 7. the public call
BETAS = [0.3, 0.7, 1.2]
M_PUB, T_PUB, R_PUB, ROUNDS, SWEEPS = 12, 3, 4, 7, 1
MEASURE = dict(measure=2, measure_from=1, measure_bins=2)


def _fresh(name, seed=40):
    ins = small(name, 1.0)
    ins.states = _random_states(ins, M_PUB, seed)
    return ins


def _walk_solver(ins, start, a, u, m):
    """ladder_ref.walk on a solver: the lattice from the solver's own host tables, the tables from the package's host functions."""
    from tnac4o_amd import exchange as ex
    from tnac4o_amd import ladder
    from tnac4o_amd import temper as tp
    cells = solver_cells(ins)
    nbits, cellbits, bitcell = tp.bit_tables(ins)
    bits = ((nbits, cellbits, bitcell) + ex.coupling_csr(ins)) if a['cluster'] else None
    rot = np.empty_like(start)
    rot[:, ins.order] = start
    plan, B = lr.schedule(a['rounds'], MEASURE['measure'], MEASURE['measure_from'], MEASURE['measure_bins'])
    final, spin, link, esums = lr.walk(cells, ins.Nx, ins.Ny, rot, a['betas'], a['rounds'], a['sweeps'], u['sweep'], bits, a['cluster_from'], a['pairs'],
                                       u['cluster'], u['swap'], nbits, bitcell, ladder.link_table(ins), m['split'], plan, B)
    final['states'] = final['states'][:, ins.order]
    return final, spin, link, esums


@pytest.mark.parametrize('how', ['uniforms', 'seed'])
@pytest.mark.parametrize('pairs_mode', ['all', 'halves'])
@pytest.mark.parametrize('cluster', [False, True], ids=['plain', 'cluster'])
def test_public_call(cluster, pairs_mode, how):
    """ising3x3, T = 3, R = 4, 7 rounds, measure=2, measure_from=1, measure_bins=2 (measurements behind rounds 2, 4, 6; bins 0, 0, 1):
    the histograms, the energy sums and temper_measurements equal temper_ref.run walked round by round with ladder_ref applied at the
    scheduled rounds; states, energy, temper_index and the swap counters are the bits of the same call with measure=None."""
    from tnac4o_amd import ladder
    from tnac4o_amd import temper as tp
    rng = np.random.default_rng(81)
    ins = _fresh('ising3x3')
    start = np.copy(ins.states)
    pairs = None
    if cluster:
        pairs = np.array([[[0, 1], [2, 3]], [[1, 0], [3, 2]]] * 4)[:ROUNDS] if pairs_mode == 'halves' else np.array([rng.permutation(4).reshape(2, 2) for _ in range(ROUNDS)])
    kw = dict(rounds=ROUNDS, sweeps=SWEEPS, cluster_moves=cluster, cluster_beta_min=0.5 if cluster else None, pairs=pairs)
    a = tp.check_arguments(ins, BETAS, ROUNDS, SWEEPS, cluster, kw['cluster_beta_min'], pairs, None, None, None)
    m = ladder.check_arguments(ins, a, MEASURE['measure'], MEASURE['measure_from'], MEASURE['measure_bins'], pairs_mode, True)
    assert m['split'] == (2 if pairs_mode == 'halves' else 0) and m['n_meas'] == 3 and m['B'] == 2
    if how == 'seed':
        rand = dict(seed=1234)
        u = {k: v.cpu().numpy() for k, v in tp.seeded_block(1234, a['shapes'], 0, ROUNDS, torch.device('cuda', torch.cuda.current_device())).items()}
    else:
        u = {k: rng.random(a['shapes'][k]) for k in tp.UNIFORM_KEYS}
        rand = dict(uniforms=u)
    final, spin, link, esums = _walk_solver(ins, start, a, u, m)
    assert final['margin'] >= 1e-9 and final['swap_margin'] >= 1e-9
    ins.temper_samples(BETAS, measure_pairs=pairs_mode, **MEASURE, **rand, **kw)
    assert ins.temper_measurements == 3
    assert ins.temper_overlap_hist.dtype == np.int64 and np.array_equal(ins.temper_overlap_hist.view(np.uint64), spin)
    assert ins.temper_link_hist.dtype == np.int64 and np.array_equal(ins.temper_link_hist.view(np.uint64), link)
    assert same_bits(ins.temper_energy_sums, esums)
    npairs = len(lr.counted_pairs(R_PUB, m['split']))
    assert ins.temper_overlap_hist.sum(axis=2).tolist() == [[2 * npairs] * 3, [npairs] * 3]
    n = spin.shape[2] - 1
    tot = esums.sum(axis=0)
    assert same_bits(ins.temper_energy_mean, tot[:, 1] / (tot[:, 0] * R_PUB))
    e1, e2 = tot[:, 1] / (tot[:, 0] * R_PUB), tot[:, 2] / (tot[:, 0] * R_PUB)
    assert same_bits(ins.temper_heat_capacity, np.array(BETAS) ** 2 * (e2 - e1 * e1) / n)
    want = ladder.moments_of(spin.sum(axis=0).astype(np.float64), link.sum(axis=0).astype(np.float64))
    for k in ladder.MOMENT_KEYS:
        assert same_bits(ins.temper_overlap_moments[k], want[k]) and ins.temper_overlap_errors[k].shape == (3,)
    assert np.array_equal(ins.states, final['states']) and np.array_equal(ins.temper_index, final['tidx'])
    plain = _fresh('ising3x3')
    plain.temper_samples(BETAS, **rand, **kw)
    assert not hasattr(plain, 'temper_overlap_hist') and not hasattr(plain, 'temper_measurements')
    assert np.array_equal(plain.states, ins.states) and same_bits(plain.energy, ins.energy) and np.array_equal(plain.temper_index, ins.temper_index)
    assert np.array_equal(plain.temper_swap_accepted, ins.temper_swap_accepted) and np.array_equal(plain.temper_swap_attempted, ins.temper_swap_attempted)
    other = _fresh('ising3x3')                                           # rounds_per_call cuts further; measure_links=False
    other.temper_samples(BETAS, measure_pairs=pairs_mode, measure_links=False, rounds_per_call=2, **MEASURE, **rand, **kw)
    assert np.array_equal(other.temper_overlap_hist, ins.temper_overlap_hist) and same_bits(other.temper_energy_sums, ins.temper_energy_sums)
    assert other.temper_link_hist is None and np.all(np.isnan(other.temper_overlap_moments['ql'])) and same_bits(other.energy, ins.energy)


def test_public_call_on_chimera_with_pairs_in_halves():
    """The 2 x 2 chimera lattice (8 spins per cell) with pairings drawn by ladder.pairs_in_halves: the reference's histograms."""
    from tnac4o_amd import ladder
    from tnac4o_amd import temper as tp
    rng = np.random.default_rng(83)
    ins = _fresh('chimera', 42)
    start = np.copy(ins.states)
    np.random.seed(5)
    pairs = ladder.pairs_in_halves(ROUNDS, R_PUB)
    a = tp.check_arguments(ins, BETAS, ROUNDS, SWEEPS, True, None, pairs, None, None, None)
    m = ladder.check_arguments(ins, a, 2, 1, 2, 'halves', True)
    u = {k: rng.random(a['shapes'][k]) for k in tp.UNIFORM_KEYS}
    final, spin, link, esums = _walk_solver(ins, start, a, u, m)
    ins.temper_samples(BETAS, rounds=ROUNDS, sweeps=SWEEPS, pairs=pairs, uniforms=u, measure_pairs='halves', **MEASURE)
    assert np.array_equal(ins.temper_overlap_hist.view(np.uint64), spin) and np.array_equal(ins.temper_link_hist.view(np.uint64), link)
    assert same_bits(ins.temper_energy_sums, esums) and np.array_equal(ins.states, final['states'])
    assert spin.shape == (2, 3, 33) and link.shape[2] == len(ladder.link_table(ins)) + 1


def test_public_call_in_the_other_rotation():
    """ising3x3 rotated by 90 degrees with the sweep's uniforms re-indexed to its walk order: the same states, so the histograms are the
    same integers (row positions are model spins in either rotation)."""
    rng = np.random.default_rng(85)
    pairs = np.array([rng.permutation(4).reshape(2, 2) for _ in range(ROUNDS)])
    u = {'sweep': rng.random((ROUNDS, SWEEPS, 9, M_PUB)), 'cluster': rng.random((ROUNDS, 3, 2)), 'swap': rng.random((ROUNDS, 4, 2))}
    a = _fresh('ising3x3', 44)
    b = small('ising3x3', 1.0)
    b.rotate_graph(1)
    b.states = np.copy(a.states)
    ub = dict(u)
    ub['sweep'] = np.empty_like(u['sweep'])
    ub['sweep'][:, :, b.order, :] = u['sweep'][:, :, a.order, :]
    a.temper_samples(BETAS, rounds=ROUNDS, sweeps=SWEEPS, pairs=pairs, uniforms=u, **MEASURE)
    b.temper_samples(BETAS, rounds=ROUNDS, sweeps=SWEEPS, pairs=pairs, uniforms=ub, **MEASURE)
    assert np.array_equal(a.states, b.states) and a.temper_overlap_hist.sum() > 0
    assert np.array_equal(a.temper_overlap_hist, b.temper_overlap_hist) and np.array_equal(a.temper_link_hist, b.temper_link_hist)
    assert np.allclose(a.temper_energy_sums, b.temper_energy_sums, rtol=0, atol=1e-9)


def test_static_chain():
    """sweeps=0, cluster_moves=False, T = 1, 4 rounds, measure=1: nothing moves, and every one of the 4 bins holds its one measurement
    times the pair histogram of the stored rows (popcounts of overlap.spin_bits and link_bits)."""
    from tnac4o_amd import overlap
    ins = _fresh('chimera', 46)
    start = np.copy(ins.states)
    sb, lb = overlap.spin_bits(ins).astype(np.int64), overlap.link_bits(ins).astype(np.int64)
    want = np.zeros(sb.shape[1] + 1, dtype=np.int64)
    lwant = np.zeros(lb.shape[1] + 1, dtype=np.int64)
    for i in range(M_PUB):
        for j in range(i + 1, M_PUB):
            want[np.count_nonzero(sb[i] != sb[j])] += 1
            lwant[np.count_nonzero(lb[i] != lb[j])] += 1
    ins.temper_samples([0.8], rounds=4, sweeps=0, cluster_moves=False, measure=1)
    assert np.array_equal(ins.states, start) and ins.temper_measurements == 4
    assert ins.temper_overlap_hist.shape == (4, 1, sb.shape[1] + 1) and ins.temper_link_hist.shape == (4, 1, lb.shape[1] + 1)
    for b in range(4):
        assert np.array_equal(ins.temper_overlap_hist[b, 0], want) and np.array_equal(ins.temper_link_hist[b, 0], lwant)
    assert same_bits(ins.temper_energy_sums[0], ins.temper_energy_sums[3]) and ins.temper_energy_sums[0, 0, 0] == 1.0
    assert np.all(ins.temper_overlap_errors['q2'] == 0.0) and np.isclose(ins.temper_overlap_P[0] @ ins.temper_overlap_values ** 2, ins.temper_overlap_moments['q2'][0])
