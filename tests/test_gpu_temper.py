"""tn_temper and tnac4o.temper_samples on the GPU against the numpy reference of tests/temper_ref.py: whole calls on the shared inputs
(mixed q with and without maps across the 256-sample tile; the Ising lattice with three sweep classes and 68 bits), cutting the rounds
into calls, T = 1 against tn_cell_sweep, independence of the chains, the edges of the swap rule, states outside their cell, the law
of the chain against the exact joint law, and the public call.  Every buffer of a library call lies between guards."""
import ctypes as ct

import numpy as np
import pytest

import exchange_ref as xr
import relax_ref as rr
import temper_ref as tr
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_relax import DeviceCells, solver_cells, sweep_device      # noqa: E402  (helpers only, no test is imported)
from test_gpu_sampling import dv, small                                 # noqa: E402


# ---------------------------------------------------------------------------------------------- helpers
def _last_error():
    from tnac4o_amd import _lib
    buf = ct.create_string_buffer(512)
    _lib.lib().tn_last_error(buf, 512)
    return buf.value.decode()


def _framed(dtype, array, seed, fill=0x55):
    """A numpy array on the device between guards."""
    array = np.ascontiguousarray(array)
    g = Guarded.of(dtype, array.shape, fill, seed=seed)
    if array.size:
        g.tensor().copy_(dv(array))
    return g


def temper_device(cells, Nx, Ny, betas, states, tidx, slot, round0, rounds, sweeps, usweep=None, bits=None, cluster_from=0, cpairs=None, ucl=None,
                  uswap=None, accepted=None, attempted=None, pad=0, optional=True, lds=None, monkeypatch=None):
    """One call of tn_temper with every buffer between guards; the arguments and the result are those of temper_ref.run.  usweep travels
    with ldu = M + pad, the columns beyond M poisoned with NaN; optional=False passes NULL for the four optional outputs."""
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    betas = np.asarray(betas, dtype=np.float64)
    M, ncell = states.shape
    T = betas.size
    R = M // T
    dc = cells if isinstance(cells, DeviceCells) else DeviceCells(cells)
    nbits = nbmax = nnz = Pc = 0
    Tc = 0
    g_bits = [None] * 4
    if bits is not None:
        nbits, cellbits, bitcell, rowptr, cols = bits
        nbmax, nnz, Tc = cellbits.shape[1], len(cols), T - cluster_from
        g_bits = [_framed(torch.int32, np.asarray(x, dtype=np.int32), 20 + i) for i, x in enumerate((cellbits, bitcell, rowptr, cols))]
        Pc = 0 if cpairs is None else cpairs.shape[1]
    need = int(L.tn_temper_ws_bytes(Nx, Ny, M, T, nbits, Pc))
    assert need > 0
    ws = Guarded(need, 'random', seed=1)
    st = _framed(torch.int16, np.asarray(states).astype(np.int16), 2)
    g_tidx, g_slot = _framed(torch.int32, np.asarray(tidx, dtype=np.int32), 3), _framed(torch.int32, np.asarray(slot, dtype=np.int32).reshape(R, T), 4)
    acc0 = np.zeros(max(T - 1, 0), dtype=np.int32) if accepted is None else np.asarray(accepted, dtype=np.int32)
    att0 = np.zeros(max(T - 1, 0), dtype=np.int32) if attempted is None else np.asarray(attempted, dtype=np.int32)
    g_acc, g_att = _framed(torch.int32, acc0, 5), _framed(torch.int32, att0, 6)
    E = Guarded.of(torch.float64, (M,), 0xFF, seed=7)
    u, ldu = None, 0
    if usweep is not None and rounds * sweeps > 0:
        ldu = M + pad
        u = Guarded.of(torch.float64, (rounds * sweeps * ncell, ldu), 0xFF, seed=8)         # 0xFF bytes: NaN beyond column M
        u.tensor()[:, :M].copy_(dv(np.array(usweep).reshape(-1, M)))
    g_cp = _framed(torch.int32, np.asarray(cpairs, dtype=np.int32), 9) if Pc and rounds else None
    g_ucl = _framed(torch.float64, np.asarray(ucl, dtype=np.float64), 10) if Pc and Tc and rounds else None
    g_us = _framed(torch.float64, np.asarray(uswap, dtype=np.float64), 11) if T > 1 and rounds else None
    et = Guarded.of(torch.float64, (rounds, M), 0xFF, seed=12)
    tt = Guarded.of(torch.int32, (rounds, M), 0x55, seed=13)
    sz = Guarded.of(torch.int32, (rounds, Tc, Pc), 0x55, seed=14)
    df = Guarded.of(torch.int32, (rounds, Tc, Pc), 0x55, seed=15)
    opt = [g.ptr if optional else None for g in (et, tt, sz, df)]
    if lds is not None:
        monkeypatch.setenv('TN_CELL_SWEEP_LDS', str(lds))
    c_betas = (ct.c_double * T)(*betas.tolist())

    def ptr(g):
        return None if g is None else g.ptr

    rc = L.tn_temper(Nx, Ny, dc.ptr, M, T, ct.cast(c_betas, ct.c_void_p), st.ptr, g_tidx.ptr, g_slot.ptr, round0, rounds, sweeps, ptr(u), ldu, nbits, nbmax,
                     ptr(g_bits[0]), ptr(g_bits[1]), ptr(g_bits[2]), ptr(g_bits[3]), nnz, cluster_from, ptr(g_cp), Pc, ptr(g_ucl), ptr(g_us), E.ptr,
                     g_acc.ptr if T > 1 else None, g_att.ptr if T > 1 else None, opt[0], opt[1], opt[2], opt[3], ws.ptr, need, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, _last_error())
    for g in [ws, st, g_tidx, g_slot, g_acc, g_att, E, et, tt, sz, df] + [x for x in [u, g_cp, g_ucl, g_us] + g_bits if x is not None]:
        assert g.intact()
    if not optional:
        assert et.untouched(0xFF) and tt.untouched(0x55) and sz.untouched(0x55) and df.untouched(0x55)
    return dict(states=st.host().astype(np.int64), tidx=g_tidx.host().astype(np.int64), slot=g_slot.host().astype(np.int64), energy=E.host(),
                energy_trace=et.host(), tidx_trace=tt.host().astype(np.int64), accepted=g_acc.host().astype(np.int64),
                attempted=g_att.host().astype(np.int64), sizes=sz.host().astype(np.int64), differing=df.host().astype(np.int64))


def device_case(c, lo=0, hi=None, round0=0, state=None, dc=None, **kw):
    """temper_device on the rounds lo .. hi - 1 of a case's inputs, from `state` = a previous result (None: the case's start)."""
    hi = c['usweep'].shape[0] if hi is None else hi
    s = state or dict(states=c['states'], tidx=c['tidx'], slot=c['slot'], accepted=None, attempted=None)
    return temper_device(dc or c['cells'], c['Nx'], c['Ny'], c['betas'], s['states'], s['tidx'], s['slot'], round0 + lo, hi - lo, tr.SWEEPS, c['usweep'][lo:hi],
                         c['bits'], c['cluster_from'], c['cpairs'][lo:hi], c['ucl'][lo:hi], c['uswap'][lo:hi], s['accepted'], s['attempted'], **kw)


FINAL = ('states', 'tidx', 'slot', 'accepted', 'attempted')
TRACES = ('tidx_trace', 'sizes', 'differing')


def assert_same_call(got, ref, traces=True):
    for k in FINAL + (TRACES if traces else ()):
        assert np.array_equal(got[k], ref[k]), k
    assert same_bits(got['energy'], ref['energy'])
    if traces:
        assert same_bits(got['energy_trace'], ref['energy_trace'])


# ---------------------------------------------------------------------------------------------- 1. whole calls against the reference
@pytest.mark.parametrize('case', tr.CASES, ids=tr.CASE_IDS)
def test_call_against_the_reference(case, monkeypatch):
    """4 rounds of 2 sweeps on every shared input: states, tidx, slot, counters, tidx_trace, size_out and diff_out equal, energy_out and
    energy_trace in the reference's bits; ldu > M with NaN beyond column M; guards intact; the optional outputs NULL; the same bits with
    no table staged in LDS (TN_CELL_SWEEP_LDS=0) and with every table that fits 150 KiB staged."""
    c = tr.case_inputs(case)
    ref = tr.case_reference(case)
    dc = DeviceCells(c['cells'])
    got = device_case(c, dc=dc, pad=3)
    assert_same_call(got, ref)
    assert tr.assignment_consistent(got['tidx'], got['slot'])
    assert_same_call(device_case(c, dc=dc, optional=False), ref, traces=False)
    for lds in (0, 150 * 1024):
        assert_same_call(device_case(c, dc=dc, pad=1, lds=lds, monkeypatch=monkeypatch), ref)


# ---------------------------------------------------------------------------------------------- 2. cutting the rounds into calls
@pytest.mark.parametrize('case', [tr.CASES[0], tr.CASES[-1]], ids=[tr.CASE_IDS[0], tr.CASE_IDS[-1]])
def test_cutting_rounds(case):
    """6 rounds as one call and as calls of 1 + 2 + 3 rounds with round0 advanced and tidx, slot and the counters carried over: everything
    identical, counters and traces included."""
    c = tr.case_inputs(case, 6)
    dc = DeviceCells(c['cells'])
    whole = device_case(c, dc=dc)
    assert_same_call(whole, tr.run_case(c))
    parts, state = [], None
    for lo, hi in ((0, 1), (1, 3), (3, 6)):
        state = device_case(c, lo=lo, hi=hi, state=state, dc=dc)
        parts.append(state)
    assert_same_call(state, whole, traces=False)
    for k in TRACES + ('energy_trace',):
        assert same_bits(np.concatenate([p[k] for p in parts]), whole[k]), k


# ---------------------------------------------------------------------------------------------- 3. T = 1 is tn_cell_sweep
def test_one_temperature_is_cell_sweep():
    """T = 1, nbits = 0: states and energies equal those of tn_cell_sweep on the same inputs at that beta, bit for bit (2 rounds of 2
    sweeps = 4 sweeps; 300 rows: two tiles); uswap and the counters NULL."""
    case = rr.CASES[[c[:3] for c in rr.CASES].index(('3x3', True, 300))]
    Ny, Nx, cells, states, _ = rr.case_inputs(case)
    M = states.shape[0]
    u = np.random.default_rng(5).random((2, 2, len(cells), M))
    dc = DeviceCells(cells)
    want = sweep_device(dc, Nx, Ny, states, 0, 4, rr.BETA, u.reshape(4, len(cells), M))
    tidx, slot = tr.fresh_assignment(M, 1)
    got = temper_device(dc, Nx, Ny, [rr.BETA], states, tidx, slot, 0, 2, 2, u)
    assert np.array_equal(got['states'], want['states']) and same_bits(got['energy'], want['energy'])
    assert not np.array_equal(got['states'], states) and np.all(got['tidx'] == 0) and np.array_equal(got['slot'].ravel(), np.arange(M))
    assert same_bits(got['energy_trace'][1], want['energy'])


# ---------------------------------------------------------------------------------------------- 4. the chains are independent
def test_chains_are_independent_without_cluster_moves():
    """nbits = 0: chains of the first shared input computed alone (R = 1), as a group of three, and embedded among other chains at other
    places give the bits they have in the whole call."""
    case = tr.CASES[0]
    c, ref = tr.case_inputs(case), tr.case_reference(case)
    dc = DeviceCells(c['cells'])
    T = c['betas'].size

    def run(st, us, uw):
        tidx, slot = tr.fresh_assignment(st.shape[0], T)
        return temper_device(dc, c['Nx'], c['Ny'], c['betas'], st, tidx, slot, 0, tr.ROUNDS, tr.SWEEPS, us, uswap=uw)

    def chains(which):
        rows = np.concatenate([np.arange(k * T, (k + 1) * T) for k in which])
        return run(c['states'][rows], c['usweep'][:, :, :, rows], c['uswap'][:, which]), rows

    for which in ([0], [64], [7, 33, 64]):
        got, rows = chains(which)
        assert np.array_equal(got['states'], ref['states'][rows]) and same_bits(got['energy'], ref['energy'][rows])
        assert np.array_equal(got['tidx'], ref['tidx'][rows]) and same_bits(got['energy_trace'], ref['energy_trace'][:, rows])
    rng = np.random.default_rng(9)                                       # chains 7 and 33 at the places 2 and 5 of eight chains
    qs = np.array([cell['q'] for cell in c['cells']])
    which, place = [7, 33], [2, 5]
    st = rng.integers(0, qs[None, :], size=(8 * T, qs.size))
    us, uw = rng.random((tr.ROUNDS, tr.SWEEPS, qs.size, 8 * T)), rng.random((tr.ROUNDS, 8, T - 1))
    for k, pl in zip(which, place):
        st[pl * T:(pl + 1) * T] = c['states'][k * T:(k + 1) * T]
        us[:, :, :, pl * T:(pl + 1) * T] = c['usweep'][:, :, :, k * T:(k + 1) * T]
        uw[:, pl] = c['uswap'][:, k]
    got = run(st, us, uw)
    for k, pl in zip(which, place):
        a, b = slice(pl * T, (pl + 1) * T), slice(k * T, (k + 1) * T)
        assert np.array_equal(got['states'][a], ref['states'][b]) and same_bits(got['energy'][a], ref['energy'][b])
        assert np.array_equal(got['tidx'][a], ref['tidx'][b])


# ---------------------------------------------------------------------------------------------- 5. the edges of the swap rule
def _two_temperatures(R, seed, maps=True):
    Ny, Nx, qs = rr.LATTICES['2x2']
    cells = rr.make_cells(Ny, Nx, qs, maps, seed)
    rng = np.random.default_rng(seed + 1)
    states = rng.integers(0, np.asarray(qs)[None, :], size=(2 * R, len(qs)))
    return cells, Nx, Ny, np.array([0.4, 1.1]), states, rng


def test_swap_edges():
    """T = 2 at odd parity: nothing swaps and nothing is counted.  D >= 0 with u = nextafter(1, 0): accepted (D = 0, two equal rows,
    included), while D < 0 with that u is refused.  sweeps = 0 moves no state; rounds = 0 writes energy_out only; Pc = 0 and cluster_from
    = T make no cluster move."""
    R = 9
    cells, Nx, Ny, betas, states, rng = _two_temperatures(R, 77)
    states[2] = states[3]                                                # chain 1: two equal rows, D = 0
    dc = DeviceCells(cells)
    tidx, slot = tr.fresh_assignment(2 * R, 2)
    E0 = rr.total_energy(cells, Nx, Ny, states)
    top = np.full((1, R, 1), xr.U_MAX)
    odd = temper_device(dc, Nx, Ny, betas, states, tidx, slot, 1, 1, 0, uswap=np.zeros((1, R, 1)), accepted=[5], attempted=[11])
    assert np.array_equal(odd['tidx'], tidx) and np.array_equal(odd['slot'], slot) and odd['accepted'][0] == 5 and odd['attempted'][0] == 11
    assert np.array_equal(odd['states'], states) and same_bits(odd['energy'], E0) and same_bits(odd['energy_trace'][0], E0)
    even = temper_device(dc, Nx, Ny, betas, states, tidx, slot, 0, 1, 0, uswap=top, accepted=[5], attempted=[11])
    delta = (betas[1] - betas[0]) * (E0[1::2] - E0[0::2])
    assert delta[1] == 0.0 and np.any(delta > 0) and np.any(delta < 0)
    assert np.array_equal(even['tidx'][0::2], (delta >= 0).astype(np.int64)) and np.array_equal(even['tidx'][1::2], (delta < 0).astype(np.int64))
    assert even['accepted'][0] == 5 + np.count_nonzero(delta >= 0) and even['attempted'][0] == 11 + R
    assert tr.assignment_consistent(even['tidx'], even['slot']) and np.array_equal(even['states'], states)
    ref = tr.run(cells, Nx, Ny, states, betas, tidx, slot, 0, 1, 0, uswap=top, accepted=[5], attempted=[11])
    assert_same_call(even, ref)
    low = temper_device(dc, Nx, Ny, betas, states, tidx, slot, 0, 1, 0, uswap=np.zeros((1, R, 1)))      # u = 0: every swap is accepted
    assert np.all(low['tidx'][0::2] == 1) and low['accepted'][0] == R
    none = temper_device(dc, Nx, Ny, betas, states, tidx, slot, 0, 0, 2)                                # rounds = 0
    assert np.array_equal(none['states'], states) and same_bits(none['energy'], E0) and np.array_equal(none['tidx'], tidx)
    assert np.all(none['accepted'] == 0) and np.all(none['attempted'] == 0)
    # the Ising lattice without a pair, and with no temperature that makes cluster moves: the sweeps and swaps of the reference
    c = tr.case_inputs(tr.CASES[-1])
    M, T = c['states'].shape[0], c['betas'].size
    for cluster_from, cpairs, ucl in ((1, np.zeros((tr.ROUNDS, 0, 2), dtype=np.int32), np.zeros((tr.ROUNDS, T - 1, 0))),
                                      (T, c['cpairs'], np.zeros((tr.ROUNDS, 0, c['cpairs'].shape[1])))):
        args = (c['cells'], c['Nx'], c['Ny'], c['states'], c['betas'], c['tidx'], c['slot'], 0, tr.ROUNDS, tr.SWEEPS, c['usweep'], c['bits'], cluster_from,
                cpairs, ucl, c['uswap'])
        got = temper_device(args[0], args[1], args[2], args[4], args[3], *args[5:])
        ref = tr.run(*args)
        assert_same_call(got, ref)
        plain = tr.run(*args[:11], uswap=c['uswap'])
        assert np.array_equal(got['states'], plain['states']) and same_bits(got['energy'], plain['energy'])


def test_a_nan_energy_never_swaps():
    """A NaN entry of Es at a state some rows hold: their energy is NaN, D is NaN, and the swap is refused even at u = 0, in either
    position of the pair; the other chains swap.  The rows hold that state on entry and sweeps = 0: a heat-bath sweep cannot pick a state
    whose weight is NaN (w > 0 fails), so no sweep's uniform numbers can lead there."""
    R = 6
    cells, Nx, Ny, betas, states, rng = _two_temperatures(R, 78)
    cells = [dict(cell) for cell in cells]
    cells[1]['Es'] = cells[1]['Es'].copy()
    cells[1]['Es'][5] = np.nan
    states[:, 1] = np.where(states[:, 1] == 5, 6, states[:, 1])
    states[0, 1] = 5                                                     # chain 0: the NaN row at temperature 0
    states[3, 1] = 5                                                     # chain 1: at temperature 1
    tidx, slot = tr.fresh_assignment(2 * R, 2)
    got = temper_device(cells, Nx, Ny, betas, states, tidx, slot, 0, 1, 0, uswap=np.zeros((1, R, 1)))
    assert np.isnan(got['energy'][[0, 3]]).all() and np.isfinite(np.delete(got['energy'], [0, 3])).all()
    assert got['tidx'][:4].tolist() == [0, 1, 0, 1] and np.all(got['tidx'][4::2] == 1) and np.all(got['tidx'][5::2] == 0)
    assert got['accepted'][0] == R - 2 and got['attempted'][0] == R
    ref = tr.run(cells, Nx, Ny, states, betas, tidx, slot, 0, 1, 0, uswap=np.zeros((1, R, 1)))
    for k in FINAL:
        assert np.array_equal(got[k], ref[k]), k


# ---------------------------------------------------------------------------------------------- 6. states outside their cell
def test_states_outside_their_cell():
    """States q, -1 and 32767 in the input: never an index (guards intact); the sweeps treat them by tn_cell_sweep's rule and leave every
    state inside; with sweeps = 0 on the Ising lattice the conversion reads them as 0 and rewrites only the cells a cluster changed."""
    case = tr.CASES[0]
    c = tr.case_inputs(case)
    qs = np.array([cell['q'] for cell in c['cells']])
    bad = c['states'].copy()
    for m, k, v in ((0, 4, qs[4]), (1, 0, -1), (2, 8, qs[8]), (3, 3, -1), (3, 4, qs[4]), (5, 1, 32767), (259, 7, -32768)):
        bad[m, k] = v
    args = (c['cells'], c['Nx'], c['Ny'], bad, c['betas'], c['tidx'], c['slot'], 0, 2, tr.SWEEPS, c['usweep'][:2])
    got = temper_device(args[0], args[1], args[2], args[4], args[3], *args[5:], uswap=c['uswap'][:2])
    ref = tr.run(*args, uswap=c['uswap'][:2])
    assert_same_call(got, ref)
    assert np.all(np.isfinite(got['energy'])) and np.all((got['states'] >= 0) & (got['states'] < qs[None, :]))
    b = tr.case_inputs(tr.CASES[-1])
    qs = np.array([cell['q'] for cell in b['cells']])
    bad = b['states'].copy()
    for m, k, v in ((0, 3, 256), (3, 0, -1), (7, 2, 32), (10, 5, 32767), (13, 15, 300), (16, 1, 8)):
        bad[m, k] = v
    args = (b['cells'], b['Nx'], b['Ny'], bad, b['betas'], b['tidx'], b['slot'], 0, 2, 0, None, b['bits'], b['cluster_from'], b['cpairs'][:2], b['ucl'][:2],
            b['uswap'][:2])
    got = temper_device(args[0], args[1], args[2], args[4], args[3], *args[5:])
    ref = tr.run(*args)
    assert_same_call(got, ref)
    assert np.any(got['states'] != bad)


# ---------------------------------------------------------------------------------------------- 7. the law
def test_law_of_the_chain():
    """relax_ref.law_problem(), T = 2, R = 2^14 independent chains from uniformly random states, 3 rounds of one sweep: the empirical law
    of the rows at each temperature index against the exact marginals of the joint law advanced by the host recursion (no mixing
    assumption); bins with M p < 20 pooled, every bin within 6 sigma.  tests/test_temper_host.py shows that the reference chain passes."""
    cells, betas, states, usweep, uswap, marginals = tr.law_inputs()
    tidx, slot = tr.fresh_assignment(states.shape[0], 2)
    got = temper_device(cells, 2, 2, betas, states, tidx, slot, 0, tr.LAW_ROUNDS, 1, usweep, uswap=uswap, optional=False)
    for t, (ok, z, bins) in enumerate(tr.law_check(got['states'], got['tidx'], marginals)):
        print('temperature %d: largest deviation %.2f sigma over %d bins' % (t, z, bins))
        assert ok
    ref = tr.run(cells, 2, 2, states, betas, tidx, slot, 0, tr.LAW_ROUNDS, 1, usweep, uswap=uswap)
    assert np.array_equal(got['states'], ref['states']) and np.array_equal(got['tidx'], ref['tidx']) and np.array_equal(got['accepted'], ref['accepted'])


# ---------------------------------------------------------------------------------------------- 8. the public call
def _random_states(ins, M, seed):
    qs = ins._cell_sizes()[ins.order]                                    # model order
    return np.random.default_rng(seed).integers(0, qs[None, :], size=(M, qs.size))


def _reference_call(ins, start, a, uniforms):
    """temper_ref.run on a solver: the lattice from the solver's own host tables (solver_cells), the bit tables and the CSR from the
    package's host functions, rows in the device's order."""
    from tnac4o_amd import exchange as ex
    from tnac4o_amd import temper as tp
    cells = solver_cells(ins)
    bits = (tp.bit_tables(ins) + ex.coupling_csr(ins)) if a['cluster'] else None
    rot = np.empty_like(start)
    rot[:, ins.order] = start
    tidx, slot = tr.fresh_assignment(a['M'], a['T'])
    ref = tr.run(cells, ins.Nx, ins.Ny, rot, a['betas'], tidx, slot, 0, a['rounds'], a['sweeps'], uniforms['sweep'], bits, a['cluster_from'], a['pairs'],
                 uniforms['cluster'], uniforms['swap'])
    ref['states'] = ref['states'][:, ins.order]
    return ref


PUBLIC = [('ising3x3', True), ('chimera', True), ('rmf3x3', False)]


@pytest.mark.parametrize('name,cluster', PUBLIC, ids=[p[0] for p in PUBLIC])
def test_public_call(name, cluster):
    """24 random states, T = 3, 4 rounds of 2 sweeps with given pairs and uniforms (cluster moves at the two upper betas): the reference's
    states, temper_index, counters and traces; energy in the bits of relax_native(..., mode=1, sweeps=0) on the final states; what is
    stored and what is left alone; keep=t slices consistently; rounds_per_call in {1, 2, None} and uniforms on the device give the same
    result."""
    from tnac4o_amd import relax
    from tnac4o_amd import temper as tp
    betas = [0.3, 0.7, 1.2]
    M, T, R, rounds, sweeps = 24, 3, 8, 4, 2
    rng = np.random.default_rng(41)

    def fresh():
        ins = small(name, 1.0)
        ins.states = _random_states(ins, M, 40)
        return ins

    ins = fresh()
    start = np.copy(ins.states)
    ncell = ins.Nx * ins.Ny
    pairs = np.array([rng.permutation(R)[:6].reshape(3, 2) for _ in range(rounds)]) if cluster else None
    kw = dict(rounds=rounds, sweeps=sweeps, cluster_moves=cluster, cluster_beta_min=0.5 if cluster else None, pairs=pairs)
    a = tp.check_arguments(ins, betas, rounds, sweeps, cluster, kw['cluster_beta_min'], pairs, None, None, None)
    u = {k: rng.random(a['shapes'][k]) for k in tp.UNIFORM_KEYS}
    assert a['cluster_from'] == (1 if cluster else 3) and u['cluster'].shape == ((rounds, 2, 3) if cluster else (rounds, 0, 0))
    ref = _reference_call(ins, start, a, u)
    assert ref['margin'] >= 1e-9 and ref['swap_margin'] >= 1e-9
    ins.degeneracy = 5
    ins.probability = np.zeros(M)
    E = ins.temper_samples(betas, uniforms=u, record=True, **kw)
    assert not hasattr(ins, 'rhoT') and ins.degeneracy == 5
    assert E is ins.energy and np.array_equal(ins.states, ref['states']) and not np.array_equal(ins.states, start)
    assert np.array_equal(ins.temper_index, ref['tidx']) and same_bits(ins.temper_beta, np.array(betas)[ref['tidx']])
    assert same_bits(ins.temper_betas, np.array(betas))
    assert np.array_equal(ins.temper_swap_accepted, ref['accepted']) and np.array_equal(ins.temper_swap_attempted, ref['attempted'])
    assert ins.temper_swap_attempted.tolist() == [2 * R, 2 * R]
    assert same_bits(ins.temper_energy_trace, tp.reorder_trace(ref['energy_trace'], ref['tidx_trace'], T)) and ins.temper_energy_trace.shape == (rounds, T, R)
    assert np.array_equal(ins.temper_cluster_sizes, ref['sizes']) and np.array_equal(ins.temper_cluster_differing, ref['differing'])
    rot = np.empty_like(ins.states)
    rot[:, ins.order] = ins.states
    assert same_bits(ins.energy, relax.relax_native(fresh(), rot, 1, 1.0, 0)[1])
    assert ins.probability is None and ins.sample_log2Z is None and ins.log2Z_lower is None and ins.log2Z_estimate is None
    for per, dev_u in ((1, False), (2, True), (None, False)):
        other = fresh()
        uu = {k: torch.as_tensor(v).cuda() for k, v in u.items()} if dev_u else u
        other.temper_samples(betas, uniforms=uu, rounds_per_call=per, record=True, **kw)
        assert np.array_equal(other.states, ins.states) and same_bits(other.energy, ins.energy) and np.array_equal(other.temper_index, ins.temper_index)
        assert np.array_equal(other.temper_swap_accepted, ins.temper_swap_accepted) and same_bits(other.temper_energy_trace, ins.temper_energy_trace)
        assert np.array_equal(other.temper_cluster_sizes, ins.temper_cluster_sizes)
        assert other.temper_cluster_sizes.shape == u['cluster'].shape
    kept = fresh()
    kept.temper_samples(betas, uniforms=u, keep=2, **kw)
    rows = np.flatnonzero(ins.temper_index == 2)
    assert rows.size == R and np.array_equal(rows // T, np.arange(R))
    assert np.array_equal(kept.states, ins.states[rows]) and same_bits(kept.energy, ins.energy[rows]) and np.array_equal(kept.temper_index, ins.temper_index)
    assert not hasattr(kept, 'temper_energy_trace')
    # no round: nothing moves, the energies are there
    idle = fresh()
    idle.temper_samples(betas, rounds=0, cluster_moves=cluster)
    assert np.array_equal(idle.states, start) and np.array_equal(idle.temper_index, np.arange(M) % T) and np.all(idle.temper_swap_attempted == 0)
    assert same_bits(idle.energy, relax.relax_native(fresh(), np.asarray(start)[:, np.argsort(ins.order)], 1, 1.0, 0)[1])


def test_public_call_in_the_other_rotation():
    """ising3x3 rotated by 90 degrees gives the same model-order result for the same uniforms re-indexed to its walk order: the number
    of (round, sweep, model cell k, row) sits at cell index ins.order[k] of uniforms['sweep'], as relax_samples' uniforms do.  (On a
    3 x 3 lattice the rotation keeps the checkerboard colours; the energies agree to rounding, their additions run in another order.)"""
    betas = [0.3, 0.7, 1.2]
    M, rounds, sweeps = 12, 4, 2
    rng = np.random.default_rng(43)
    pairs = np.array([rng.permutation(4).reshape(2, 2) for _ in range(rounds)])
    u = {'sweep': rng.random((rounds, sweeps, 9, M)), 'cluster': rng.random((rounds, 3, 2)), 'swap': rng.random((rounds, 4, 2))}
    a = small('ising3x3', 1.0)
    a.states = _random_states(a, M, 44)
    b = small('ising3x3', 1.0)
    b.rotate_graph(1)
    b.states = np.copy(a.states)
    ub = dict(u)
    ub['sweep'] = np.empty_like(u['sweep'])
    ub['sweep'][:, :, b.order, :] = u['sweep'][:, :, a.order, :]
    a.temper_samples(betas, rounds=rounds, sweeps=sweeps, pairs=pairs, uniforms=u, record=True)
    b.temper_samples(betas, rounds=rounds, sweeps=sweeps, pairs=pairs, uniforms=ub, record=True)
    assert np.array_equal(a.states, b.states) and np.array_equal(a.temper_index, b.temper_index)
    assert np.array_equal(a.temper_swap_accepted, b.temper_swap_accepted) and np.array_equal(a.temper_cluster_sizes, b.temper_cluster_sizes)
    assert np.allclose(a.energy, b.energy, rtol=0, atol=1e-12) and np.allclose(a.temper_energy_trace, b.temper_energy_trace, rtol=0, atol=1e-12)


def test_public_call_refusals_and_the_global_generator():
    """RMF with cluster_moves=True is a ValueError; with uniforms=None the numbers come from numpy's global generator: all pairings,
    then per block sweep, cluster, swap."""
    r = small('rmf3x3', 1.0)
    r.states = _random_states(r, 8, 1)
    with pytest.raises(ValueError, match='Ising'):
        r.temper_samples([0.5, 1.0], cluster_moves=True)
    from tnac4o_amd import exchange as ex
    from tnac4o_amd import temper as tp
    ins = small('chimera', 1.0)
    ins.states = _random_states(ins, 8, 2)
    start = np.copy(ins.states)
    np.random.seed(17)
    ins.temper_samples([0.5, 1.0], rounds=3, rounds_per_call=2)
    np.random.seed(17)
    pairs = ex.check_pairs(None, 3, 4)
    shapes = tp.uniform_shapes(3, 1, 4, 8, 2, 2, 2)
    blocks = [tp.draw_block(shapes, 0, 2), tp.draw_block(shapes, 2, 3)]
    u = {k: np.concatenate([blk[k] for blk in blocks]) for k in tp.UNIFORM_KEYS}
    other = small('chimera', 1.0)
    other.states = start
    other.temper_samples([0.5, 1.0], rounds=3, pairs=pairs, uniforms=u)
    assert np.array_equal(other.states, ins.states) and same_bits(other.energy, ins.energy) and np.array_equal(other.temper_index, ins.temper_index)
