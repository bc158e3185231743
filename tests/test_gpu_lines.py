"""tn_line_sweep and tnac4o.relax_lines on the GPU against the numpy reference of tests/lines_ref.py: the kernel on synthetic tables
(every lattice edge, mixed q, with and without the Ising maps, transfer tables built once and evaluated in place), rows and columns
alone, a heat bath close to the range guard, slicing, states outside their cell, the error contract, the public call on the solvers of
the sampling tests, the law of the chain against the exact mu0 P^k, and the fixed points of the line quench."""
import ctypes as ct

import numpy as np
import pytest

import lines_ref as lr
import relax_ref as rr
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_relax import DeviceCells, _last_error, make, model_energy      # noqa: E402  (helpers only, no test is imported)
from test_gpu_sampling import dv                                             # noqa: E402

LINES = {'rows': 0, 'columns': 1, 'both': 2}


# ---------------------------------------------------------------------------------------------- helpers
def line_device(cells, Nx, Ny, states, mode, sweeps, lines='both', beta=1.0, uniforms=None, pad=0, want_rc=0, tables=None, monkeypatch=None):
    """One call of tn_line_sweep with every buffer between guards: dict(rc, states, energy, moves, last_moves).  uniforms
    (sweeps, P, ncell, M) travel with ldu = M + pad, the columns beyond M poisoned with NaN."""
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    M, ncell = states.shape
    dc = cells if isinstance(cells, DeviceCells) else DeviceCells(cells)
    need = int(L.tn_line_sweep_ws_bytes(Nx, Ny, M))
    assert need > 0
    ws = Guarded(need, 0xA5, seed=1)
    st = Guarded.of(torch.int16, (M, ncell), 0xFF, seed=2)
    st.tensor().copy_(dv(np.asarray(states).astype(np.int16)))
    E = Guarded.of(torch.float64, (M,), 0xFF, seed=3)
    mv = Guarded.of(torch.int32, (M,), 0xFF, seed=4)
    lm = Guarded.of(torch.int32, (M,), 0xFF, seed=5)
    u, ldu = None, 0
    if uniforms is not None:
        ldu = M + pad
        u = Guarded.of(torch.float64, (int(np.prod(uniforms.shape[:-1])), ldu), 0xFF, seed=6)     # 0xFF bytes: NaN beyond column M
        if u.nbytes:
            u.tensor()[:, :M].copy_(dv(np.array(uniforms).reshape(-1, M)))
    if tables is not None:
        monkeypatch.setenv('TN_LINE_SWEEP_TABLES', str(tables))
    rc = L.tn_line_sweep(Nx, Ny, dc.ptr, M, st.ptr, mode, LINES[lines], beta, sweeps, u.ptr if u is not None else None, ldu, E.ptr, mv.ptr, lm.ptr,
                         ws.ptr, need, ops._stream())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _last_error())
    for g in (ws, st, E, mv, lm) + ((u,) if u is not None else ()):
        assert g.intact()
    return dict(rc=rc, states=st.host().astype(np.int64), energy=E.host(), moves=mv.host().astype(np.int64),
                last_moves=lm.host().astype(np.int64))


def assert_same_run(got, ref):
    assert np.array_equal(got['states'], ref['states'])
    assert same_bits(got['energy'], ref['energy'])
    assert np.array_equal(got['moves'], ref['moves']) and np.array_equal(got['last_moves'], ref['last_moves'])


def case(name):
    return lr.CASES[lr.CASE_IDS.index(name)]


# ---------------------------------------------------------------------------------------------- 1. kernel on synthetic tables
@pytest.mark.parametrize('case', lr.CASES, ids=lr.CASE_IDS)
def test_kernel_against_the_reference(case, monkeypatch):
    """2 heat-bath sweeps and 3 quench sweeps of rows and columns on every shared case: the reference's states, the bits of its
    energies, its move counts; sweeps = 0 returns the states untouched and their energies; ldu > M with NaN beyond column M; guards
    intact.  With no transfer table built in the workspace (TN_LINE_SWEEP_TABLES=0) the same bits as with all of them."""
    Ny, Nx, cells, states, uniforms = lr.case_inputs(case)
    dc = DeviceCells(cells)
    heat = line_device(dc, Nx, Ny, states, 0, lr.HEAT_SWEEPS, 'both', lr.BETA, uniforms, pad=3)
    assert_same_run(heat, lr.case_reference(case, 0))
    quench = line_device(dc, Nx, Ny, states, 1, lr.QUENCH_SWEEPS)
    assert_same_run(quench, lr.case_reference(case, 1))
    none = line_device(dc, Nx, Ny, states, 1, 0)
    assert np.array_equal(none['states'], states) and same_bits(none['energy'], rr.total_energy(cells, Nx, Ny, states))
    assert np.all(none['moves'] == 0) and np.all(none['last_moves'] == 0)
    none = line_device(dc, Nx, Ny, states, 0, 0, 'both', lr.BETA, uniforms[:0], pad=1)
    assert np.array_equal(none['states'], states) and same_bits(none['energy'], rr.total_energy(cells, Nx, Ny, states))
    inplace = line_device(dc, Nx, Ny, states, 0, lr.HEAT_SWEEPS, 'both', lr.BETA, uniforms, pad=3, tables=0, monkeypatch=monkeypatch)
    for key in ('states', 'energy', 'moves', 'last_moves'):
        assert same_bits(inplace[key], heat[key]), key
    inplace = line_device(dc, Nx, Ny, states, 1, lr.QUENCH_SWEEPS, tables=0, monkeypatch=monkeypatch)
    for key in ('states', 'energy', 'moves', 'last_moves'):
        assert same_bits(inplace[key], quench[key]), key


ALONE = ['3x3-maps-M65', '3x3-nomaps-M65', '1x3-maps-M65', '1x3-nomaps-M65', '3x1-maps-M65', '3x1-nomaps-M65']


@pytest.mark.parametrize('lines', ['rows', 'columns'])
@pytest.mark.parametrize('name', ALONE)
def test_rows_and_columns_alone(name, lines):
    """lines = 0 and lines = 1 (one pass per sweep; pass 0 of the case's uniforms), on lattices that have a line of one cell too."""
    Ny, Nx, cells, states, uniforms = lr.case_inputs(case(name))
    dc = DeviceCells(cells)
    ref = lr.case_reference(case(name), 0, lines)
    assert ref['margin'] >= lr.MARGIN_FLOOR
    assert_same_run(line_device(dc, Nx, Ny, states, 0, lr.HEAT_SWEEPS, lines, lr.BETA, uniforms[:, :1], pad=2), ref)
    assert_same_run(line_device(dc, Nx, Ny, states, 1, lr.QUENCH_SWEEPS, lines), lr.case_reference(case(name), 1, lines))


def test_move_outputs_may_be_null():
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    Ny, Nx, cells, states, uniforms = lr.case_inputs(case('3x3-maps-M65'))
    dc = DeviceCells(cells)
    M = states.shape[0]
    need = int(L.tn_line_sweep_ws_bytes(Nx, Ny, M))
    ws = Guarded(need, 0xFF, seed=1)
    st, u = dv(states.astype(np.int16)), dv(np.array(uniforms))
    E = Guarded.of(torch.float64, (M,), 0xFF, seed=3)
    rc = L.tn_line_sweep(Nx, Ny, dc.ptr, M, st.data_ptr(), 0, 2, lr.BETA, lr.HEAT_SWEEPS, u.data_ptr(), M, E.ptr, None, None, ws.ptr, need, ops._stream())
    torch.cuda.synchronize()
    ref = lr.case_reference(case('3x3-maps-M65'), 0)
    assert rc == 0 and ws.intact() and E.intact()
    assert np.array_equal(st.cpu().numpy(), ref['states']) and same_bits(E.host(), ref['energy'])


def test_heat_bath_close_to_the_range_guard(monkeypatch):
    """beta x (range of a chain table) = 250: the linear-domain messages stay far from underflow; the reference's states."""
    Ny, Nx, cells, beta, states, u = lr.steep_inputs()
    assert 200.0 <= beta * lr.chain_ranges(cells, Nx, Ny, 'both') <= 300.0
    ref = lr.run(cells, Nx, Ny, states, 0, 1, 'both', beta, u)
    assert ref['margin'] >= lr.MARGIN_FLOOR
    got = line_device(cells, Nx, Ny, states, 0, 1, 'both', beta, u, pad=1)
    assert_same_run(got, ref)
    assert_same_run(line_device(cells, Nx, Ny, states, 0, 1, 'both', beta, u, tables=0, monkeypatch=monkeypatch), ref)


# ---------------------------------------------------------------------------------------------- 2. slicing
@pytest.mark.parametrize('mode', [0, 1])
def test_slicing(mode):
    """The first 65 samples of the M = 300 run equal the M = 65 run on the same columns; so do chunks of 7 and the samples embedded at
    offset 123 among others: identical bits per sample."""
    Ny, Nx, cells, states, uniforms = lr.case_inputs(case('3x3-maps-M300'))
    dc = DeviceCells(cells)
    sweeps = lr.HEAT_SWEEPS if mode == 0 else lr.QUENCH_SWEEPS
    u = uniforms if mode == 0 else None
    whole = line_device(dc, Nx, Ny, states, mode, sweeps, 'both', lr.BETA, u, pad=2)
    assert_same_run(whole, lr.case_reference(case('3x3-maps-M300'), mode))
    for lo, hi in [(0, 65)] + [(lo, lo + 7) for lo in range(65, 300, 47)]:
        part = line_device(dc, Nx, Ny, states[lo:hi], mode, sweeps, 'both', lr.BETA, None if u is None else u[..., lo:hi])
        for key in ('states', 'energy', 'moves', 'last_moves'):
            assert same_bits(part[key], whole[key][lo:hi]), (lo, key)
    rng = np.random.default_rng(8)
    qs = np.array([c['q'] for c in cells])
    big = rng.integers(0, qs[None, :], size=(700, qs.size))
    big[123:423] = states
    ub = None
    if mode == 0:
        ub = rng.random((sweeps, 2, qs.size, 700))
        ub[..., 123:423] = uniforms
    emb = line_device(dc, Nx, Ny, big, mode, sweeps, 'both', lr.BETA, ub, pad=5)
    for key in ('states', 'energy', 'moves', 'last_moves'):
        assert same_bits(emb[key][123:423], whole[key]), key


# ---------------------------------------------------------------------------------------------- 3. states outside their cell
def test_states_outside_their_cell():
    """States q and -1 in a few samples of the 3 x 3 lattice: never an index (guards intact, finite energies); as neighbours they are
    read as 0, in a quench the energy of their line counts as +inf -- the reference's rules -- and a sweep over every line leaves every
    state inside."""
    Ny, Nx, cells, states, uniforms = lr.case_inputs(case('3x3-maps-M65'))
    qs = np.array([c['q'] for c in cells])
    bad = states.copy()
    for m, k, v in ((0, 4, qs[4]), (1, 0, -1), (2, 8, qs[8]), (3, 3, -1), (3, 4, qs[4]), (4, 5, 1), (5, 1, 32767), (6, 7, -32768)):
        bad[m, k] = v
    dc = DeviceCells(cells)
    for mode, sweeps, lines, u in ((0, lr.HEAT_SWEEPS, 'both', uniforms), (1, 1, 'both', None), (1, lr.QUENCH_SWEEPS, 'both', None),
                                   (1, 1, 'rows', None), (1, 1, 'columns', None), (0, 1, 'columns', uniforms[:1, :1])):
        got = line_device(dc, Nx, Ny, bad, mode, sweeps, lines, lr.BETA, u, pad=1)
        ref = lr.run(cells, Nx, Ny, bad, mode, sweeps, lines, lr.BETA, u)
        assert_same_run(got, ref)
        assert np.all(np.isfinite(got['energy'])) and np.all((got['states'] >= 0) & (got['states'] < qs[None, :]))
    none = line_device(dc, Nx, Ny, bad, 1, 0)
    assert np.array_equal(none['states'], bad) and same_bits(none['energy'], rr.total_energy(cells, Nx, Ny, bad))
    assert np.all(np.isfinite(none['energy']))


# ---------------------------------------------------------------------------------------------- 4. error contract
def test_error_contract():
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    Ny, Nx, cells, states, uniforms = lr.case_inputs(case('2x2-maps-M65'))
    dc = DeviceCells(cells)
    M, ncell = states.shape
    need = int(L.tn_line_sweep_ws_bytes(Nx, Ny, M))
    st = Guarded.of(torch.int16, (M, ncell), 0x11, seed=2)
    out = [Guarded.of(torch.float64, (M,), 0x22, seed=3), Guarded.of(torch.int32, (M,), 0x22, seed=4), Guarded.of(torch.int32, (M,), 0x22, seed=5)]
    u = dv(np.array(uniforms))

    def call(mode=0, lines=2, beta=lr.BETA, sweeps=2, uptr=u.data_ptr(), ldu=M, wsb=need, Mc=M, stp=st.ptr, Ep=out[0].ptr, ws_clean=True):
        ws = Guarded(max(wsb, 8), 0x33, seed=1)
        rc = L.tn_line_sweep(Nx, Ny, dc.ptr, Mc, stp, mode, lines, beta, sweeps, uptr, ldu, Ep, out[1].ptr, out[2].ptr, ws.ptr, wsb, ops._stream())
        torch.cuda.synchronize()
        assert ws.intact() and st.untouched(0x11) and st.intact() and all(o.untouched(0x22) and o.intact() for o in out)
        assert ws.untouched(0x33) == ws_clean
        return rc, _last_error()

    for kw, word in ((dict(mode=2), 'mode'), (dict(mode=-1), 'mode'), (dict(lines=3), 'lines'), (dict(lines=-1), 'lines'), (dict(beta=0.0), 'beta'),
                     (dict(beta=-1.0), 'beta'), (dict(beta=float('inf')), 'beta'), (dict(beta=float('nan')), 'beta'), (dict(uptr=None), 'uniforms'),
                     (dict(mode=1), 'uniforms'), (dict(ldu=M - 1), 'ldu'), (dict(sweeps=-1), 'sweeps'), (dict(Mc=0), 'M'), (dict(stp=None), 'states'),
                     (dict(Ep=None), 'energy_out')):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = call(wsb=need - 8)
    assert rc == -3 and 'workspace' in msg
    # the range guard: the one refusal that comes after a launch (the ranges are reduced on the device): only the head of ws is written
    r = lr.chain_ranges(cells, Nx, Ny, 'both')
    rc, msg = call(beta=301.0 / r, ws_clean=False)
    assert rc == -1 and 'range guard' in msg, (rc, msg)
    for lines in (0, 1):                                                           # each direction is held to its own tables
        rc, msg = call(beta=301.0 / lr.chain_ranges(cells, Nx, Ny, ('rows', 'columns')[lines]), lines=lines, ws_clean=False)
        assert rc == -1 and 'range guard' in msg and ('E1', 'E4')[lines] in msg, (rc, msg)
    assert L.tn_line_sweep_ws_bytes(0, 1, 5) == 0 and L.tn_line_sweep_ws_bytes(2, 2, 2 ** 31) == 0
    bad = DeviceCells(cells)
    bad.cells[1].q = 40000
    ws = Guarded(need, 0x33, seed=1)
    rc = L.tn_line_sweep(Nx, Ny, bad.ptr, M, st.ptr, 1, 2, 1.0, 1, None, 0, out[0].ptr, out[1].ptr, out[2].ptr, ws.ptr, need, ops._stream())
    torch.cuda.synchronize()
    assert rc == -1 and 'cells' in _last_error() and ws.untouched(0x33) and st.untouched(0x11) and out[0].untouched(0x22)


# ---------------------------------------------------------------------------------------------- 5. the public call
def device_cells(ins):
    """The reference lattice of a solver in its current rotation, from the tables relax.EnergyCells puts on the device, read back."""
    from tnac4o_amd.relax import EnergyCells
    t = EnergyCells(ins, torch.device('cuda', torch.cuda.current_device()))
    ising = ins.mode == 'Ising'
    cells = []
    for ny in range(ins.Ny):
        for nx in range(ins.Nx):
            tb = t.keep[(ny, nx)]
            q = int(tb.q)
            c = dict(q=q, Es=tb.Es.cpu().numpy().reshape(q), E1=None, E4=None, left_map=None, up_map=None)
            if nx > 0:
                c['E1'] = np.ascontiguousarray(tb.E1.cpu().numpy().reshape(q, -1))
                c['left_map'] = t.keep[(ny, nx - 1)].right.cpu().numpy().astype(np.int64) if ising else None
            if ny > 0:
                c['E4'] = np.ascontiguousarray(tb.E4.cpu().numpy().reshape(q, -1))
                c['up_map'] = t.keep[(ny - 1, nx)].down.cpu().numpy().astype(np.int64) if ising else None
            cells.append(c)
    return cells


SOLVERS = ['ising3x3', 'rmf3x3', 'chimera2x2', 'droplet0', 'droplet1']     # droplet1: a rotated lattice


@pytest.mark.parametrize('name', SOLVERS)
def test_public_call(name):
    from tnac4o_amd import rng as trng
    ins = make(name)                                                     # a fresh solver: no contraction has run
    qs = ins._cell_sizes()[ins.order]                                     # model order
    M, ncell = 64, qs.size
    rng = np.random.default_rng(78)
    start = rng.integers(0, qs[None, :], size=(M, ncell))
    u = rng.random((2, 2, ncell, M))
    ins.degeneracy = 5
    E = ins.relax_lines(sweeps=2, states=start, uniforms=u, chunk=24)
    assert not hasattr(ins, 'rhoT') and ins.degeneracy == 5
    cells = device_cells(ins)
    rot = np.empty_like(start)
    rot[:, ins.order] = start
    ref = lr.run(cells, ins.Nx, ins.Ny, rot, 0, 2, 'both', float(ins.beta), u)
    assert ref['margin'] >= lr.MARGIN_FLOOR
    assert E is ins.energy and np.array_equal(ins.states, ref['states'][:, ins.order])
    assert same_bits(ins.energy, ref['energy']) and same_bits(ins.relax_energy_before, rr.total_energy(cells, ins.Nx, ins.Ny, rot))
    assert np.array_equal(ins.relax_moves, ref['moves']) and ins.relax_sweeps == 2
    assert np.array_equal(ins.relax_converged, ref['last_moves'] == 0)
    assert float(np.max(np.abs(ins.energy - model_energy(name, ins)))) <= 1e-9
    assert ins.probability is None and ins.sample_log2Z is None and ins.log2Z_lower is None and ins.log2Z_estimate is None
    heat_states, heat_energy = np.copy(ins.states), np.copy(ins.energy)
    for chunk in (1, 7, M):                                               # chunk does not matter
        other = make(name)
        other.relax_lines(sweeps=2, states=start, uniforms=u, chunk=chunk)
        assert same_bits(other.states, heat_states) and same_bits(other.energy, heat_energy), chunk
    # one direction alone, numbers on the device
    for lines in ('rows', 'columns'):
        other = make(name)
        other.relax_lines(sweeps=1, lines=lines, states=start, uniforms=torch.as_tensor(u[:1, :1]).cuda(), chunk=17)
        ref1 = lr.run(cells, ins.Nx, ins.Ny, rot, 0, 1, lines, float(ins.beta), u[:1, :1])
        assert ref1['margin'] >= lr.MARGIN_FLOOR
        assert np.array_equal(other.states, ref1['states'][:, ins.order]) and same_bits(other.energy, ref1['energy']), lines
    # seed= equals uniforms= from the host generator, bit for bit, for every chunk
    us = trng.rows_host(4711, trng.RELAX_LINE, 0, 2 * 2 * ncell, 0, M).reshape(2, 2, ncell, M)
    byu = make(name)
    byu.relax_lines(sweeps=2, states=start, uniforms=us)
    for chunk in (None, 7):
        other = make(name)
        other.relax_lines(sweeps=2, states=start, seed=4711, chunk=chunk)
        assert same_bits(other.states, byu.states) and same_bits(other.energy, byu.energy) and same_bits(other.relax_moves, byu.relax_moves)
    # quench until nothing moves
    ins.relax_lines(mode='quench', sweeps=None)
    assert np.all(ins.relax_converged) and np.all(ins.energy <= ins.relax_energy_before) and same_bits(ins.relax_energy_before, heat_energy)
    hrot = np.empty_like(heat_states)
    hrot[:, ins.order] = heat_states
    refq = lr.run(cells, ins.Nx, ins.Ny, hrot, 1, ins.relax_sweeps)
    assert np.array_equal(ins.states, refq['states'][:, ins.order]) and same_bits(ins.energy, refq['energy'])
    assert np.array_equal(ins.relax_moves, refq['moves']) and np.all(refq['last_moves'] == 0)
    assert float(np.max(np.abs(ins.energy - model_energy(name, ins)))) <= 1e-9
    low = np.copy(ins.energy)
    ins.relax_lines(mode='quench', sweeps=1)
    assert np.all(ins.relax_moves == 0) and same_bits(ins.energy, low) and np.all(ins.relax_converged)


def test_public_range_guard_raises_before_device_work():
    from tnac4o_amd import lines
    ins = make('chimera2x2')
    r = lines.chain_range(ins, 'both')
    with pytest.raises(ValueError, match='range guard'):
        ins.relax_lines(states=np.zeros((3, 4), dtype=np.int64), beta=301.0 / r, seed=1)
    assert ins.states.shape[0] == 0


# ---------------------------------------------------------------------------------------------- 6. law of the chain
def test_law_of_the_chain():
    """2^14 chains from uniformly random states on 2 x 2 cells of q = 4 at beta = 0.7: after 1 sweep of rows and after 2 sweeps of rows
    and columns the empirical frequencies of the 256 configurations lie within 6 sigma of the exact mu0 P^k built from enumerated line
    conditionals (bins with M p < 20 pooled; the pooled bin holds less than 10 % of the mass)."""
    cells, beta, states, u, law_rows, law_both = lr.law_inputs()
    for lines, sweeps, law in (('rows', 1, law_rows), ('both', 2, law_both)):
        got = line_device(cells, 2, 2, states, 0, sweeps, lines, beta, u[:sweeps, :len(lr.PASSES[lines])])
        ok, z, bins = rr.law_statistic(rr.configuration_index(got['states']), law)
        pooled = float(law[lr.LAW_M * law < 20.0].sum())
        print('%s: largest deviation %.2f sigma over %d bins, pooled mass %.3f' % (lines, z, bins, pooled))
        assert ok and pooled < 0.1


# ---------------------------------------------------------------------------------------------- 7. fixed points of the line quench
@pytest.mark.parametrize('name', ['chimera2x2', 'droplet0'])
def test_line_minima_are_cell_minima(name):
    """After relax_lines(mode='quench', sweeps=None) reports convergence the cell quench of relax_samples moves nothing; the energies
    reached are reported next to those the cell quench reaches from the same starts."""
    ins = make(name)
    qs = ins._cell_sizes()[ins.order]
    start = np.random.default_rng(5).integers(0, qs[None, :], size=(128, qs.size))
    ins.relax_lines(mode='quench', sweeps=None, states=start)
    assert np.all(ins.relax_converged)
    E_line = np.copy(ins.energy)
    kept = np.copy(ins.states)
    ins.relax_samples(mode='quench', sweeps=1)
    assert np.all(ins.relax_moves == 0) and same_bits(ins.states, kept) and same_bits(ins.energy, E_line)
    other = make(name)
    other.relax_samples(mode='quench', sweeps=None, states=start)
    print('%s: mean energy after the line quench %.4f, after the cell quench %.4f (difference %.4f)'
          % (name, E_line.mean(), other.energy.mean(), E_line.mean() - other.energy.mean()))
