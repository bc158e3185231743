"""tn_cell_sweep and tnac4o.relax_samples on the GPU against the numpy reference of tests/relax_ref.py: the kernel on synthetic tables
(every lattice edge, mixed q, with and without the Ising maps, tables in LDS and in global memory), slicing, states outside their cell,
the error contract, the public call on the solvers of the sampling tests, and the law of the chain against the exact mu0 P^5."""
import ctypes as ct

import numpy as np
import pytest

import relax_ref as rr
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_sampling import droplet, dv, small      # noqa: E402  (helpers only, no test is imported)

CASE_IDS = ['%s-%s-M%d%s' % (c[0], 'maps' if c[1] else 'nomaps', c[2], '-int' if c[4] else '') for c in rr.CASES]


# ---------------------------------------------------------------------------------------------- helpers
class DeviceCells:
    """The tn_beam_cell array of a reference lattice: the energy part on the device, everything else NULL / 0."""

    def __init__(self, cells):
        from tnac4o_amd.beam import _Cell
        self.keep = []
        self.cells = (_Cell * len(cells))()
        for k, c in enumerate(cells):
            d = self.cells[k]
            d.q = c['q']
            d.Es = self._put(c['Es'])
            d.E1, d.E4 = self._put(c['E1']), self._put(c['E4'])
            d.left_map, d.up_map = self._put(c['left_map']), self._put(c['up_map'])
            d.e1cols = c['E1'].shape[1] if c['E1'] is not None else 0
            d.e4cols = c['E4'].shape[1] if c['E4'] is not None else 0
        self.ptr = ct.cast(self.cells, ct.c_void_p)

    def _put(self, a):
        if a is None:
            return None
        self.keep.append(dv(a))
        return self.keep[-1].data_ptr()


def sweep_device(cells, Nx, Ny, states, mode, sweeps, beta=1.0, uniforms=None, pad=0, want_rc=0, lds=None, monkeypatch=None):
    """One call of tn_cell_sweep with every buffer between guards: dict(rc, states, energy, moves, last_moves).  uniforms
    (sweeps, ncell, M) travel with ldu = M + pad, the columns beyond M poisoned with NaN."""
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    M, ncell = states.shape
    dc = cells if isinstance(cells, DeviceCells) else DeviceCells(cells)
    need = int(L.tn_cell_sweep_ws_bytes(Nx, Ny, M))
    assert need > 0
    ws = Guarded(need, 'random', seed=1)
    st = Guarded.of(torch.int16, (M, ncell), 0xFF, seed=2)
    st.tensor().copy_(dv(np.asarray(states).astype(np.int16)))
    E = Guarded.of(torch.float64, (M,), 0xFF, seed=3)
    mv = Guarded.of(torch.int32, (M,), 0xFF, seed=4)
    lm = Guarded.of(torch.int32, (M,), 0xFF, seed=5)
    u, ldu = None, 0
    if uniforms is not None:
        ldu = M + pad
        u = Guarded.of(torch.float64, (uniforms.shape[0] * ncell, ldu), 0xFF, seed=6)      # 0xFF bytes: NaN beyond column M
        u.tensor()[:, :M].copy_(dv(np.array(uniforms).reshape(-1, M)))
    if lds is not None:
        monkeypatch.setenv('TN_CELL_SWEEP_LDS', str(lds))
    rc = L.tn_cell_sweep(Nx, Ny, dc.ptr, M, st.ptr, mode, beta, sweeps, u.ptr if u is not None else None, ldu, E.ptr, mv.ptr, lm.ptr,
                         ws.ptr, need, ops._stream())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _last_error())
    for g in (ws, st, E, mv, lm) + ((u,) if u is not None else ()):
        assert g.intact()
    return dict(rc=rc, states=st.host().astype(np.int64), energy=E.host(), moves=mv.host().astype(np.int64),
                last_moves=lm.host().astype(np.int64))


def _last_error():
    from tnac4o_amd import _lib
    buf = ct.create_string_buffer(512)
    _lib.lib().tn_last_error(buf, 512)
    return buf.value.decode()


def assert_same_run(got, ref):
    assert np.array_equal(got['states'], ref['states'])
    assert same_bits(got['energy'], ref['energy'])
    assert np.array_equal(got['moves'], ref['moves']) and np.array_equal(got['last_moves'], ref['last_moves'])


# ---------------------------------------------------------------------------------------------- 1. kernel on synthetic tables
@pytest.mark.parametrize('case', rr.CASES, ids=CASE_IDS)
def test_kernel_against_the_reference(case, monkeypatch):
    """2 heat-bath sweeps and 3 quench sweeps of every shared case: the reference's states, the bits of its energies, its move counts;
    sweeps = 0 returns the states untouched and their energies; ldu > M with NaN beyond column M; guards intact.  With no table
    staged in LDS (TN_CELL_SWEEP_LDS=0) and with every table that fits 150 KiB staged, the same bits as with the default."""
    Ny, Nx, cells, states, uniforms = rr.case_inputs(case)
    dc = DeviceCells(cells)
    heat = sweep_device(dc, Nx, Ny, states, 0, rr.HEAT_SWEEPS, rr.BETA, uniforms, pad=3)
    assert_same_run(heat, rr.case_reference(case, 0))
    quench = sweep_device(dc, Nx, Ny, states, 1, rr.QUENCH_SWEEPS)
    assert_same_run(quench, rr.case_reference(case, 1))
    none = sweep_device(dc, Nx, Ny, states, 1, 0)
    assert np.array_equal(none['states'], states) and same_bits(none['energy'], rr.total_energy(cells, Nx, Ny, states))
    assert np.all(none['moves'] == 0) and np.all(none['last_moves'] == 0)
    none = sweep_device(dc, Nx, Ny, states, 0, 0, rr.BETA, uniforms, pad=1)
    assert np.array_equal(none['states'], states) and same_bits(none['energy'], rr.total_energy(cells, Nx, Ny, states))
    for lds in (0, 150 * 1024):                                          # no table staged / every table that fits 150 KiB
        assert_same_run(sweep_device(dc, Nx, Ny, states, 0, rr.HEAT_SWEEPS, rr.BETA, uniforms, pad=3, lds=lds, monkeypatch=monkeypatch), heat)
        assert_same_run(sweep_device(dc, Nx, Ny, states, 1, rr.QUENCH_SWEEPS, lds=lds, monkeypatch=monkeypatch), quench)


def test_move_outputs_may_be_null():
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    case = rr.CASES[CASE_IDS.index('3x3-maps-M65')]
    Ny, Nx, cells, states, uniforms = rr.case_inputs(case)
    dc = DeviceCells(cells)
    M = states.shape[0]
    need = int(L.tn_cell_sweep_ws_bytes(Nx, Ny, M))
    ws = Guarded(need, 0xFF, seed=1)
    st, u = dv(states.astype(np.int16)), dv(np.array(uniforms))
    E = Guarded.of(torch.float64, (M,), 0xFF, seed=3)
    rc = L.tn_cell_sweep(Nx, Ny, dc.ptr, M, st.data_ptr(), 0, rr.BETA, rr.HEAT_SWEEPS, u.data_ptr(), M, E.ptr, None, None, ws.ptr, need, ops._stream())
    torch.cuda.synchronize()
    ref = rr.case_reference(case, 0)
    assert rc == 0 and ws.intact() and E.intact()
    assert np.array_equal(st.cpu().numpy(), ref['states']) and same_bits(E.host(), ref['energy'])


# ---------------------------------------------------------------------------------------------- 2. slicing
@pytest.mark.parametrize('mode', [0, 1])
def test_slicing(mode):
    """The 300 samples of a case as one call, as chunks of 7, and embedded at offset 123 among other samples: identical bits per sample."""
    case = rr.CASES[CASE_IDS.index('3x3-maps-M300')]
    Ny, Nx, cells, states, uniforms = rr.case_inputs(case)
    dc = DeviceCells(cells)
    sweeps = rr.HEAT_SWEEPS if mode == 0 else rr.QUENCH_SWEEPS
    u = uniforms if mode == 0 else None
    whole = sweep_device(dc, Nx, Ny, states, mode, sweeps, rr.BETA, u, pad=2)
    assert_same_run(whole, rr.case_reference(case, mode))
    for lo in range(0, 300, 7):
        part = sweep_device(dc, Nx, Ny, states[lo:lo + 7], mode, sweeps, rr.BETA, None if u is None else u[:, :, lo:lo + 7])
        for key in ('states', 'energy', 'moves', 'last_moves'):
            assert same_bits(part[key], whole[key][lo:lo + 7]), (lo, key)
    rng = np.random.default_rng(8)
    qs = np.array([c['q'] for c in cells])
    big = rng.integers(0, qs[None, :], size=(700, qs.size))
    big[123:423] = states
    ub = None
    if mode == 0:
        ub = rng.random((sweeps, qs.size, 700))
        ub[:, :, 123:423] = uniforms
    emb = sweep_device(dc, Nx, Ny, big, mode, sweeps, rr.BETA, ub, pad=5)
    for key in ('states', 'energy', 'moves', 'last_moves'):
        assert same_bits(emb[key][123:423], whole[key]), key


# ---------------------------------------------------------------------------------------------- 3. states outside their cell
def test_states_outside_their_cell():
    """States q and -1 in a few samples of the 3 x 3 lattice: never an index (guards intact, finite energies); as neighbours they are
    read as 0, in a quench their own energy counts as +inf -- the reference's rules -- and a heat-bath sweep leaves every state inside."""
    case = rr.CASES[CASE_IDS.index('3x3-maps-M65')]
    Ny, Nx, cells, states, uniforms = rr.case_inputs(case)
    qs = np.array([c['q'] for c in cells])
    bad = states.copy()
    for m, k, v in ((0, 4, qs[4]), (1, 0, -1), (2, 8, qs[8]), (3, 3, -1), (3, 4, qs[4]), (4, 5, 1), (5, 1, 32767), (6, 7, -32768)):
        bad[m, k] = v
    dc = DeviceCells(cells)
    for mode, sweeps, u in ((0, rr.HEAT_SWEEPS, uniforms), (1, 1, None), (1, rr.QUENCH_SWEEPS, None)):
        got = sweep_device(dc, Nx, Ny, bad, mode, sweeps, rr.BETA, u, pad=1)
        ref = rr.run(cells, Nx, Ny, bad, mode, sweeps, rr.BETA, u)
        assert_same_run(got, ref)
        assert np.all(np.isfinite(got['energy'])) and np.all((got['states'] >= 0) & (got['states'] < qs[None, :]))
    none = sweep_device(dc, Nx, Ny, bad, 1, 0)
    assert np.array_equal(none['states'], bad) and same_bits(none['energy'], rr.total_energy(cells, Nx, Ny, bad))
    assert np.all(np.isfinite(none['energy']))


# ---------------------------------------------------------------------------------------------- 4. error contract
def test_error_contract():
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    case = rr.CASES[CASE_IDS.index('2x2-maps-M65')]
    Ny, Nx, cells, states, uniforms = rr.case_inputs(case)
    dc = DeviceCells(cells)
    M, ncell = states.shape
    need = int(L.tn_cell_sweep_ws_bytes(Nx, Ny, M))
    st = Guarded.of(torch.int16, (M, ncell), 0x11, seed=2)
    out = [Guarded.of(torch.float64, (M,), 0x22, seed=3), Guarded.of(torch.int32, (M,), 0x22, seed=4), Guarded.of(torch.int32, (M,), 0x22, seed=5)]
    u = dv(np.array(uniforms))

    def call(mode=0, beta=rr.BETA, sweeps=2, uptr=u.data_ptr(), ldu=M, wsb=need, Mc=M):
        ws = Guarded(max(wsb, 8), 0x33, seed=1)
        rc = L.tn_cell_sweep(Nx, Ny, dc.ptr, Mc, st.ptr, mode, beta, sweeps, uptr, ldu, out[0].ptr, out[1].ptr, out[2].ptr, ws.ptr, wsb, ops._stream())
        torch.cuda.synchronize()
        assert ws.untouched(0x33) and ws.intact() and st.untouched(0x11) and all(o.untouched(0x22) and o.intact() for o in out)
        return rc, _last_error()

    for kw, word in ((dict(mode=2), 'mode'), (dict(mode=-1), 'mode'), (dict(beta=0.0), 'beta'), (dict(beta=-1.0), 'beta'),
                     (dict(beta=float('inf')), 'beta'), (dict(beta=float('nan')), 'beta'), (dict(uptr=None), 'uniforms'),
                     (dict(mode=1), 'uniforms'), (dict(ldu=M - 1), 'ldu'), (dict(sweeps=-1), 'sweeps'), (dict(Mc=0), 'M')):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    rc, msg = call(wsb=need - 8)
    assert rc == -3 and 'workspace' in msg
    assert L.tn_cell_sweep_ws_bytes(0, 1, 5) == 0 and L.tn_cell_sweep_ws_bytes(2, 2, 2 ** 31) == 0


# ---------------------------------------------------------------------------------------------- 5. the public call
def solver_cells(ins):
    """The reference lattice of a solver in its current rotation, from the solver's own host tables."""
    ising = ins.mode == 'Ising'
    cells = []
    for ny in range(ins.Ny):
        for nx in range(ins.Nx):
            Es, E1, E4 = ins._cell_energies(ny, nx)
            c = dict(q=int(ins._cell_sizes()[ny * ins.Nx + nx]), Es=np.asarray(Es, dtype=np.float64), E1=None, E4=None, left_map=None, up_map=None)
            if nx > 0:
                c['E1'] = np.ascontiguousarray(E1, dtype=np.float64)
                c['left_map'] = np.asarray(ins._cell_maps(ny, nx - 1)[1], dtype=np.int64) if ising else None
            if ny > 0:
                c['E4'] = np.ascontiguousarray(E4, dtype=np.float64)
                c['up_map'] = np.asarray(ins._cell_maps(ny - 1, nx)[0], dtype=np.int64) if ising else None
            cells.append(c)
    return cells


def model_energy(name, ins):
    from tnac4o_amd import auxx
    import golden_inputs as gi
    import marginals_ref as mr
    if name == 'rmf3x3':
        return auxx.energy_RMF(auxx.synthetic_rmf(3, 3, 3, 17), np.asarray(ins.states))
    J = {'ising3x3': mr.ising_3x3_nc2(), 'chimera2x2': auxx.synthetic_chimera(2, 2, 29)}.get(name)
    return auxx.energy_Jij(gi.droplet_J(128, 1) if J is None else J, ins.binary_states())


def make(name):
    if name.startswith('droplet'):
        return droplet(int(name[-1]), beta=1.0)
    return small(name, 1.0)


SOLVERS = ['ising3x3', 'rmf3x3', 'chimera2x2', 'droplet0', 'droplet1']


@pytest.mark.parametrize('name', SOLVERS)
def test_public_call(name):
    ins = make(name)                                                     # a fresh solver: no contraction has run
    qs = ins._cell_sizes()[ins.order]                                     # model order
    M, ncell = 64, qs.size
    rng = np.random.default_rng(77)
    start = rng.integers(0, qs[None, :], size=(M, ncell))
    u = rng.random((2, ncell, M))
    ins.degeneracy = 5
    E = ins.relax_samples(sweeps=2, states=start, uniforms=u, chunk=24)
    assert not hasattr(ins, 'rhoT') and ins.degeneracy == 5
    cells = solver_cells(ins)
    rot = np.empty_like(start)
    rot[:, ins.order] = start
    ref = rr.run(cells, ins.Nx, ins.Ny, rot, 0, 2, float(ins.beta), u)
    assert ref['margin'] >= 1e-9
    assert E is ins.energy and np.array_equal(ins.states, ref['states'][:, ins.order])
    assert same_bits(ins.energy, ref['energy']) and same_bits(ins.relax_energy_before, rr.total_energy(cells, ins.Nx, ins.Ny, rot))
    assert np.array_equal(ins.relax_moves, ref['moves']) and ins.relax_sweeps == 2
    assert np.array_equal(ins.relax_converged, ref['last_moves'] == 0)
    assert float(np.max(np.abs(ins.energy - model_energy(name, ins)))) <= 1e-9
    assert ins.probability is None and ins.sample_log2Z is None and ins.log2Z_lower is None and ins.log2Z_estimate is None
    kept = np.copy(ins.states)
    ins.calculate_log_probability(boundary='build', Dmax=4)             # states = None: the relaxed ones
    assert same_bits(ins.scored_energy, ins.energy) and same_bits(ins.states, kept)
    # quench until nothing moves
    before = np.copy(ins.energy)
    ins.relax_samples(mode='quench', sweeps=None)
    assert np.all(ins.relax_converged) and np.all(ins.energy <= ins.relax_energy_before) and same_bits(ins.relax_energy_before, before)
    rot = np.empty_like(kept)
    rot[:, ins.order] = kept
    refq = rr.run(cells, ins.Nx, ins.Ny, rot, 1, ins.relax_sweeps)
    assert np.array_equal(ins.states, refq['states'][:, ins.order]) and same_bits(ins.energy, refq['energy'])
    assert np.array_equal(ins.relax_moves, refq['moves']) and np.all(refq['last_moves'] == 0)
    assert float(np.max(np.abs(ins.energy - model_energy(name, ins)))) <= 1e-9
    low = np.copy(ins.energy)
    ins.relax_samples(mode='quench', sweeps=1)
    assert np.all(ins.relax_moves == 0) and same_bits(ins.energy, low) and np.all(ins.relax_converged)
    assert hasattr(ins, 'rhoT') and ins.degeneracy == 5                  # (the boundaries of the scoring call are still there)


@pytest.mark.parametrize('rot', [0, 1])
def test_public_call_on_samples(rot):
    """The droplet: states from sample_boltzmann(M=64, Dmax=4), one heat-bath sweep with numbers from numpy's global generator, then a
    quench; uniforms on the device give the same result."""
    ins = droplet(rot)
    ins.sample_boltzmann(M=64, Dmax=4, uniforms=np.random.default_rng(3).random((16, 64)))
    start, E0 = np.copy(ins.states), np.copy(ins.energy)
    np.random.seed(11)
    ins.relax_samples()
    np.random.seed(11)
    u = np.random.rand(1, 16, 64)
    cells = solver_cells(ins)
    srot = np.empty_like(start)
    srot[:, ins.order] = start
    ref = rr.run(cells, ins.Nx, ins.Ny, srot, 0, 1, float(ins.beta), u)
    assert ref['margin'] >= 1e-9
    assert np.array_equal(ins.states, ref['states'][:, ins.order]) and same_bits(ins.energy, ref['energy'])
    assert same_bits(ins.relax_energy_before, E0)                        # the bits of the sampling walk's energy
    assert ins.probability is None and ins.sample_log2Z is None and ins.log2Z_lower is None and ins.log2Z_estimate is None
    relaxed = np.copy(ins.states)
    ins.calculate_log_probability(boundary='keep')
    assert same_bits(ins.scored_energy, ins.energy)
    other = droplet(rot)
    other.relax_samples(states=start, uniforms=torch.as_tensor(u).cuda(), chunk=17)
    assert same_bits(other.states, relaxed) and same_bits(other.energy, ins.energy)
    ins.relax_samples(mode='quench', sweeps=None)
    assert np.all(ins.relax_converged) and np.all(ins.energy <= ins.relax_energy_before)


# ---------------------------------------------------------------------------------------------- 6. law of the chain
def test_law_of_the_chain():
    """2^14 chains from uniformly random states, 5 sweeps with seeded uniforms, on 2 x 2 cells of q = 4 at beta = 0.7: the empirical
    frequencies of the 256 configurations against the exact law mu0 P^5 of the reference matrix (no mixing assumption); bins with
    M p < 20 pooled, every bin within 6 sqrt(p (1 - p) / M).  tests/test_relax_host.py shows that the reference chain passes on this
    seed."""
    cells, beta, states, uniforms, law = rr.law_inputs()
    got = sweep_device(cells, 2, 2, states, 0, rr.LAW_SWEEPS, beta, uniforms)
    ok, z, bins = rr.law_statistic(rr.configuration_index(got['states']), law)
    print('largest deviation %.2f sigma over %d bins' % (z, bins))
    assert ok
    assert np.array_equal(got['states'], rr.run(cells, 2, 2, states, 0, rr.LAW_SWEEPS, beta, uniforms)['states'])
