"""tn_anneal and tnac4o.anneal_population on the GPU against the numpy reference of tests/anneal_ref.py: whole calls on the shared inputs
(mixed q with and without maps across the 256-row tile of the running sums), the tiling of the sums, every width of the row copy, the
degenerate forms, cutting the schedule into calls, independence of the LDS staging, the errors, and the public call.  Every buffer of a
library call lies between guards."""
import ctypes as ct

import numpy as np
import pytest

import anneal_ref as ar
import relax_ref as rr
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_relax import DeviceCells, solver_cells                    # noqa: E402  (helpers only, no test is imported)
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


def anneal_device(cells, Nx, Ny, states, family, betas, sweeps, usweep=None, ures=None, pad=0, optional=True, lds=None, monkeypatch=None, want_rc=0,
                  short_ws=0, override=None):
    """One call of tn_anneal with every buffer between guards; the arguments and the result are those of anneal_ref.run.  usweep travels
    with ldu = M + pad, the columns beyond M poisoned with NaN; optional=False passes NULL for the two traces.  want_rc != 0: the call
    must fail with that code and write nothing; override: arguments replaced by hand (None = a null pointer)."""
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    betas = np.asarray(betas, dtype=np.float64)
    M, ncell = states.shape
    K = betas.size
    dc = cells if isinstance(cells, DeviceCells) else DeviceCells(cells)
    need = int(L.tn_anneal_ws_bytes(Nx, Ny, M))
    assert need > 0
    ws = Guarded(need - short_ws, 'random', seed=1)
    st = _framed(torch.int16, np.asarray(states).astype(np.int16), 2)
    fam = _framed(torch.int32, np.asarray(family, dtype=np.int32), 3)
    E = Guarded.of(torch.float64, (M,), 0xFF, seed=4)
    u, ldu = None, 0
    if usweep is not None and (K - 1) * sweeps > 0:
        ldu = M + pad
        u = Guarded.of(torch.float64, ((K - 1) * sweeps * ncell, ldu), 0xFF, seed=5)         # 0xFF bytes: NaN beyond column M
        u.tensor()[:, :M].copy_(dv(np.array(usweep).reshape(-1, M)))
    g_r = _framed(torch.float64, np.asarray(ures, dtype=np.float64), 6) if K > 1 else None
    emin, wsum, w2sum = (Guarded.of(torch.float64, (K - 1,), 0xFF, seed=7 + i) for i in range(3))
    surv = Guarded.of(torch.int32, (K - 1,), 0x55, seed=10)
    et = Guarded.of(torch.float64, (K - 1, M), 0xFF, seed=11)
    pt = Guarded.of(torch.int32, (K - 1, M), 0x55, seed=12)
    if lds is not None:
        monkeypatch.setenv('TN_CELL_SWEEP_LDS', str(lds))
    c_betas = (ct.c_double * K)(*betas.tolist())

    def ptr(g):
        return None if g is None else g.ptr

    per_step = [ptr(g) if K > 1 else None for g in (emin, wsum, w2sum, surv)]
    a = dict(Nx=Nx, Ny=Ny, cells=dc.ptr, M=M, K=K, betas=ct.cast(c_betas, ct.c_void_p), states=st.ptr, family=fam.ptr, sweeps=sweeps, usweep=ptr(u), ldu=ldu,
             ures=ptr(g_r), E=E.ptr, emin=per_step[0], wsum=per_step[1], w2sum=per_step[2], surv=per_step[3], et=et.ptr if optional else None,
             pt=pt.ptr if optional else None, ws=ws.ptr, wsb=need - short_ws)
    a.update(override or {})
    if 'schedule' in a:                                                  # (another HOST array of betas)
        c_bad = (ct.c_double * len(a['schedule']))(*a['schedule'])
        a['betas'] = ct.cast(c_bad, ct.c_void_p)
    rc = L.tn_anneal(a['Nx'], a['Ny'], a['cells'], a['M'], a['K'], a['betas'], a['states'], a['family'], a['sweeps'], a['usweep'], a['ldu'], a['ures'], a['E'],
                     a['emin'], a['wsum'], a['w2sum'], a['surv'], a['et'], a['pt'], a['ws'], a['wsb'], ops._stream())
    torch.cuda.synchronize()
    assert rc == want_rc, (rc, _last_error())
    every = [ws, st, fam, E, emin, wsum, w2sum, surv, et, pt] + [x for x in (u, g_r) if x is not None]
    for g in every:
        assert g.intact()
    if want_rc:
        assert np.array_equal(st.host(), np.asarray(states).astype(np.int16)) and np.array_equal(fam.host(), np.asarray(family, dtype=np.int32))
        assert all(g.untouched(0xFF) for g in (E, emin, wsum, w2sum, et)) and surv.untouched(0x55) and pt.untouched(0x55)
        return _last_error()
    if not optional:
        assert et.untouched(0xFF) and pt.untouched(0x55)
    return dict(states=st.host().astype(np.int64), family=fam.host().astype(np.int64), energy=E.host(), emin=emin.host(), wsum=wsum.host(),
                w2sum=w2sum.host(), survivors=surv.host().astype(np.int64), energy_trace=et.host(), parent_trace=pt.host().astype(np.int64))


def device_case(c, lo=0, hi=None, state=None, dc=None, sweeps=ar.SWEEPS, **kw):
    """anneal_device on the steps lo .. hi - 1 of a case's inputs, from `state` = a previous result (None: the case's start)."""
    hi = c['betas'].size - 1 if hi is None else hi
    s = state or c
    return anneal_device(dc or c['cells'], c['Nx'], c['Ny'], s['states'], s['family'], c['betas'][lo:hi + 1], sweeps,
                         c['usweep'][lo:hi] if sweeps else None, c['ures'][lo:hi], **kw)


def assert_same_call(got, ref, M, traces=True):
    """Equal: states, family, parents, survivors; energy_out, the energy trace and emin_out in the reference's bits; wsum_out and w2sum_out
    within (M + 8) 2^-52 (relative) of the exactly summed reference."""
    for k in ('states', 'family', 'survivors') + (('parent_trace',) if traces else ()):
        assert np.array_equal(got[k], ref[k]), k
    assert same_bits(got['energy'], ref['energy']) and same_bits(got['emin'], ref['emin'])
    if traces:
        assert same_bits(got['energy_trace'], ref['energy_trace'])
    tol = (M + 8) * 2.0 ** -52
    for k in ('wsum', 'w2sum'):
        err = np.abs(got[k] - ref[k]) / ref[k] if ref[k].size else np.zeros(0)
        print('%s: largest relative error %.2e (bound %.2e)' % (k, err.max() if err.size else 0.0, tol))
        assert np.all(err <= tol), k


# ---------------------------------------------------------------------------------------------- 1. whole calls against the reference
@pytest.mark.parametrize('case', ar.CASES, ids=ar.CASE_IDS)
def test_call_against_the_reference(case):
    """3 steps of 2 sweeps on every shared input (the integer tables with tied energies among them): ldu > M with NaN beyond column M;
    guards intact; then the traces NULL."""
    c, ref = ar.case_inputs(case), ar.case_reference(case)
    dc = DeviceCells(c['cells'])
    M = case[2]
    assert_same_call(device_case(c, dc=dc, pad=3), ref, M)
    assert_same_call(device_case(c, dc=dc, optional=False), ref, M, traces=False)


# ---------------------------------------------------------------------------------------------- 2. the tiling of the running sums
@pytest.mark.parametrize('M,seed', ar.TILE_CASES, ids=['M%d' % c[0] for c in ar.TILE_CASES])
def test_scan_tiling(M, seed):
    """Resampling alone (sweeps = 0, usweep NULL) on the one-cell lattice, M = tile - 1, tile, tile + 1 and above tile^2: parents, states,
    families and survivors equal the reference, the sums within their bound."""
    c, ref = ar.tile_inputs(M, seed), ar.tile_reference(M, seed)
    got = anneal_device(c['cells'], c['Nx'], c['Ny'], c['states'], c['family'], c['betas'], 0, None, c['ures'])
    assert_same_call(got, ref, M)
    assert np.all(np.diff(got['parent_trace'], axis=1) >= 0) and np.all(ref['survivors'] < M)


@pytest.mark.parametrize('case', ar.WIDTH_CASES, ids=['%dx%d' % c[:2] for c in ar.WIDTH_CASES])
def test_row_widths(case):
    """Rows of 4, 16 and 32 bytes: the pieces of 4 and 16 bytes of the row copy (the other inputs take those of 2 and 8)."""
    c, ref = ar.width_inputs(case), ar.width_reference(case)
    assert_same_call(device_case(c, sweeps=1, pad=1), ref, case[3])


# ---------------------------------------------------------------------------------------------- 3. degenerate forms
def test_degenerate_forms():
    """K = 1 writes energy_out only (every other pointer NULL); M = 1 keeps its row through every step; sweeps = 0 carries the energies."""
    case = ar.CASES[[c[:3] for c in ar.CASES].index(('2x2', True, 65))]
    c = ar.case_inputs(case)
    dc = DeviceCells(c['cells'])
    E0 = rr.total_energy(c['cells'], c['Nx'], c['Ny'], c['states'])
    one = anneal_device(dc, c['Nx'], c['Ny'], c['states'], c['family'], c['betas'][:1], 2, None, None, optional=False)
    assert np.array_equal(one['states'], c['states']) and np.array_equal(one['family'], c['family']) and same_bits(one['energy'], E0)
    got = device_case(c, dc=dc, sweeps=0)
    ref = ar.run(c['cells'], c['Nx'], c['Ny'], c['states'], c['family'], c['betas'], 0, None, c['ures'])
    assert ref['resample_margin'] >= ar.delta(65)
    assert_same_call(got, ref, 65)
    assert same_bits(got['energy_trace'][0], E0[got['parent_trace'][0]])
    single = ar.CASES[[c[:3] for c in ar.CASES].index(('2x2', True, 1))]
    got = device_case(ar.case_inputs(single))
    assert np.all(got['parent_trace'] == 0) and np.all(got['survivors'] == 1) and np.all(got['wsum'] == 1.0) and np.all(got['w2sum'] == 1.0)


def test_a_dominating_row():
    """db so large that every weight but one underflows to 0: M copies of that row, whatever u; one family is left."""
    Ny, Nx, qs = rr.LATTICES['1x1']
    cells = rr.make_cells(Ny, Nx, qs, False, 31)
    low = int(np.argmin(cells[0]['Es']))
    M = 300
    states = np.random.default_rng(32).integers(0, qs[0], size=(M, 1))
    states[states[:, 0] == low, 0] = (low + 1) % qs[0]
    states[211, 0] = low
    for u in (0.0, 0.43, np.nextafter(1.0, 0.0)):
        got = anneal_device(cells, Nx, Ny, states, np.arange(M), [0.0, 1e6], 0, None, [u])
        assert np.all(got['parent_trace'] == 211) and np.all(got['family'] == 211) and np.all(got['states'] == low)
        assert got['survivors'][0] == 1 and got['wsum'][0] == 1.0 and got['w2sum'][0] == 1.0 and got['emin'][0] == cells[0]['Es'][low]


def test_nan_energies_leave_the_rows_where_they_are():
    """A NaN in Es of the one-cell lattice.  Every row holds that state: Emin and every weight are NaN, W = 0 and the step is the identity.
    Some rows hold it: they get no copy, the others are resampled as the reference does.  Nothing out of range is accessed."""
    Ny, Nx, qs = rr.LATTICES['1x1']
    cells = [dict(c) for c in rr.make_cells(Ny, Nx, qs, False, 33)]
    cells[0]['Es'] = cells[0]['Es'].copy()
    cells[0]['Es'][7] = np.nan
    M = 300
    states = np.full((M, 1), 7)
    fam = np.arange(M)[::-1].copy()
    got = anneal_device(cells, Nx, Ny, states, fam, [0.2, 0.9, 1.1], 0, None, [0.3, 0.8])
    assert np.array_equal(got['parent_trace'], np.tile(np.arange(M), (2, 1))) and np.array_equal(got['family'], fam) and np.array_equal(got['states'], states)
    assert np.isnan(got['emin']).all() and np.all(got['wsum'] == 0.0) and np.all(got['w2sum'] == 0.0) and np.all(got['survivors'] == M)
    assert np.isnan(got['energy']).all()
    states = np.random.default_rng(34).integers(0, qs[0], size=(M, 1))
    states[::17, 0] = 7
    ref = ar.run(cells, Nx, Ny, states, fam, [0.2, 0.9], 0, None, [0.3])
    assert ref['resample_margin'] >= ar.delta(M)
    got = anneal_device(cells, Nx, Ny, states, fam, [0.2, 0.9], 0, None, [0.3])
    assert np.array_equal(got['parent_trace'], ref['parent_trace']) and np.array_equal(got['states'], ref['states']) and not np.any(got['states'] == 7)
    assert same_bits(got['emin'], ref['emin']) and np.isfinite(got['energy']).all() and got['survivors'][0] == ref['survivors'][0]


# ---------------------------------------------------------------------------------------------- 4. cutting, independence
def test_cutting_the_schedule():
    """5 steps as one call and as calls of 1 + 2 + 2 steps with states and family carried over: everything identical, traces included
    (an odd and an even number of steps: the result comes home from either copy of the rows)."""
    case = ar.CASES[[c[:3] for c in ar.CASES].index(('3x3', True, 300))]
    c = ar.case_inputs(case, 6)
    dc = DeviceCells(c['cells'])
    whole = device_case(c, dc=dc)
    ref = ar.run_case(c)
    assert ref['margin'] >= 1e-9 and ref['resample_margin'] >= ar.delta(300)
    assert_same_call(whole, ref, 300)
    parts, state = [], None
    for lo, hi in ((0, 1), (1, 3), (3, 5)):
        state = device_case(c, lo=lo, hi=hi, state=state, dc=dc)
        parts.append(state)
    for k in ('states', 'family', 'energy'):
        assert same_bits(state[k], whole[k]), k
    for k in ('emin', 'wsum', 'w2sum', 'survivors', 'energy_trace', 'parent_trace'):
        assert same_bits(np.concatenate([p[k] for p in parts]), whole[k]), k


def test_independent_of_the_lds_staging(monkeypatch):
    """TN_CELL_SWEEP_LDS=0 (no table staged) against the default: the same bits of everything."""
    case = ar.CASES[[c[:3] for c in ar.CASES].index(('3x3', False, 65))]
    c = ar.case_inputs(case)
    dc = DeviceCells(c['cells'])
    a = device_case(c, dc=dc)
    b = device_case(c, dc=dc, lds=0, monkeypatch=monkeypatch)
    for k in a:
        assert same_bits(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- 5. errors
def test_errors_write_nothing():
    """A short workspace gives -3; bad betas, ldu < M and null pointers give -1; states, family and every output keep their bytes."""
    case = ar.CASES[[c[:3] for c in ar.CASES].index(('2x2', False, 65))]
    c = ar.case_inputs(case)
    dc = DeviceCells(c['cells'])
    assert 'workspace' in device_case(c, dc=dc, want_rc=-3, short_ws=1)
    for override, word in ((dict(schedule=[0.5, 0.4, 0.9, 1.0]), 'increasing'), (dict(schedule=[-0.1, 0.4, 0.9, 1.0]), 'negative'),
                           (dict(schedule=[0.1, 0.4, 0.9, float('inf')]), 'finite'), (dict(ldu=64), 'ldu'), (dict(states=None), 'states'),
                           (dict(family=None), 'family'), (dict(E=None), 'energy_out'), (dict(ures=None), 'ures'), (dict(usweep=None), 'usweep'),
                           (dict(surv=None), 'survivors_out'), (dict(ws=None), 'ws'), (dict(cells=None), 'cells')):
        msg = device_case(c, dc=dc, want_rc=-1, override=override)
        assert msg.startswith('tn_anneal') and word in msg, (override, msg)


# ---------------------------------------------------------------------------------------------- 6. the law on the device
def test_law_of_the_final_population():
    """The run of tests/test_anneal_host.py at M = 2^14 on the device: the reference's states, and the exact law at 0.7 within 6 sigma."""
    from tnac4o_amd import anneal as an
    c, ref = ar.law_inputs(ar.LAW_M, ar.LAW_SEED), ar.law_reference(ar.LAW_M, ar.LAW_SEED)
    got = device_case(c, sweeps=ar.LAW_SWEEPS, optional=False)
    assert_same_call(got, ref, ar.LAW_M, traces=False)
    _, pi = rr.boltzmann(c['cells'], 2, 2, ar.LAW_BETAS[-1])
    ok, z, bins = rr.law_statistic(rr.configuration_index(got['states']), pi)
    lz = an.log2Z_path(ar.LAW_BETAS, got['emin'], got['wsum'], ar.LAW_M, 8.0)[-1]
    print('largest deviation %.2f sigma over %d bins; log2 Z %.6f (exact %.6f)' % (z, bins, lz, ar.exact_log2Z(c['cells'], 2, 2, ar.LAW_BETAS[-1])))
    assert ok


# ---------------------------------------------------------------------------------------------- 7. the public call
def _random_states(ins, M, seed):
    qs = ins._cell_sizes()[ins.order]                                    # model order
    return np.random.default_rng(seed).integers(0, qs[None, :], size=(M, qs.size))


PUBLIC = ['ising3x3', 'chimera', 'rmf3x3']


@pytest.mark.parametrize('name', PUBLIC)
def test_public_call(name):
    """40 random states, 4 steps of 2 sweeps with given uniforms: model-order states and energies equal the reference run on solver_cells;
    anneal_log2Z is the host formula on the reference's Emin and W; what is stored and what is reset; steps_per_call in {1, 2, None},
    uniforms on the device and record on / off give the same result; M= with betas[0] = 0 reproduces the init rule."""
    from tnac4o_amd import anneal as an
    betas = [0.2, 0.5, 0.9, 1.4, 2.0]
    M, K, sweeps = 40, 5, 2
    rng = np.random.default_rng(51)

    def fresh():
        ins = small(name, 1.0)
        ins.states = _random_states(ins, M, 50)
        return ins

    ins = fresh()
    start = np.copy(ins.states)
    ncell = ins.Nx * ins.Ny
    shapes = an.uniform_shapes(K, sweeps, ncell, M)
    u = {k: rng.random(shapes[k]) for k in an.STEP_KEYS}
    cells = solver_cells(ins)
    rot = np.empty_like(start)
    rot[:, ins.order] = start
    ref = ar.run(cells, ins.Nx, ins.Ny, rot, np.arange(M), betas, sweeps, u['sweep'], u['resample'])
    assert ref['margin'] >= 1e-9 and ref['resample_margin'] >= ar.delta(M)
    ins.degeneracy = 5
    ins.probability = np.zeros(M)
    E = ins.anneal_population(betas, sweeps=sweeps, uniforms=u, record=True)
    assert not hasattr(ins, 'rhoT') and ins.degeneracy == 5
    assert E is ins.energy and same_bits(E, ref['energy']) and np.array_equal(ins.states, ref['states'][:, ins.order]) and not np.array_equal(ins.states, start)
    assert same_bits(ins.anneal_betas, np.array(betas)) and np.array_equal(ins.anneal_family, ref['family'])
    assert np.array_equal(ins.anneal_survivors, ref['survivors']) and np.array_equal(ins.anneal_parent_trace, ref['parent_trace'])
    assert same_bits(ins.anneal_energy_trace, ref['energy_trace'])
    want = an.log2Z_path(betas, ref['emin'], ref['wsum'], M, 0.0)
    # (W within (M + 8) 2^-52 of the reference's moves a step's log2 by 2e-14; four steps and the rounding of sums of size 100 stay below 1e-12)
    assert ins.anneal_log2Z.shape == (K,) and ins.anneal_log2Z[0] == 0.0 and np.allclose(ins.anneal_log2Z, want, rtol=0, atol=1e-12)
    assert same_bits(ins.anneal_free_energy, an.free_energy_path(betas, ins.anneal_log2Z))
    E_all = np.concatenate([rr.total_energy(cells, ins.Nx, ins.Ny, rot)[None, :], ref['energy_trace']])
    assert np.allclose(ins.anneal_energy_mean, E_all.mean(axis=1), rtol=1e-14) and np.allclose(ins.anneal_heat_capacity, np.array(betas) ** 2 * E_all.var(axis=1), rtol=1e-12)
    assert np.allclose(ins.anneal_ess, ref['wsum'] ** 2 / ref['w2sum'], rtol=1e-12) and np.all(ins.anneal_ess <= M)
    assert (ins.anneal_rho_t, ins.anneal_family_entropy) == an.family_statistics(ref['family'])
    assert ins.probability is None and ins.sample_log2Z is None and ins.log2Z_lower is None and ins.log2Z_estimate is None
    for per, dev_u, record in ((1, False, False), (2, True, True), (None, False, False)):
        other = fresh()
        uu = {k: torch.as_tensor(v).cuda() for k, v in u.items()} if dev_u else u
        other.anneal_population(betas, sweeps=sweeps, uniforms=uu, steps_per_call=per, record=record)
        assert np.array_equal(other.states, ins.states) and same_bits(other.energy, ins.energy) and np.array_equal(other.anneal_family, ins.anneal_family)
        assert same_bits(other.anneal_log2Z, ins.anneal_log2Z) and same_bits(other.anneal_ess, ins.anneal_ess)
        assert np.array_equal(other.anneal_survivors, ins.anneal_survivors) and same_bits(other.anneal_heat_capacity, ins.anneal_heat_capacity)
        assert hasattr(other, 'anneal_parent_trace') == record
    # a drawn population: betas[0] = 0, cells of 'init' in the walk order of the rotation
    zero = [0.0] + betas
    shapes = an.uniform_shapes(K + 1, sweeps, ncell, M)
    u0 = {k: rng.random(shapes[k]) for k in an.STEP_KEYS + ('init',)}
    drawn = small(name, 1.0)
    drawn.anneal_population(zero, sweeps=sweeps, M=M, uniforms=u0)
    qs = drawn._cell_sizes()
    init = np.minimum(np.floor(u0['init'] * qs[None, :]).astype(np.int64), qs[None, :] - 1)
    ref0 = ar.run(cells, ins.Nx, ins.Ny, init, np.arange(M), zero, sweeps, u0['sweep'], u0['resample'])
    assert ref0['margin'] >= 1e-9 and ref0['resample_margin'] >= ar.delta(M)
    assert np.array_equal(drawn.states, ref0['states'][:, drawn.order]) and same_bits(drawn.energy, ref0['energy'])
    assert drawn.anneal_log2Z[0] == pytest.approx(float(np.sum(np.log2(qs)))) and np.isnan(drawn.anneal_free_energy[0])
    assert np.allclose(drawn.anneal_log2Z, an.log2Z_path(zero, ref0['emin'], ref0['wsum'], M, drawn.anneal_log2Z[0]), rtol=0, atol=1e-12)
    # one beta: nothing moves, the energies are there
    idle = fresh()
    idle.anneal_population([0.7])
    assert np.array_equal(idle.states, start) and same_bits(idle.energy, E_all[0]) and idle.anneal_log2Z.tolist() == [0.0] and idle.anneal_ess.shape == (0,)
    assert idle.anneal_rho_t == pytest.approx(1.0)


def test_public_call_draws_from_the_global_generator():
    """uniforms=None: init first, then per block of steps resample, sweep from numpy's global generator."""
    from tnac4o_amd import anneal as an
    betas = [0.0, 0.4, 0.8, 1.2]
    a = small('chimera', 1.0)
    np.random.seed(19)
    a.anneal_population(betas, M=16, steps_per_call=2)
    np.random.seed(19)
    shapes = an.uniform_shapes(4, 1, 4, 16)
    u = {'init': np.random.rand(16, 4)}
    blocks = [an.draw_block(shapes, 0, 2), an.draw_block(shapes, 2, 3)]
    u.update({k: np.concatenate([blk[k] for blk in blocks]) for k in an.STEP_KEYS})
    b = small('chimera', 1.0)
    b.anneal_population(betas, M=16, uniforms=u)
    assert np.array_equal(a.states, b.states) and same_bits(a.energy, b.energy) and same_bits(a.anneal_log2Z, b.anneal_log2Z)
