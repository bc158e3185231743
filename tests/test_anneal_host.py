"""Host side of tnac4o.anneal_population (tnac4o_amd/anneal.py), the reference of tests/anneal_ref.py -- the defining property of
systematic resampling, the margins of the shared inputs, unbiasedness of Z, the law of the final population, cutting the schedule --
and the argument errors of tn_anneal.  No GPU."""
import ctypes as ct

import numpy as np
import pytest

import anneal_ref as ar
import relax_ref as rr
from overlap_ref import droplet, ising3x3, last_error, rmf
from tnac4o_amd import anneal as an


# ---------------------------------------------------------------------------------------------- systematic resampling
def test_expected_copy_counts():
    """The mean of n_m(u) over u = (i + 1/2) / G equals M w_m / W within 1 / G, sum n_m = M for every u, and every n_m is the floor or
    the ceiling of M w_m / W."""
    rng = np.random.default_rng(3)
    M, G = 37, 512
    w = rng.random(M) ** 3
    w[5] = 0.0
    counts = np.array([ar.offsets(w, (i + 0.5) / G)['counts'] for i in range(G)])
    assert np.all(counts.sum(axis=1) == M) and np.all(counts >= 0)
    want = M * w / w.sum()
    worst = float(np.max(np.abs(counts.mean(axis=0) - want)))
    print('largest |mean n_m - M w_m / W| = %.2e (1 / G = %.2e)' % (worst, 1.0 / G))
    assert worst <= 1.0 / G
    assert np.all(counts >= np.floor(want)[None, :] - (np.arange(M) == M - 1)) and np.all(counts <= np.ceil(want)[None, :] + (np.arange(M) == M - 1))
    assert np.all(counts[:, 5] == 0)


def test_degenerate_weights():
    """Equal weights give the identity; one dominating weight (the others underflow to 0) gives M copies of that row; energies that
    are all NaN give the identity; a NaN among finite energies gets no copy."""
    M = 9
    r = ar.offsets(np.ones(M), 0.37)
    assert np.array_equal(r['parent'], np.arange(M)) and np.all(r['counts'] == 1)
    E = np.full(M, 3.0)
    E[4] = -5.0
    emin, w = ar.weights(E, 1000.0)
    assert emin == -5.0 and w[4] == 1.0 and np.count_nonzero(w) == 1
    for u in (0.0, 0.5, np.nextafter(1.0, 0.0)):
        r = ar.offsets(w, u)
        assert np.all(r['parent'] == 4) and r['counts'][4] == M and r['wsum'] == 1.0
    emin, w = ar.weights(np.full(M, np.nan), 0.5)
    assert np.isnan(emin) and np.all(w == 0.0)
    r = ar.offsets(w, 0.2)
    assert np.array_equal(r['parent'], np.arange(M)) and r['wsum'] == 0.0 and r['margin'] == np.inf
    E = np.arange(M, dtype=np.float64)
    E[2] = np.nan
    emin, w = ar.weights(E, 0.1)
    assert emin == 0.0 and w[2] == 0.0 and np.all(ar.offsets(w, 0.6)['counts'][2] == 0)


# ---------------------------------------------------------------------------------------------- conditions on the shared inputs
@pytest.mark.parametrize('case', ar.CASES, ids=ar.CASE_IDS)
def test_margins_of_the_shared_inputs(case):
    """A condition on the INPUTS: the reference keeps every heat-bath draw at least 1e-9 W away from a running sum and every
    C_m / W * M + u at least delta(M) = 4 M (M + 8) 2^-52 away from an integer, so a last-bit difference of exp or another
    order of the additions on the device cannot change an offset.  The resampling is no identity: rows die."""
    ref = ar.case_reference(case)
    M = case[2]
    print('draw margin %.3e, resampling margin %.3e (delta %.3e), survivors %s' % (ref['margin'], ref['resample_margin'], ar.delta(M), ref['survivors']))
    assert ref['margin'] >= 1e-9 and ref['resample_margin'] >= ar.delta(M)
    assert M == 1 or np.all(ref['survivors'] < M)
    assert np.all(np.bincount(ref['parent_trace'].ravel(), minlength=M) <= 3 * M) and ref['family'].shape == (M,)


@pytest.mark.parametrize('M,seed', ar.TILE_CASES, ids=['M%d' % c[0] for c in ar.TILE_CASES])
def test_margins_of_the_tile_inputs(M, seed):
    ref = ar.tile_reference(M, seed)
    print('resampling margin %.3e (delta %.3e), survivors %s' % (ref['resample_margin'], ar.delta(M), ref['survivors']))
    assert ref['resample_margin'] >= ar.delta(M) and np.all(ref['survivors'] < M)


# ---------------------------------------------------------------------------------------------- Z and the law
def test_Z_is_unbiased():
    """relax_ref.law_problem(), betas from 0 to 0.7 in 8 steps, M = 2^12, 2 sweeps, 16 fixed seeds: the mean of Zhat / Z over the runs lies
    within 5 standard errors (computed from those runs) of 1; Z by enumeration.  The spread is printed, it is no condition."""
    cells, _ = rr.law_problem()
    exact = ar.exact_log2Z(cells, 2, 2, ar.LAW_BETAS[-1])
    ratio = []
    for seed in ar.Z_SEEDS:
        ref = ar.law_reference(ar.Z_M, seed)
        assert ref['margin'] >= 1e-9 and ref['resample_margin'] >= ar.delta(ar.Z_M)
        ratio.append(2.0 ** (an.log2Z_path(ar.LAW_BETAS, ref['emin'], ref['wsum'], ar.Z_M, 8.0)[-1] - exact))
    ratio = np.array(ratio)
    se = ratio.std(ddof=1) / np.sqrt(ratio.size)
    print('Zhat / Z over %d runs: mean %.5f, standard error %.5f, spread %.5f' % (ratio.size, ratio.mean(), se, ratio.std(ddof=1)))
    assert abs(ratio.mean() - 1.0) <= 5.0 * se
    assert an.log2Z_path([0.0], [], [], 7, 8.0).tolist() == [8.0]


def test_law_of_the_final_population():
    """One such run at M = 2^14 against the exact Boltzmann law at 0.7: bins with M p < 20 pooled, every bin within 6 sigma, with the
    2 sweeps per step of the run (family members are correlated; the sweeps take them apart)."""
    cells, _ = rr.law_problem()
    ref = ar.law_reference(ar.LAW_M, ar.LAW_SEED)
    assert ref['margin'] >= 1e-9 and ref['resample_margin'] >= ar.delta(ar.LAW_M)
    _, pi = rr.boltzmann(cells, 2, 2, ar.LAW_BETAS[-1])
    ok, z, bins = rr.law_statistic(rr.configuration_index(ref['states']), pi)
    rho, ent = an.family_statistics(ref['family'])
    print('largest deviation %.2f sigma over %d bins; rho_t %.2f, family entropy %.2f' % (z, bins, rho, ent))
    assert ok
    assert 1.0 < rho < 10.0


def test_cutting_the_reference_into_calls():
    case = ar.CASES[-1]
    c = ar.case_inputs(case, 6)
    whole = ar.run_case(c)
    part, traces = None, []
    for lo, hi in ((0, 1), (1, 3), (3, 5)):
        part = ar.run_case(c, lo=lo, hi=hi, state=part)
        traces.append(part)
    for k in ('states', 'family', 'energy'):
        assert np.array_equal(part[k], whole[k]), k
    for k in ('emin', 'wsum', 'w2sum', 'survivors', 'energy_trace', 'parent_trace'):
        assert np.array_equal(np.concatenate([p[k] for p in traces]), whole[k]), k


# ---------------------------------------------------------------------------------------------- the driver's host parts
def test_family_statistics_and_paths():
    fam = np.array([0, 0, 0, 3, 3, 7, 7, 7, 7, 9])
    rho, ent = an.family_statistics(fam)
    p = np.array([0.3, 0.2, 0.4, 0.1])
    assert rho == pytest.approx(10 * (0.09 + 0.04 + 0.16 + 0.01), rel=1e-15) and ent == pytest.approx(-np.sum(p * np.log(p)), rel=1e-15)
    assert an.family_statistics(np.arange(6)) == pytest.approx((1.0, np.log(6.0))) and an.family_statistics(np.zeros(6, dtype=int)) == (6.0, 0.0)
    betas = np.array([0.0, 0.5, 1.5])
    lz = an.log2Z_path(betas, [-2.0, -3.0], [4.0, 2.0], 8, 5.0)
    want1 = 5.0 + np.log2(0.5) + 0.5 * 2.0 / np.log(2.0)
    want2 = want1 + np.log2(0.25) + 1.0 * 3.0 / np.log(2.0)
    assert np.allclose(lz, [5.0, want1, want2], rtol=1e-15, atol=0)
    assert an.log2Z_path(betas, [0.0, np.nan], [8.0, 0.0], 8, 0.0)[1] == 0.0
    F = an.free_energy_path(betas, lz)
    assert np.isnan(F[0]) and np.allclose(F[1:], -lz[1:] * np.log(2.0) / betas[1:], rtol=1e-15)
    q = np.array([3, 1, 4])
    u = np.array([[0.0, 0.9, 0.25], [np.nextafter(1.0, 0.0), 0.0, 0.9999]])
    assert an.draw_population(u, q).tolist() == [[0, 0, 1], [2, 0, 3]]
    shapes = an.uniform_shapes(5, 2, 16, 48)
    assert shapes == {'resample': (4,), 'sweep': (4, 2, 16, 48), 'init': (48, 16)}
    assert an.step_bytes(shapes, 48, False) == (1 + 2 * 16 * 48) * 8 + 48 * 8 and an.step_bytes(shapes, 48, True) == an.step_bytes(shapes, 48, False) + 192
    np.random.seed(3)
    blk = an.draw_block(shapes, 1, 3)
    np.random.seed(3)
    assert np.array_equal(blk['resample'], np.random.rand(2)) and np.array_equal(blk['sweep'], np.random.rand(2, 2, 16, 48)) and set(blk) == {'resample', 'sweep'}


def test_cell_states_enumerate_the_active_spins():
    """The convention of anneal_log2Z: the default log2Z0 at betas[0] = 0, sum_k log2 q_k, is the number of active spins of an Ising
    model -- the configurations calculate_free_energy's Z runs over."""
    from tnac4o_amd import overlap as ov
    for s in (droplet(), ising3x3()):
        s.states = np.zeros((2, s.Nx * s.Ny), dtype=s.indtype)
        a = an.check_arguments(s, [0.0, 1.0], 1, None, None, None, None)
        assert a['log2Z0'] == float(ov.active_spins(s).size)
    r = rmf()
    a = an.check_arguments(r, [0.0, 1.0], 1, 4, None, None, None)
    assert a['log2Z0'] == pytest.approx(float(np.sum(np.log2(r._cell_sizes())))) and a['fresh'] and a['states'] is None
    r.states = np.zeros((4, 9), dtype=r.indtype)
    assert an.check_arguments(r, [0.5, 1.0], 1, None, None, None, None)['log2Z0'] == 0.0
    assert an.check_arguments(r, [0.5, 1.0], 1, None, None, 2.5, 3)['log2Z0'] == 2.5


def test_public_call_value_errors():
    """Every refusal of anneal.py / anneal_population is raised before device work (this test has no device)."""
    torch = pytest.importorskip('torch')
    s = droplet()
    with pytest.raises(ValueError, match='stored states'):
        s.anneal_population([0.0, 1.0])
    s.states = np.random.default_rng(4).integers(0, 256, (6, 16)).astype(s.indtype)
    kept = np.copy(s.states)
    for bad in ([], [[0.5, 1.0]], [1.0, 0.5], [0.5, 0.5], [-0.1, 1.0], [0.5, np.inf], [0.5, np.nan], [np.nan], 'ab', None):
        with pytest.raises(ValueError, match='betas'):
            an.check_schedule(bad)
        with pytest.raises(ValueError, match='betas'):
            s.anneal_population(bad)
    assert an.check_schedule([0.0]).tolist() == [0.0] and an.check_schedule((0, 1, 2.5)).dtype == np.float64
    betas = [0.2, 0.6, 1.0]
    for kw, word in ((dict(sweeps=-1), 'sweeps'), (dict(sweeps=0.5), 'sweeps'), (dict(sweeps=True), 'sweeps'), (dict(steps_per_call=0), 'steps_per_call'),
                     (dict(steps_per_call=1.5), 'steps_per_call'), (dict(M=0), 'M must'), (dict(M=2.5), 'M must'), (dict(M=8), r'betas\[0\] = 0'),
                     (dict(log2Z0=np.inf), 'log2Z0'), (dict(log2Z0='x'), 'log2Z0'), (dict(uniforms=np.zeros(3)), 'uniforms'),
                     (dict(uniforms={'sweep': np.zeros((2, 1, 16, 6))}), 'uniforms'),
                     (dict(uniforms={'sweep': np.zeros((2, 1, 16, 6)), 'resample': np.zeros(2), 'init': np.zeros((6, 16))}), 'uniforms')):
        with pytest.raises(ValueError, match=word):
            s.anneal_population(betas, **kw)
    ok = {'sweep': np.zeros((2, 1, 16, 6)), 'resample': np.zeros(2)}
    for key, bad in (('sweep', np.zeros((2, 1, 16, 5))), ('sweep', np.zeros((2, 1, 16, 6), dtype=np.float32)), ('sweep', np.ones((2, 1, 16, 6))),
                     ('resample', np.zeros(3)), ('resample', np.full(2, np.nan)), ('resample', [0.0, 0.0]), ('resample', np.full(2, -0.5)),
                     ('resample', torch.zeros(2)), ('resample', torch.ones(2, dtype=torch.float64))):
        u = dict(ok)
        u[key] = bad
        with pytest.raises(ValueError, match=key):
            s.anneal_population(betas, uniforms=u)
    fresh = {'sweep': np.zeros((1, 1, 16, 4)), 'resample': np.zeros(1), 'init': np.zeros((4, 16))}
    with pytest.raises(ValueError, match='uniforms'):                    # a drawn population needs 'init'
        s.anneal_population([0.0, 1.0], M=4, uniforms={k: fresh[k] for k in ('sweep', 'resample')})
    for bad in (np.zeros((4, 15)), np.ones((4, 16)), np.full((4, 16), np.nan)):
        with pytest.raises(ValueError, match='init'):
            s.anneal_population([0.0, 1.0], M=4, uniforms=dict(fresh, init=bad))
    assert np.array_equal(s.states, kept) and not hasattr(s, 'anneal_log2Z') and not hasattr(s, 'anneal_betas')
    s.states = np.full((6, 16), 256)
    with pytest.raises(ValueError, match='states'):
        s.anneal_population(betas)


# ---------------------------------------------------------------------------------------------- argument errors of the export
def test_anneal_argument_errors():
    """rc = -1 / -3 with a message that starts with tn_anneal and names the limit, nothing launched: the device pointers below are not
    device memory, they are never followed.  tn_anneal_ws_bytes returns 0 on the shapes the call refuses."""
    from tnac4o_amd import _lib
    from tnac4o_amd.beam import _Cell
    L = _lib.lib()
    p = 4096                                                             # stands for a non-null device pointer
    Nx = Ny = 2

    def table(q=4):
        cells = (_Cell * 4)()
        for k in range(4):
            cells[k].q, cells[k].Es, cells[k].E1, cells[k].E4, cells[k].e1cols, cells[k].e4cols = q, p, p, p, 4, 4
        return cells

    cells, M = table(), 12

    def arr(*v):
        return (ct.c_double * len(v))(*v)

    good = arr(0.0, 0.5, 2.0)

    def call(Nx=Nx, Ny=Ny, cells=cells, M=M, K=3, betas=good, states=p, family=p, sweeps=1, usweep=p, ldu=M, ures=p, E=p, emin=p, wsum=p, w2sum=p,
             surv=p, ws=p, wsb=None):
        if wsb is None:
            wsb = max(int(L.tn_anneal_ws_bytes(Nx, Ny, M)), 1)
        return L.tn_anneal(Nx, Ny, ct.cast(cells, ct.c_void_p) if cells is not None else None, M, K,
                           ct.cast(betas, ct.c_void_p) if betas is not None else None, states, family, sweeps, usweep, ldu, ures, E, emin, wsum, w2sum,
                           surv, None, None, ws, wsb, None)

    bad_cells = table()
    bad_cells[2].q = 40000
    for kw, word in ((dict(Nx=0), 'Nx'), (dict(cells=None), 'cells'), (dict(M=0), 'M'), (dict(M=2 ** 31), 'M'), (dict(K=0), 'K'), (dict(betas=None), 'betas'),
                     (dict(betas=arr(0.5, 0.5, 2.0)), 'increasing'), (dict(betas=arr(1.0, 0.5, 2.0)), 'increasing'), (dict(betas=arr(-0.5, 0.5, 2.0)), 'negative'),
                     (dict(betas=arr(0.0, 1.0, float('inf'))), 'finite'), (dict(betas=arr(0.5, float('nan'), 2.0)), 'betas'),
                     (dict(betas=arr(float('nan'), 1.0, 2.0)), 'betas'), (dict(sweeps=-1), 'sweeps'), (dict(states=None), 'states'), (dict(family=None), 'family'),
                     (dict(E=None), 'energy_out'), (dict(ures=None), 'ures'), (dict(emin=None), 'emin_out'), (dict(wsum=None), 'wsum_out'),
                     (dict(w2sum=None), 'w2sum_out'), (dict(surv=None), 'survivors_out'), (dict(usweep=None), 'usweep'), (dict(ldu=M - 1), 'ldu'),
                     (dict(cells=bad_cells), '32767'), (dict(ws=None), 'ws')):
        assert call(**kw) == -1, kw
        msg = last_error(L)
        assert msg.startswith('tn_anneal') and word in msg, (kw, msg)
    need = int(L.tn_anneal_ws_bytes(Nx, Ny, M))
    assert need > 0 and call(wsb=need - 1) == -3
    msg = last_error(L)
    assert msg.startswith('tn_anneal') and 'workspace' in msg and str(need) in msg
    assert call(K=1, ures=None, emin=None, wsum=None, w2sum=None, surv=None, usweep=None, wsb=need - 1) == -3       # K = 1 needs none of them
    assert call(sweeps=0, usweep=None, ldu=0, wsb=need - 1) == -3                                                    # nor sweeps = 0 its numbers
    assert int(L.tn_anneal_ws_bytes(Nx, Ny, 1000 * M)) >= 1000 * M * (2 * 4 + 20)       # the second copy of the rows, family, l, O, parent
    for shape in ((0, 2, 12), (2, 0, 12), (2, 2, 0), (2, 2, 2 ** 31), (2 ** 20, 2 ** 20, 12), (2 ** 15, 2 ** 15, 2 ** 30)):
        assert int(L.tn_anneal_ws_bytes(*shape)) == 0, shape


@pytest.mark.parametrize('case', ar.WIDTH_CASES, ids=['%dx%d' % c[:2] for c in ar.WIDTH_CASES])
def test_margins_of_the_width_inputs(case):
    ref = ar.width_reference(case)
    print('draw margin %.3e, resampling margin %.3e (delta %.3e), survivors %s' % (ref['margin'], ref['resample_margin'], ar.delta(case[3]), ref['survivors']))
    assert ref['margin'] >= 1e-9 and ref['resample_margin'] >= ar.delta(case[3]) and np.all(ref['survivors'] < case[3])
