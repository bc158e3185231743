"""Host side of tnac4o.temper_samples (tnac4o_amd/temper.py), the reference of tests/temper_ref.py -- margins of the shared inputs,
invariance of a round, conservation in the cluster step, the assignment's invariant, the statistic on the reference chain -- and the
argument errors of tn_temper.  No GPU."""
import ctypes as ct

import numpy as np
import pytest

import relax_ref as rr
import temper_ref as tr
from overlap_ref import droplet, ising3x3, last_error, rmf
from tnac4o_amd import temper as tp


# ---------------------------------------------------------------------------------------------- conditions on the shared inputs
@pytest.mark.parametrize('case', tr.CASES, ids=tr.CASE_IDS)
def test_margins_of_the_shared_inputs(case):
    """A condition on the INPUTS: the reference keeps every draw at least 1e-9 W away from a running sum (the bound of DESIGN §18) and
    every swap decision with D < 0 at least 1e-9 away from exp(D), so a last-bit difference of exp or of the summation order on the
    device cannot change a decision.  Both parities occur, swaps are accepted and refused."""
    ref = tr.case_reference(case)
    print('draw margin %.3e, swap margin %.3e, accepted %s of %s' % (ref['margin'], ref['swap_margin'], ref['accepted'], ref['attempted']))
    assert ref['margin'] >= 1e-9 and ref['swap_margin'] >= 1e-9
    c = tr.case_inputs(case)
    T, R = c['betas'].size, c['states'].shape[0] // c['betas'].size
    want = np.array([2 * R if t + 1 < T else 0 for t in range(T - 1)])   # 4 rounds: each parity twice
    assert np.array_equal(ref['attempted'], want) and ref['accepted'].sum() > 0 and np.any(ref['accepted'] < ref['attempted'])
    assert tr.assignment_consistent(ref['tidx'], ref['slot'])
    for r in range(tr.ROUNDS):                                           # ... after every round
        chain = np.arange(ref['tidx'].size) // T
        assert all(np.array_equal(np.sort(ref['tidx_trace'][r][chain == k]), np.arange(T)) for k in range(R))
    assert not np.array_equal(ref['tidx'], c['tidx'])


def test_cluster_step_conserves_the_pair_energy():
    """(b): E_a + E_b of every row pair is exactly what it was across the cluster step (integer couplings), clusters of more than one
    spin and fewer than all differing spins occur, and the tables give the energy of the couplings they were tabulated from."""
    case = tr.CASES[-1]
    ref, c = tr.case_reference(case), tr.case_inputs(case)
    assert len(ref['pair_sums']) == tr.ROUNDS * 2 * 3
    assert all(a == b for a, b in ref['pair_sums'])
    assert np.any((ref['sizes'] > 1) & (ref['sizes'] < ref['differing'])) and np.all(ref['sizes'] >= 1)
    lat = tr.ising_lattice()
    assert lat['nbits'] == 68 and sorted({rr_class(cell['q']) for cell in lat['cells']}) == [0, 1, 2]
    assert np.array_equal(rr.total_energy(lat['cells'], 4, 4, c['states']), tr.ising_energy(lat, c['states']).astype(np.float64))
    assert np.array_equal(ref['energy'], tr.ising_energy(lat, ref['states']).astype(np.float64))


def rr_class(q):
    return 0 if q <= 8 else 1 if q <= 32 else 2 if q <= 256 else 3


def test_bits_round_trip():
    lat = tr.ising_lattice()
    c = tr.case_inputs(tr.CASES[-1])
    rows = tr.to_bits(lat['cells'], c['states'], lat['nbits'], lat['bitcell'])
    assert np.array_equal(tr.from_bits(lat['cells'], c['states'], rows, lat['nbits'], lat['cellbits']), c['states'])
    flipped = [v ^ ((1 << 68) - 1) for v in rows]                        # every spin flipped: every state complemented
    qs = np.array([cell['q'] for cell in lat['cells']])
    assert np.array_equal(tr.from_bits(lat['cells'], c['states'], flipped, lat['nbits'], lat['cellbits']), qs[None, :] - 1 - c['states'])
    bad = lat['cellbits'].copy()
    bad[3, 0], bad[7, 1] = 68, 2 ** 31 - 1                               # positions outside the row are skipped
    out = tr.from_bits(lat['cells'], c['states'], flipped, lat['nbits'], bad)
    assert np.array_equal(out[:, 3] & 1, c['states'][:, 3] & 1) and np.array_equal((out[:, 7] >> 1) & 1, (c['states'][:, 7] >> 1) & 1)


# ---------------------------------------------------------------------------------------------- the law
def test_one_round_keeps_the_product_law():
    """The exact round of the reference on relax_ref.law_problem() (2 x 2 cells of q = 4), T = 2, one chain, as a map on the joint law
    mu (256 x 256): mu <- P_b0^T mu P_b1, then the swap.  pi_b0 x pi_b1 is invariant to 1e-14 in the 1-norm, with and without the swap;
    another law is not."""
    cells, _ = rr.law_problem()
    betas = np.array(tr.LAW_BETAS)
    P0, P1 = rr.sweep_matrix(cells, 2, 2, betas[0]), rr.sweep_matrix(cells, 2, 2, betas[1])
    a = tr.swap_acceptance(cells, betas)
    pi = np.outer(rr.boltzmann(cells, 2, 2, betas[0])[1], rr.boltzmann(cells, 2, 2, betas[1])[1])
    for swap in (True, False):
        err = float(np.abs(tr.joint_round(pi, P0, P1, a, swap) - pi).sum())
        print('swap %s: |round(pi0 x pi1) - pi0 x pi1|_1 = %.2e' % (swap, err))
        assert err <= 1e-14
    assert float(np.abs(pi * (1 - a) + pi.T * a.T - pi).sum()) <= 1e-14  # the swap alone
    assert np.any((a > 0) & (a < 1))
    other = np.outer(rr.boltzmann(cells, 2, 2, betas[1])[1], rr.boltzmann(cells, 2, 2, betas[0])[1])
    assert float(np.abs(tr.joint_round(other, P0, P1, a, True) - other).sum()) > 1e-3


def test_the_reference_chain_passes_the_statistic():
    """The statistical test of tests/test_gpu_temper.py on the reference chain alone: the same inputs, the same pooling."""
    cells, betas, states, usweep, uswap, marginals = tr.law_inputs()
    tidx, slot = tr.fresh_assignment(states.shape[0], 2)
    ref = tr.run(cells, 2, 2, states, betas, tidx, slot, 0, tr.LAW_ROUNDS, 1, usweep, uswap=uswap)
    assert ref['margin'] >= 1e-9 and ref['swap_margin'] >= 1e-9
    for t, (ok, z, bins) in enumerate(tr.law_check(ref['states'], ref['tidx'], marginals)):
        print('temperature %d: largest deviation %.2f sigma over %d bins' % (t, z, bins))
        assert ok
    assert 0 < ref['accepted'][0] < ref['attempted'][0] == 2 * tr.LAW_R


def test_cutting_the_reference_into_calls():
    case = tr.CASES[-1]
    c = tr.case_inputs(case)
    whole = tr.case_reference(case)
    part = tr.run_case(c, lo=0, hi=1)
    part = tr.run_case(c, lo=1, hi=4, state=part)
    for k in ('states', 'tidx', 'slot', 'energy', 'accepted', 'attempted'):
        assert np.array_equal(part[k], whole[k]), k


# ---------------------------------------------------------------------------------------------- the driver's host parts
def test_bit_tables_follow_binary_states():
    """cellbits / bitcell of the droplet in both rotations against binary_states / states_from_binary: converting random states to spin
    bits through the tables gives overlap.spin_bits, and back gives the states."""
    from tnac4o_amd import overlap as ov
    for rot in (0, 1):
        s = droplet()
        if rot:
            s.rotate_graph(1)
        n, cellbits, bitcell = tp.bit_tables(s)
        act = ov.active_spins(s)
        assert n == act.size and cellbits.dtype == np.int32 and bitcell.shape == (n, 2)
        s.states = np.random.default_rng(2).integers(0, 256, (5, 16))
        rotst = np.empty_like(s.states)
        rotst[:, s.order] = s.states                                    # the device's order
        cells = [dict(q=int(q)) for q in s._cell_sizes()]
        rows = tr.to_bits(cells, rotst, n, bitcell)
        want = ov.spin_bits(s)
        assert all(rows[m] == sum(int(b) << p for p, b in enumerate(want[m])) for m in range(5))
        assert np.array_equal(tr.from_bits(cells, np.zeros_like(rotst), rows, n, cellbits), rotst)
        for k in range(16):
            for j in range(cellbits.shape[1]):
                if cellbits[k, j] >= 0:
                    assert tuple(bitcell[cellbits[k, j]]) == (k, j)


def test_plan_and_trace_helpers():
    shapes = tp.uniform_shapes(7, 2, 16, 48, 3, 2, 8)
    assert shapes == {'sweep': (7, 2, 16, 48), 'cluster': (7, 2, 8), 'swap': (7, 16, 2)}
    per = tp.round_bytes(shapes, 48, False)
    assert per == (2 * 16 * 48 + 16 + 32) * 8 and tp.round_bytes(shapes, 48, True) == per + 48 * 12 + 16 * 8
    assert tp.plan_rounds(7, per, 3 * per + 1) == 3 and tp.plan_rounds(7, per, 0) == 1 and tp.plan_rounds(7, per, 10 ** 12) == 7
    assert tp.plan_rounds(0, per, 10 ** 12) == 1
    E = np.arange(12.0).reshape(2, 6)
    tidx = np.array([[0, 1, 2, 2, 0, 1], [1, 0, 2, 0, 2, 1]])
    out = tp.reorder_trace(E, tidx, 3)
    assert out.shape == (2, 3, 2) and out[0].tolist() == [[0, 4], [1, 5], [2, 3]] and out[1].tolist() == [[7, 9], [6, 11], [8, 10]]
    np.random.seed(3)
    blk = tp.draw_block(shapes, 2, 5)
    np.random.seed(3)
    assert np.array_equal(blk['sweep'], np.random.rand(3, 2, 16, 48)) and np.array_equal(blk['cluster'], np.random.rand(3, 2, 8))
    assert np.array_equal(blk['swap'], np.random.rand(3, 16, 2))


def test_public_call_value_errors():
    """Every refusal of temper.py / temper_samples is raised before device work (this test has no device)."""
    torch = pytest.importorskip('torch')
    s = droplet()
    betas = [0.5, 1.0]
    with pytest.raises(ValueError, match='stored states'):
        s.temper_samples(betas)
    s.states = np.random.default_rng(4).integers(0, 256, (6, 16)).astype(s.indtype)
    kept = np.copy(s.states)
    for bad in ([], [[0.5, 1.0]], [1.0, 0.5], [0.5, 0.5], [0.0, 1.0], [-1.0, 1.0], [0.5, np.inf], [0.5, np.nan], 'ab', None):
        with pytest.raises(ValueError, match='betas'):
            s.temper_samples(bad)
    with pytest.raises(ValueError, match='multiple'):
        s.temper_samples([0.2, 0.4, 0.6, 0.8])
    for kw, word in ((dict(rounds=-1), 'rounds'), (dict(rounds=1.5), 'rounds'), (dict(sweeps=-1), 'sweeps'), (dict(sweeps=0.5), 'sweeps'),
                     (dict(keep=2), 'keep'), (dict(keep=-1), 'keep'), (dict(keep=0.5), 'keep'), (dict(rounds_per_call=0), 'rounds_per_call'),
                     (dict(rounds_per_call=1.5), 'rounds_per_call'), (dict(cluster_beta_min=np.nan), 'cluster_beta_min'),
                     (dict(cluster_moves=False, pairs=np.zeros((10, 1, 2), dtype=np.int64)), 'pairs'),
                     (dict(cluster_moves=False, cluster_beta_min=0.7), 'cluster_beta_min'),
                     (dict(rounds=1, pairs=np.array([[[0, 3]]])), 'pairs'), (dict(rounds=1, pairs=np.array([[[0, 0]]])), 'pairs'),
                     (dict(rounds=2, pairs=np.array([[[0, 1]]])), 'pairs'), (dict(uniforms=np.zeros(3)), 'uniforms'),
                     (dict(uniforms={'sweep': np.zeros((10, 1, 16, 6))}), 'uniforms')):
        with pytest.raises(ValueError, match=word):
            s.temper_samples(betas, **kw)
    with pytest.raises(ValueError, match='two chains'):                  # R = 1
        s.temper_samples([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    ok = {'sweep': np.zeros((1, 1, 16, 6)), 'cluster': np.zeros((1, 2, 1)), 'swap': np.zeros((1, 3, 1))}
    p = np.array([[[0, 2]]])
    for key, bad in (('sweep', np.zeros((1, 1, 16, 5))), ('sweep', np.zeros((1, 1, 16, 6), dtype=np.float32)), ('sweep', np.ones((1, 1, 16, 6))),
                     ('cluster', np.zeros((1, 1, 1))), ('cluster', np.full((1, 2, 1), np.nan)), ('cluster', [[[0.0], [0.0]]]),
                     ('swap', np.zeros((1, 3, 2))), ('swap', np.full((1, 3, 1), -0.5)), ('swap', torch.zeros((1, 3, 1))),
                     ('swap', torch.ones((1, 3, 1), dtype=torch.float64))):
        u = dict(ok)
        u[key] = bad
        with pytest.raises(ValueError, match=key):
            s.temper_samples(betas, rounds=1, pairs=p, uniforms=u)
    with pytest.raises(ValueError, match='cluster'):                     # cluster_beta_min = 0.7: one temperature makes cluster moves
        s.temper_samples(betas, rounds=1, pairs=p, uniforms=ok, cluster_beta_min=0.7)
    assert np.array_equal(s.states, kept) and not hasattr(s, 'temper_index') and not hasattr(s, 'temper_betas')
    r = rmf()
    r.states = np.zeros((4, 9), dtype=r.indtype)
    with pytest.raises(ValueError, match='Ising'):
        r.temper_samples(betas)
    with pytest.raises(ValueError, match='Ising'):
        tp.bit_tables(r)
    s.states = np.full((6, 16), 256)
    with pytest.raises(ValueError, match='states'):
        s.temper_samples(betas)
    t = ising3x3()                                                       # T = 1 and no round are valid arguments
    t.states = np.zeros((2, 9), dtype=t.indtype)
    assert tp.check_arguments(t, [1.0], 0, 0, True, None, None, None, 0, None)['shapes']['swap'] == (0, 2, 0)


def test_check_arguments_returns_the_plan():
    s = droplet()
    s.states = np.random.default_rng(4).integers(0, 256, (12, 16)).astype(s.indtype)
    np.random.seed(8)
    a = tp.check_arguments(s, (0.5, 1.0, 2.0), 3, 2, True, 1.0, None, None, 1, 2)
    np.random.seed(8)
    from tnac4o_amd import exchange as ex
    assert np.array_equal(a['pairs'], ex.check_pairs(None, 3, 4)) and a['pairs'].shape == (3, 2, 2)
    assert (a['T'], a['R'], a['M'], a['cluster_from'], a['keep'], a['rounds_per_call']) == (3, 4, 12, 1, 1, 2)
    assert a['shapes'] == {'sweep': (3, 2, 16, 12), 'cluster': (3, 2, 2), 'swap': (3, 4, 2)} and a['uniforms'] is None
    assert tp.check_arguments(s, (0.5, 1.0, 2.0), 3, 2, True, 2.5, None, None, None, None)['cluster_from'] == 3
    b = tp.check_arguments(s, (0.5, 1.0, 2.0), 3, 2, False, None, None, None, None, None)
    assert b['cluster_from'] == 3 and b['pairs'].shape == (3, 0, 2) and b['shapes']['cluster'] == (3, 0, 0)
    r = rmf()
    r.states = np.zeros((4, 9), dtype=r.indtype)
    assert tp.check_arguments(r, [0.5, 1.0], 1, 1, False, None, None, None, None, None)['R'] == 2


# ---------------------------------------------------------------------------------------------- argument errors of the export
def test_temper_argument_errors():
    """rc = -1 / -3 with a message that starts with tn_temper and names the limit, nothing launched: the device pointers below are not
    device memory, they are never followed.  tn_temper_ws_bytes returns 0 on the shapes the call refuses."""
    from tnac4o_amd import _lib
    from tnac4o_amd.beam import _Cell
    L = _lib.lib()
    p = 4096                                                             # stands for a non-null device pointer
    Nx = Ny = 2
    cells = (_Cell * 4)()
    for k in range(4):
        cells[k].q, cells[k].Es, cells[k].E1, cells[k].E4, cells[k].e1cols, cells[k].e4cols = 4, p, p, p, 4, 4
    M, T = 12, 3
    good = (ct.c_double * 3)(0.5, 1.0, 2.0)

    def call(Nx=Nx, Ny=Ny, cells=cells, M=M, T=T, betas=good, states=p, tidx=p, slot=p, round0=0, rounds=2, sweeps=1, usweep=p, ldu=M, nbits=10,
             nbmax=2, cellbits=p, bitcell=p, rowptr=p, cols=p, nnz=5, cluster_from=1, cpairs=p, Pc=2, ucl=p, uswap=p, E=p, acc=p, att=p, ws=p,
             wsb=None):
        if wsb is None:
            wsb = max(int(L.tn_temper_ws_bytes(Nx, Ny, M, T, nbits, Pc)), 1)
        return L.tn_temper(Nx, Ny, ct.cast(cells, ct.c_void_p) if cells is not None else None, M, T,
                           ct.cast(betas, ct.c_void_p) if betas is not None else None, states, tidx, slot, round0, rounds, sweeps, usweep, ldu, nbits,
                           nbmax, cellbits, bitcell, rowptr, cols, nnz, cluster_from, cpairs, Pc, ucl, uswap, E, acc, att, None, None, None, None, ws,
                           wsb, None)

    def arr(*v):
        return (ct.c_double * len(v))(*v)

    bad_cells = (_Cell * 4)()
    for k in range(4):
        bad_cells[k].q, bad_cells[k].Es, bad_cells[k].E1, bad_cells[k].E4, bad_cells[k].e1cols, bad_cells[k].e4cols = 4, p, p, p, 4, 4
    bad_cells[2].q = 40000
    for kw, word in ((dict(Nx=0), 'Nx'), (dict(cells=None), 'cells'), (dict(M=0), 'M'), (dict(M=2 ** 31), 'M'), (dict(T=0), 'T'), (dict(M=13), 'multiple'),
                     (dict(betas=None), 'betas'), (dict(betas=arr(0.5, 0.5, 2.0)), 'increasing'), (dict(betas=arr(1.0, 0.5, 2.0)), 'increasing'),
                     (dict(betas=arr(0.0, 0.5, 2.0)), 'positive'), (dict(betas=arr(0.5, 1.0, float('inf'))), 'finite'),
                     (dict(betas=arr(0.5, float('nan'), 2.0)), 'finite'), (dict(round0=-1), 'round0'), (dict(rounds=-1), 'rounds'),
                     (dict(sweeps=-1), 'sweeps'), (dict(states=None), 'states'), (dict(tidx=None), 'tidx'), (dict(slot=None), 'slot'),
                     (dict(E=None), 'energy_out'), (dict(acc=None), 'swap_accepted'), (dict(att=None), 'swap_attempted'), (dict(uswap=None), 'uswap'),
                     (dict(usweep=None), 'usweep'), (dict(ldu=M - 1), 'ldu'), (dict(nbits=-1), '65534'), (dict(nbits=65535), '65534'),
                     (dict(nbmax=0), 'nbmax'), (dict(nbmax=16), 'nbmax'), (dict(cellbits=None), 'cellbits'), (dict(bitcell=None), 'bitcell'),
                     (dict(rowptr=None), 'rowptr'), (dict(cols=None), 'cols'), (dict(nnz=-1), 'nnz'), (dict(nnz=2 ** 31), '2^31'),
                     (dict(cluster_from=-1), 'cluster_from'), (dict(cluster_from=4), 'cluster_from'), (dict(Pc=-1), 'Pc'), (dict(Pc=3), 'Pc'),
                     (dict(nbits=0, Pc=3), 'Pc'), (dict(cpairs=None), 'cpairs'), (dict(ucl=None), 'ucl'), (dict(cells=bad_cells), '32767'),
                     (dict(ws=None), 'ws')):
        assert call(**kw) == -1, kw
        msg = last_error(L)
        assert msg.startswith('tn_temper') and word in msg, (kw, msg)
    need = int(L.tn_temper_ws_bytes(Nx, Ny, M, T, 10, 2))
    assert need > 0 and call(wsb=need - 1) == -3
    msg = last_error(L)
    assert msg.startswith('tn_temper') and 'workspace' in msg and str(need) in msg
    assert int(L.tn_temper_ws_bytes(Nx, Ny, M, T, 0, 0)) < need
    for shape in ((0, 2, 12, 3, 10, 2), (2, 2, 0, 3, 10, 2), (2, 2, 2 ** 31, 1, 0, 0), (2, 2, 12, 0, 10, 2), (2, 2, 13, 3, 10, 2), (2, 2, 12, 3, -1, 2),
                  (2, 2, 12, 3, 65535, 2), (2, 2, 12, 3, 10, -1), (2, 2, 12, 3, 10, 3), (2 ** 20, 2 ** 20, 12, 3, 10, 2), (2 ** 15, 2 ** 15, 2 ** 30, 1, 0, 0)):
        assert int(L.tn_temper_ws_bytes(*shape)) == 0, shape
