"""tnac4o.calculate_correlation_function on the GPU: the three library entry points behind it at the smallest shapes that can go
wrong (tn_mpo_from_factor_ops, tn_env3_stack, tn_stack_cell_law and their workspace contracts), exact two-point functions on small
instances (enumeration / transfer matrices) under rotations and gauges, the invariants of one three-layer network at truncating bond
dimensions, parity with the numpy restatement, the management of the stack, and what the call leaves alone."""
import ctypes as ct
import functools
import importlib

import numpy as np
import pytest

import correlation_function_ref as cfr
import golden_inputs as gi
import marginals_ref as mr
import test_gpu_workspace as tw
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

F64 = torch.float64
dev, host = tw.dev, tw.host


@pytest.fixture(scope='module')
def L():
    from tnac4o_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def ops():
    from tnac4o_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------------------------ kernels
# Dt, pd, Dt2, bl, br, pu, Db, Db2, q: all different, multiples of nothing (pu < br: the middle product walks u), and a cell with the
# chimera tile bl = pu = 16, q = 256 (br = pu: it walks r)
SMALL = (3, 2, 5, 2, 4, 3, 3, 2, 6)
TILE = (3, 16, 5, 16, 16, 16, 4, 2, 256)
STACKS = [(SMALL, nE, nop) for nE in (1, 3, 7) for nop in (0, 1, 4)] + [(TILE, 3, 2)]


def _operands(dims, nE, nop, seed=0):
    Dt, pd, Dt2, bl, br, pu, Db, Db2, q = dims
    rng = np.random.default_rng(1000 * nE + 10 * nop + q + seed)
    F = rng.random((q, bl, pu)) + 0.1
    if q == pd * br:
        dmap, rmap = np.arange(q) % pd, np.arange(q) // pd
    else:
        dmap, rmap = rng.integers(0, pd, q), rng.integers(0, br, q)
    O = rng.standard_normal((nop, q))
    E = rng.standard_normal((nE, bl, Dt, Db))
    At, Ab = rng.standard_normal((Dt, pd, Dt2)), rng.standard_normal((Db, pu, Db2))
    return F, dmap, rmap, O, E, At, Ab


@pytest.mark.parametrize('dims,nop', [(SMALL, 0), (SMALL, 1), (SMALL, 4), (TILE, 2)])
def test_mpo_from_factor_ops(ops, dims, nop):
    Dt, pd, Dt2, bl, br, pu, Db, Db2, q = dims
    F, dmap, rmap, O, _, _, _ = _operands(dims, 1, nop)
    Fd, dm, rm = dev(F), dev(dmap, torch.int32), dev(rmap, torch.int32)
    Wops = ops.mpo_from_factor_ops(Fd, dm, rm, pd, br, dev(O) if nop else None)
    assert tuple(Wops.shape) == (1 + nop, bl, pd, br, pu)
    assert same_bits(host(Wops[0]), host(ops.mpo_from_factor(Fd, dm, rm, pd, br)))
    ref = cfr.ops_site_np(F, dmap, rmap, pd, br, O)
    assert float(np.max(np.abs(host(Wops) - ref))) <= 1e-14 * max(1.0, float(np.max(np.abs(ref))))


@pytest.mark.parametrize('dims,nE,nop', STACKS)
def test_env3_stack_against_env3_slot_by_slot(ops, dims, nE, nop):
    """Every output slot, its normalisation undone, against tn_env3 run on that slot alone with its own W; the first products too."""
    Dt, pd, Dt2, bl, br, pu, Db, Db2, q = dims
    F, dmap, rmap, O, E, At, Ab = _operands(dims, nE, nop)
    Wops = ops.mpo_from_factor_ops(dev(F), dev(dmap, torch.int32), dev(rmap, torch.int32), pd, br, dev(O) if nop else None)
    Ed, Atd, Abd, lg0 = dev(E), dev(At), dev(Ab), dev(np.array([3.0]))
    out, lg, half = ops.env3_stack(Ed, Atd, Wops, Abd, lg0, keep_half=True)
    out2, lg2 = ops.env3_stack(Ed, Atd, Wops, Abd, lg0)
    assert same_bits(host(out), host(out2)) and same_bits(host(lg), host(lg2))
    assert tuple(out.shape) == (nE + nop, br, Dt2, Db2) and tuple(half.shape) == (nE, bl, pd, Dt2, Db)
    o, scale = host(out), 2.0 ** (float(host(lg)[0]) - 3.0)
    assert 1.0 <= float(np.max(np.abs(o[0]))) < 2.0                 # slot 0 carries the normalisation
    for e in range(nE + nop):
        src, W = (e, Wops[0]) if e < nE else (0, Wops[1 + e - nE])
        r, rl, rh = ops.env3(0, Ed[src].contiguous(), Atd, W.contiguous(), Abd, keep_half=True)
        ref = host(r) * 2.0 ** float(host(rl)[0])
        assert float(np.max(np.abs(o[e] * scale - ref))) <= 1e-13 * float(np.linalg.norm(ref)), e
        if e < nE:
            assert float(np.max(np.abs(host(half[e]) - host(rh)))) <= 1e-13 * float(np.linalg.norm(host(rh))), e


@pytest.mark.parametrize('dims,nE', [(SMALL, 1), (SMALL, 3), (SMALL, 7), (TILE, 3)])
def test_stack_cell_law_against_einsum(ops, dims, nE):
    Dt, pd, Dt2, bl, br, pu, Db, Db2, q = dims
    F, dmap, rmap, _, _, _, _ = _operands(dims, nE, 0)
    rng = np.random.default_rng(q + nE)
    HL, HR = rng.standard_normal((nE, bl, pd, Dt2, Db)), rng.standard_normal((pu, br, Dt2, Db))
    dmap[0] = pd                                  # out of range: contributes 0
    D = host(ops.stack_cell_law(dev(HL), dev(HR), dev(F), dev(dmap, torch.int32), dev(rmap, torch.int32)))
    X = np.einsum('eldxb,urxb->eldur', HL, HR)
    ref = np.einsum('slu,elsu->es', F[1:], X[:, :, dmap[1:], :, rmap[1:]].transpose(1, 2, 0, 3))
    assert D.shape == (nE, q) and np.all(D[:, 0] == 0)
    assert float(np.max(np.abs(D[:, 1:] - ref))) <= 1e-13 * float(np.max(np.abs(ref)))


def _one_byte_short(L, call, wsb, outs):
    ws = Guarded(wsb - 1, 0x00)
    bufs = {k: Guarded.of(dt, sh, 0xFF) for k, (dt, sh) in outs.items()}
    rc, _ = call(bufs, ws.ptr, wsb - 1)
    torch.cuda.synchronize()
    assert rc < 0 and 'too small' in tw._msg(L), (rc, tw._msg(L))
    assert ws.intact() and all(b.intact() and b.untouched(0xFF) for b in bufs.values())


@pytest.mark.parametrize('dims,nE,nop', [(SMALL, 1, 0), (SMALL, 3, 4), (SMALL, 7, 1), (TILE, 3, 2), ((33, 4, 31, 4, 4, 4, 17, 65, 16), 5, 3)])
@pytest.mark.parametrize('half', (False, True))
def test_env3_stack_workspace(L, ops, dims, nE, nop, half):
    Dt, pd, Dt2, bl, br, pu, Db, Db2, q = dims
    F, dmap, rmap, O, E, At, Ab = _operands(dims, nE, nop, seed=1)
    Wops = ops.mpo_from_factor_ops(dev(F), dev(dmap, torch.int32), dev(rmap, torch.int32), pd, br, dev(O) if nop else None)
    Ed, Atd, Abd = dev(E), dev(At), dev(Ab)
    wsb = int(L.tn_env3_stack_ws_bytes(nE, nop, *dims[:8], 0 if half else 1))
    outs = {'out': (F64, (nE + nop, br, Dt2, Db2)), 'lg': (F64, (1,))}
    if half:
        outs['half'] = (F64, (nE, bl, pd, Dt2, Db))

    def call(b, ws, wsb_):
        return L.tn_env3_stack(Ed.data_ptr(), Atd.data_ptr(), Wops.data_ptr(), Abd.data_ptr(), nE, nop, *dims[:8], None, b['out'].ptr,
                               b['lg'].ptr, b['half'].ptr if half else None, ws, wsb_, tw._st()), None
    res, _ = tw.contract(L, ops, wsb, outs, call)
    _one_byte_short(L, call, wsb, outs)
    ref = ops.env3_stack(Ed, Atd, Wops, Abd, keep_half=half)
    assert same_bits(res['out'], host(ref[0])) and same_bits(res['lg'], host(ref[1]))
    if half:
        assert same_bits(res['half'], host(ref[2]))


@pytest.mark.parametrize('dims,nE', [(SMALL, 1), (SMALL, 7), (TILE, 3), ((3, 8, 33, 8, 8, 8, 31, 2, 8), 5)])
def test_stack_cell_law_workspace(L, ops, dims, nE):
    Dt, pd, Dt2, bl, br, pu, Db, Db2, q = dims
    F, dmap, rmap, _, _, _, _ = _operands(dims, nE, 0, seed=2)
    rng = np.random.default_rng(q + nE + 5)
    HL, HR = dev(rng.standard_normal((nE, bl, pd, Dt2, Db))), dev(rng.standard_normal((pu, br, Dt2, Db)))
    Fd, dm, rm = dev(F), dev(dmap, torch.int32), dev(rmap, torch.int32)
    K = Dt2 * Db
    wsb = int(L.tn_stack_cell_law_ws_bytes(nE, bl, pd, br, pu, K))
    outs = {'D': (F64, (nE, q))}

    def call(b, ws, wsb_):
        return L.tn_stack_cell_law(HL.data_ptr(), HR.data_ptr(), Fd.data_ptr(), dm.data_ptr(), rm.data_ptr(), q, nE, bl, pd, br, pu, K,
                                   b['D'].ptr, ws, wsb_, tw._st()), None
    res, _ = tw.contract(L, ops, wsb, outs, call)
    _one_byte_short(L, call, wsb, outs)
    assert same_bits(res['D'], host(ops.stack_cell_law(HL, HR, Fd, dm, rm)))


def test_argument_checks(L):
    z = ct.c_void_p(0)
    assert L.tn_env3_stack(z, z, z, z, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, None, z, z, None, z, 0, None) == -1 and 'null' in tw._msg(L)
    one = torch.ones(8, dtype=F64, device='cuda')
    p = one.data_ptr()
    assert L.tn_env3_stack(p, p, p, p, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, None, p, p, None, p, 1 << 20, None) == -1 and 'slot' in tw._msg(L)
    assert L.tn_env3_stack(p, p, p, p, 1, -1, 1, 1, 1, 1, 1, 1, 1, 1, None, p, p, None, p, 1 << 20, None) == -1
    assert L.tn_env3_stack(p, p, p, p, 1, 0, 1, 0, 1, 1, 1, 1, 1, 1, None, p, p, None, p, 1 << 20, None) == -1 and 'dimension' in tw._msg(L)
    assert L.tn_stack_cell_law(p, p, p, p, p, 1, 0, 1, 1, 1, 1, 1, p, p, 1 << 20, None) == -1 and 'dimension' in tw._msg(L)
    assert L.tn_mpo_from_factor_ops(p, p, p, None, 1, 1, 1, 1, 1, 1, p, None) == -1 and 'operator' in tw._msg(L)
    assert L.tn_env3_stack_ws_bytes(0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1) == 0 and L.tn_stack_cell_law_ws_bytes(1, 1, 0, 1, 1, 1) == 0


# ------------------------------------------------------------------------------------------------------------------ exactness
BETAS = (0.5, 1.0, 3.0)
CASES = ('ising3x3', 'rmf3x3', 'chimera2x2', 'rmf4x4')


def _model(case):
    from tnac4o_amd import auxx
    if case == 'ising3x3':
        return mr.ising_3x3_nc2()
    if case == 'rmf3x3':
        return auxx.synthetic_rmf(3, 3, 3, 17)
    if case == 'chimera2x2':
        return auxx.synthetic_chimera(2, 2, 29)
    return auxx.synthetic_rmf(4, 4, 2, 31)           # 65 536 configurations; distance 3 takes two propagation steps


def _make(case, beta):
    import tnac4o_amd
    J = _model(case)
    if case == 'ising3x3':
        return tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=J, beta=beta)
    if case == 'chimera2x2':
        return tnac4o_amd.tnac4o(mode='Ising', Nx=2, Ny=2, Nc=8, J=J, beta=beta)
    return tnac4o_amd.tnac4o(mode='RMF', Nx=J['Nx'], Ny=J['Ny'], J=J, beta=beta)


@functools.lru_cache(maxsize=None)
def _exact(case, beta):
    """Ising: (line_pairs, line_distance, C, m); RMF: the dictionary of joints.  Computed once per (case, beta) and left unchanged."""
    J = _model(case)
    if case == 'ising3x3':
        return cfr.exact_line_ising(J, 3, 3, 2, beta)
    if case == 'chimera2x2':
        return cfr.exact_line_chimera_2x2(J, beta)
    return cfr.exact_line_rmf(J, beta)


def _check_exact(ins, case, beta, tol=1e-10):
    ex = _exact(case, beta)
    if ins.mode == 'Ising':
        pairs, dist, C, m = ex
        assert ins.line_pairs.dtype == np.int64 and np.array_equal(ins.line_pairs, pairs)
        assert np.array_equal(ins.line_distance, dist)
        assert float(np.max(np.abs(ins.line_correlations - C))) <= tol
        assert float(np.max(np.abs(ins.line_magnetization - m))) <= tol
        assert ins.line_pair_marginals is None
    else:
        out = ins.line_pair_marginals
        assert sorted(out) == sorted(ex)
        for key, P in ex.items():
            assert out[key].shape == P.shape and float(np.max(np.abs(out[key] - P))) <= tol, key
        assert ins.line_correlations is None
    assert -1e-12 < ins.line_negative <= 0
    _row_constant(ins.line_row_log2)


def _row_constant(log2z, tol=1e-10):
    for ny in range(log2z.shape[0]):
        row = log2z[ny]
        assert np.all(np.isfinite(row)), row
        assert np.max(np.abs(row - row[0])) <= tol * max(abs(row[0]), 1.0), (ny, row)


@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('case', CASES)
def test_exact_on_small_instances(case, beta):
    ins = _make(case, beta)
    out = ins.calculate_correlation_function(Dmax=64)
    assert out is (ins.line_correlations if ins.mode == 'Ising' else ins.line_pair_marginals)
    _check_exact(ins, case, beta)


@pytest.mark.parametrize('rot', [1, 2, 3])
@pytest.mark.parametrize('case', CASES)
def test_exact_under_rotations(case, rot):
    ins = _make(case, 3.0)
    ins.rotate_graph(rot)
    ins.calculate_correlation_function(Dmax=64)
    _check_exact(ins, case, 3.0)


@pytest.mark.parametrize('case', CASES)
def test_exact_after_precondition(case):
    ins = _make(case, 1.0)
    ins.precondition()
    ins.calculate_correlation_function(Dmax=64)
    _check_exact(ins, case, 1.0)


def test_rows_and_columns_make_both():
    a, b, c = (_make('ising3x3', 1.0) for _ in range(3))
    a.calculate_correlation_function(Dmax=64, lines='rows')
    b.calculate_correlation_function(Dmax=64, lines='columns')
    c.calculate_correlation_function(Dmax=64, lines='both')
    got = {tuple(p): v for x in (a, b) for p, v in zip(x.line_pairs.tolist(), x.line_correlations)}
    assert len(got) == len(a.line_pairs) + len(b.line_pairs) == len(c.line_pairs)
    assert all(i // 2 // 3 == j // 2 // 3 for i, j in a.line_pairs) and all(i // 2 % 3 == j // 2 % 3 for i, j in b.line_pairs)
    assert float(np.max(np.abs(np.array([got[tuple(p)] for p in c.line_pairs.tolist()]) - c.line_correlations))) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ one network
@functools.lru_cache(maxsize=None)
def _network(L_, chi):
    """A droplet instance with its boundaries at chi and the results of one pass over them (shared; nobody changes them)."""
    import tnac4o_amd
    n = {128: 4, 512: 8}[L_]
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=n, Ny=n, Nc=8, J=gi.droplet_J(L_, 1), beta=3.0)
    ins._setup_rhoT(Dmax=chi)
    ins._setup_rhoB(Dmax=chi)
    return ins, ins._line_pass()


NETWORKS = [(128, 8), (512, 16)]


@pytest.mark.parametrize('L_,chi', NETWORKS)
def test_inserted_operator_does_not_depend_on_where_it_is_closed(L_, chi):
    """<O_a(k)> from the slot of (k, a) closed with the identity at any k' equals the value from the plain slot's law at k; the raw
    total is the same at every cell of a row."""
    ins, (laws, joints, log2z) = _network(L_, chi)
    Nx = ins.Nx
    assert len(joints) == Nx * Nx * (Nx - 1) // 2
    for (c1, c2), M in joints.items():
        m = ins._line_operators(*divmod(c1, Nx)) @ laws[c1]
        assert float(np.max(np.abs(M.sum(1) - m))) <= 1e-10, (c1, c2)
    for p in laws:
        assert abs(p.sum() - 1) <= 1e-12
    _row_constant(log2z)


@pytest.mark.parametrize('L_,chi', NETWORKS)
def test_distance_one_is_the_bond_table_of_the_same_network(L_, chi):
    from tnac4o_amd.tnac4o import _spins
    ins, (laws, joints, log2z) = _network(L_, chi)
    Pl, Pu, _, clog2z = ins._correlation_pass()
    Nx = ins.Nx
    compared = 0
    for ny in range(ins.Ny):
        for nx in range(1, Nx):
            c = ny * Nx + nx
            bond = np.asarray(ins.ir[ny][nx - 1])
            if not bond.size:
                continue
            S = _spins(ins.sN[ny][nx])
            Cb = _spins(bond.size).T @ Pl[c].T @ S                          # [bond spin of the left cell, spin of this cell]
            Cl = joints[(c - 1, c)] @ ins._line_operators(ny, nx).T
            assert float(np.max(np.abs(Cl[bond] - Cb))) <= 1e-11, c
            assert float(np.max(np.abs(laws[c] - Pl[c].sum(1)))) <= 1e-11, c
            compared += 1
    assert compared >= ins.Ny * (Nx - 1) // 2
    assert float(np.max(np.abs(log2z - clog2z))) <= 1e-10 * float(np.max(np.abs(clog2z)))


@pytest.mark.parametrize('L_,chi', NETWORKS)
def test_pass_equals_numpy_restatement(L_, chi):
    ins, (laws, joints, log2z) = _network(L_, chi)
    rlaws, rjoints, rlog2z = cfr.line_pass_np(ins)
    assert sorted(joints) == sorted(rjoints)
    for key, M in rjoints.items():
        assert joints[key].shape == M.shape and float(np.max(np.abs(joints[key] - M))) <= 1e-11, key
    for c, p in enumerate(rlaws):
        assert float(np.max(np.abs(laws[c] - p))) <= 1e-11, c
    assert float(np.max(np.abs(log2z - rlog2z))) <= 1e-9 * max(1.0, float(np.max(np.abs(rlog2z))))


# ------------------------------------------------------------------------------------------------------------------ stack management
def test_max_distance_is_a_subset_of_the_uncapped_result():
    ins, (laws, joints, log2z) = _network(128, 8)
    claws, cjoints, clog2z = ins._line_pass(max_distance=2)
    want = {key: M for key, M in joints.items() if key[1] - key[0] <= 2}
    assert sorted(cjoints) == sorted(want) and 0 < len(want) < len(joints)
    for key, M in want.items():
        assert float(np.max(np.abs(cjoints[key] - M))) <= 1e-12, key
    assert all(float(np.max(np.abs(a - b))) <= 1e-12 for a, b in zip(claws, laws))
    rl, rj, _ = cfr.line_pass_np(ins, max_distance=2)
    assert sorted(rj) == sorted(cjoints)


def test_slot_budget_splits_the_start_cells_without_changing_the_result(monkeypatch):
    mod = importlib.import_module('tnac4o_amd.tnac4o')              # (the package re-exports the class under this name)
    ins, (laws, joints, log2z) = _network(128, 8)
    seen = []
    plan = mod._plan_line_groups

    def spy(nops, reach, cap):
        seen.append(plan(nops, reach, cap))
        return seen[-1]
    monkeypatch.setattr(mod, '_plan_line_groups', spy)
    budget = 9 * max(ins._line_slot_bytes(ny) for ny in range(ins.Ny))          # the plain slot and one cell's 8 operators
    blaws, bjoints, blog2z = ins._line_pass(slot_budget=budget)
    assert max(len(g) for g in seen) >= 3, seen
    assert sorted(bjoints) == sorted(joints)
    for key, M in joints.items():
        assert float(np.max(np.abs(bjoints[key] - M))) <= 1e-12, key
    assert all(float(np.max(np.abs(a - b))) <= 1e-12 for a, b in zip(blaws, laws))
    assert float(np.max(np.abs(blog2z - log2z))) <= 1e-12 * float(np.max(np.abs(log2z)))
    with pytest.raises(MemoryError):
        ins._line_pass(slot_budget=budget // 2)


def test_two_identical_calls_are_bit_equal():
    ins, (laws, joints, log2z) = _network(128, 8)
    laws2, joints2, log2z2 = ins._line_pass()
    assert same_bits(log2z, log2z2) and all(same_bits(a, b) for a, b in zip(laws, laws2))
    assert sorted(joints) == sorted(joints2) and all(same_bits(joints[k], joints2[k]) for k in joints)
    a, b = _make('rmf3x3', 1.0), _make('rmf3x3', 1.0)
    pa, pb = a.calculate_correlation_function(Dmax=64), b.calculate_correlation_function(Dmax=64)
    assert all(same_bits(pa[k], pb[k]) for k in pa)


# ------------------------------------------------------------------------------------------------------------------ frame hygiene
@pytest.mark.parametrize('lines', ['rows', 'columns', 'both'])
def test_leaves_frame_gauges_search_results_and_thermal_outputs_alone(lines):
    ins = _make('ising3x3', 3.0)
    ins.rotate_graph(1)
    ins.precondition()
    assert any(not np.all(getattr(ins, k) == 1) for k in ('Xu', 'Xd', 'Xl', 'Xr'))     # the gauges are not trivial here
    ins.search_ground_state(M=64, Dmax=64)
    ins.calculate_marginals(Dmax=64)
    ins.calculate_correlations(Dmax=64)
    keep = {k: np.copy(getattr(ins, k)) for k in ('energy', 'states', 'probability', 'degeneracy', 'Xu', 'Xd', 'Xl', 'Xr', 'order', 'order_i',
                                                  'magnetization', 'marginal_row_log2', 'correlations', 'bond_pairs',
                                                  'correlation_row_log2', 'J', 'overlaps_ud')}
    marg = [np.copy(p) for p in ins.marginals]
    scal = (ins.rotation, ins.marginals_negative, ins.correlations_negative, ins.energy_mean, ins.Nx, ins.Ny)
    rhoT, rhoB = ins.rhoT, ins.rhoB
    ins.calculate_correlation_function(Dmax=64, lines=lines)
    for k, v in keep.items():
        assert np.array_equal(getattr(ins, k), v), k
    assert scal == (ins.rotation, ins.marginals_negative, ins.correlations_negative, ins.energy_mean, ins.Nx, ins.Ny)
    assert all(np.array_equal(p, q) for p, q in zip(ins.marginals, marg))
    assert ins.rhoT is rhoT and ins.rhoB is rhoB
    pairs, dist, C, m = _exact('ising3x3', 3.0)
    cells = pairs // 2                                                    # model cells; the frame is turned once, so its rows are
    same_row, same_col = cells[:, 0] // 3 == cells[:, 1] // 3, cells[:, 0] % 3 == cells[:, 1] % 3        # the model's columns
    want = {'rows': same_col, 'columns': same_row, 'both': same_row | same_col}[lines]
    assert np.array_equal(ins.line_pairs, pairs[want]) and np.array_equal(ins.line_distance, dist[want])
    assert float(np.max(np.abs(ins.line_correlations - C[want]))) <= 1e-10
    assert float(np.max(np.abs(ins.line_magnetization - m))) <= 1e-10
