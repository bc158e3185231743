"""tnac4o.calculate_log_probability on the GPU: the scoring kernel against the table tn_calc_pn writes, the bits of the draw for
configurations sample_boltzmann drew, the oracle's forced walk on configurations it did not draw, exact log2 p(x) of every
configuration of a small lattice, normalisation of q under truncation, rotations, and the contract of the call and of tn_gibbs_score."""
import ctypes as ct
import itertools

import numpy as np
import pytest

import golden_inputs as gi
import sampling_ref as sref
from guarded import Guarded, same_bits
from oracle import solver_ref as sr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_sampling import G8, SWEEP, _kernel_inputs, droplet, dv, load, small      # noqa: E402  (helpers only, no test is imported)

LN2 = float(np.log(2.0))


# ---------------------------------------------------------------------------------------------- 1. kernel against tn_calc_pn
@pytest.mark.parametrize('q', [1, 3, 257, 5000])
def test_score_pn_against_calc_pn(q):
    """Groups of 1, 3 and 300 members among n + 7 samples: the increment has the bits of tn_calc_pn's log2p_out[g, s] with parent 0, minP
    its bits; a pre-filled log2p is added to; the 7 samples of no group are untouched; P[s] = 0, s = q and s = -1 give -inf (the last two
    with child = 0); no NaN anywhere."""
    from tnac4o_amd import ops
    rng = np.random.default_rng(300 + q)
    T1, RR, F, dmap, rmap = _kernel_inputs(q, rng)
    sizes = [1, 3, 300]
    rows = np.array([[1, 0, 0, 0],                       # an all-zero table: comes back uniform
                     [0, 1, 2, 2],                       # a table under the negative rule
                     [2, 1, 1, 1]], dtype=np.int32)      # (l, u) = (1, 1): P[0] = 0 when q > 1
    n, spare, ld, pos = sum(sizes), 7, 5, 2
    perm = rng.permutation(n + spare)[:n].astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    forced = rng.integers(-3, 40, (n + spare, ld)).astype(np.int16)      # the other columns: anything, they are never read
    group = np.full(n + spare, -1)
    for g in range(3):
        group[perm[starts[g]:starts[g + 1]]] = g
    mem = perm[starts[2]:starts[3]]
    forced[:, pos] = rng.integers(0, q, n + spare)
    forced[mem[:4], pos] = (0, q, -1, q - 1)             # P[0] = 0, two states outside [0, q), the last state
    forced[mem[4:40], pos] = np.arange(36) % q           # the low states, whatever q
    base = rng.normal(0.0, 5.0, n + spare)
    args = [dv(T1), dv(RR), dv(F), dv(dmap), dv(rmap)] + [dv(rows[:, j].copy()) for j in range(4)]
    P, mP, LP = ops.calc_pn(*args, parent_log2p=torch.zeros(3, dtype=torch.float64, device='cuda'))
    child, log2p, mP2, cl = ops.score_pn(*args, dv(perm), dv(starts), dv(forced), pos, log2p=dv(base), cells=True)
    torch.cuda.synchronize()
    P, mP, LP, child, log2p, mP2, cl = (t.cpu().numpy() for t in (P, mP, LP, child, log2p, mP2, cl))
    assert same_bits(mP2, mP)
    assert mP[0] == -1.0 and np.all(P[0] == 1.0 / q)
    if q > 1:
        assert P[2, 0] == 0.0 and P[2, q - 1] > 0
    s = forced[:, pos].astype(np.int64)
    inside = (s >= 0) & (s < q)
    want_inc = np.zeros(n + spare)
    want_child = np.zeros(n + spare, dtype=np.int32)
    for k in range(n + spare):
        if group[k] < 0:
            continue
        want_inc[k] = LP[group[k], s[k]] if inside[k] else -np.inf
        want_child[k] = s[k] if inside[k] else 0
    scored = group >= 0
    assert np.array_equal(child, want_child)
    assert same_bits(cl[scored, pos], want_inc[scored])
    assert same_bits(log2p[scored], (base + want_inc)[scored])
    assert same_bits(log2p[~scored], base[~scored]) and np.all(cl[~scored] == 0.0)
    assert np.all(np.delete(cl, pos, axis=1) == 0.0)                     # one column is written
    assert not np.isnan(log2p).any() and not np.isnan(cl).any()
    assert cl[mem[1], pos] == -np.inf and cl[mem[2], pos] == -np.inf and child[mem[1]] == 0 and child[mem[2]] == 0
    if q > 1:
        assert cl[mem[0], pos] == -np.inf and child[mem[0]] == 0 and np.isfinite(cl[mem[3], pos])
    print('q = %d: %d of %d scored samples at -inf' % (q, int(np.isinf(cl[scored, pos]).sum()), n))
    # -inf stays -inf under a later finite increment
    child, log2p2, _ = ops.score_pn(*args, dv(perm), dv(starts), dv(np.zeros_like(forced)), pos, log2p=dv(log2p))
    log2p2 = log2p2.cpu().numpy()
    gone = np.isinf(log2p)
    assert gone.any() and np.all(log2p2[gone] == -np.inf) and not np.isnan(log2p2).any()


# ---------------------------------------------------------------------------------------------- 2. the bits of the draw
def test_same_bits_as_the_draw():
    """Identical arithmetic, so no tolerance: a configuration sample_boltzmann drew comes back with the log2 q and the energy it was drawn
    with, whatever shares the call (a permutation, a subset with duplicates, chunks of 512, 64 and 7), on the kept boundaries and on
    boundaries built again with the same options."""
    M = 512
    u = np.random.default_rng(2024).random((16, M))
    s = droplet()
    s.sample_boltzmann(M=M, Dmax=8, uniforms=u)
    st, E, lq = np.copy(s.states), np.copy(s.energy), np.copy(s.probability)
    rng = np.random.default_rng(12)
    for idx, chunk in ((np.arange(M), None), (rng.permutation(M), None), (rng.integers(0, M, 100), None), (np.arange(M), 512),
                       (np.arange(M), 64), (np.arange(M), 7)):
        out = s.calculate_log_probability(np.ascontiguousarray(st[idx]), boundary='keep', chunk=chunk)
        assert out is s.scored_log2q
        assert same_bits(s.scored_log2q, lq[idx]) and same_bits(s.scored_energy, E[idx]), chunk
        assert s.scored_cell_log2q is None
    s.calculate_log_probability(st, cells=True, boundary='keep')
    assert same_bits(s.scored_log2q, lq) and s.scored_cell_log2q.shape == (M, 16)
    assert float(np.max(np.abs(s.scored_cell_log2q.sum(axis=1) - lq))) <= 1e-12 * float(np.max(np.abs(lq)))
    # nothing of the sampling result moved
    assert same_bits(s.states, st) and same_bits(s.energy, E) and same_bits(s.probability, lq)
    b = droplet()
    b.calculate_log_probability(st, boundary='build', Dmax=8)
    assert same_bits(b.scored_log2q, lq) and same_bits(b.scored_energy, E)
    assert b.scored_negative <= 0 and b.energy.size == 0 and b.states.shape[0] == 0


# ---------------------------------------------------------------------------------------------- 3. the oracle, on states that were not drawn
def undrawn(states):
    """Row k of the golden configurations with spin (k // 16 + k) mod 8 of cell k mod 16 flipped.  (Replacing that cell by
    (s + 1 + k) mod q leaves 10 of 64 / 8 of 32 rows whose oracle conditionals all reach 1e-9 -- an arbitrary state of a 256-state cell
    is too improbable at beta = 3; with one spin flipped the oracle alone keeps 40 of 64 / 20 of 32, and no row is among the drawn.)"""
    st = np.array(states, dtype=np.int64)
    for k in range(st.shape[0]):
        st[k, k % 16] ^= 1 << ((k // 16 + k) % 8)
    return st


@pytest.mark.parametrize('rot,chi,M,seed', G8)
def test_against_the_oracle_on_states_that_were_not_drawn(rot, chi, M, seed):
    g = load('g8_gibbs.npz')
    drawn = g['r%d_chi%d_M%d_seed%d_states' % (rot, chi, M, seed)].astype(np.int64)
    st = undrawn(drawn)
    assert not any(np.array_equal(a, b) for a in st for b in drawn)
    s = droplet(rot)
    lq = s.calculate_log_probability(st, cells=True, Dmax=chi)
    o = sr.RefSolver(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=3.0)
    if rot:
        o.rotate_graph(rot)
    olq, Pc = sref.oracle_log2q(o, sref.rotated_states(s, st), Dmax=chi, **SWEEP)
    keep = np.all(Pc >= 1e-9, axis=1)
    assert 2 * int(keep.sum()) >= M, int(keep.sum())
    diff, bound = np.abs(lq - olq)[keep], sref.log2q_bound(Pc)[keep]
    k = int(np.argmax(diff / bound))
    Pmodel = Pc[:, np.asarray(s.order)]                                  # the oracle's cells in model order, as scored_cell_log2q
    cdiff = np.abs(np.exp2(s.scored_cell_log2q) - Pmodel)[keep]
    print('rot %d chi %d: %d of %d rows kept, largest |log2 q - oracle| = %.3e (bound there %.3e), largest |P_cell - oracle| = %.3e'
          % (rot, chi, int(keep.sum()), M, diff.max(), bound[k], cdiff.max()))
    assert np.all(diff <= bound), (k, diff[k], bound[k])
    np.testing.assert_allclose(np.exp2(s.scored_cell_log2q)[keep], Pmodel[keep], rtol=1e-10, atol=1e-14)


# ---------------------------------------------------------------------------------------------- 4. / 5. every configuration of rmf3x3
_ALL = np.array(list(itertools.product(range(3), repeat=9)), dtype=np.int64)


@pytest.mark.parametrize('beta', [0.5, 3.0])
def test_exhaustive_exact(beta):
    """Untruncated, q is the Boltzmann distribution: log2 q(x) = -beta E(x) / ln 2 - log2 Z for all 3^9 configurations."""
    from tnac4o_amd import auxx
    ins = small('rmf3x3', beta)
    lq = ins.calculate_log_probability(_ALL, Dmax=64)
    E = auxx.energy_RMF(auxx.synthetic_rmf(3, 3, 3, 17), _ALL)
    dev = np.abs(lq + beta * E / LN2 + sref.exact_log2Z('rmf3x3', beta))
    print('beta %.1f: largest |log2 q - log2 p| = %.3e, largest energy deviation %.3e' % (beta, dev.max(), np.abs(ins.scored_energy - E).max()))
    assert lq.shape == (_ALL.shape[0],) and float(dev.max()) <= 1e-10
    assert float(np.max(np.abs(ins.scored_energy - E))) <= 1e-9
    assert -1e-14 < ins.scored_negative <= 0


def test_exhaustive_truncated():
    """Dmax = 2, beta = 3 (the oracle discards 2.4e-3 there, so no other beta was needed): every conditional table is normalised, so q
    sums to 1 whatever the truncation; 1e-12 is about 100 x the rounding of 9 normalisations and a log2 / exp2 round trip (the oracle's
    forced walk alone: 2.2e-16)."""
    from tnac4o_amd import auxx
    beta = 3.0
    ins = small('rmf3x3', beta)
    lq = ins.calculate_log_probability(_ALL, Dmax=2)
    assert max(float(d) for d in ins.rhoT_discarded) > 0
    total = float(np.sum(np.exp2(lq)))
    lp = -beta * auxx.energy_RMF(auxx.synthetic_rmf(3, 3, 3, 17), _ALL) / LN2 - sref.exact_log2Z('rmf3x3', beta)
    kl = float(np.sum(np.exp2(lq) * (lq - lp))) * LN2
    print('sum q - 1 = %.3e, KL(q || p) = %.6e nats, largest |log2 q - log2 p| = %.3e' % (total - 1.0, kl, np.abs(lq - lp).max()))
    assert abs(total - 1.0) <= 1e-12
    assert kl > 0 and float(np.abs(lq - lp).max()) > 1e-6                # the truncation is felt


# ---------------------------------------------------------------------------------------------- 6. rotations and frame
@pytest.mark.parametrize('rot', [0, 1, 2, 3])
@pytest.mark.parametrize('case', ['ising3x3', 'chimera2x2'])
def test_rotation_and_frame(case, rot):
    beta = 1.0
    exact = _exact(case, beta)
    ins = small(case, beta)
    qs = ins._cell_sizes()                                               # (before the rotation: model order)
    if rot:
        ins.rotate_graph(rot)
    st = np.random.default_rng(50 + rot).integers(0, qs[None, :], size=(64, qs.size))
    lq = ins.calculate_log_probability(st, Dmax=64)
    tmp = small(case, beta)
    tmp.states = st
    E = sref.model_energy(case, tmp)
    assert float(np.max(np.abs(lq + beta * E / LN2 + exact))) <= 1e-10
    assert float(np.max(np.abs(ins.scored_energy - E))) <= 1e-9
    assert ins.states.shape[0] == 0                                      # nothing was stored as a search result
    # states = None: the stored states of a search, in their own (narrow) dtype
    ins.search_ground_state(M=64, Dmax=64)
    kept = np.copy(ins.states)
    lq = ins.calculate_log_probability(Dmax=64)
    assert lq.shape == ins.energy.shape
    assert float(np.max(np.abs(lq + beta * sref.model_energy(case, ins) / LN2 + exact))) <= 1e-10
    assert float(np.max(np.abs(ins.scored_energy - ins.energy))) <= 1e-9
    assert same_bits(ins.states, kept)


_EXACT = {}


def _exact(case, beta):
    if (case, beta) not in _EXACT:
        _EXACT[(case, beta)] = sref.exact_log2Z(case, beta)
    return _EXACT[(case, beta)]


# ---------------------------------------------------------------------------------------------- 7. contract
def test_contract_of_the_call():
    ins = small('ising3x3', 3.0)
    ins.rotate_graph(1)
    ok = np.zeros((5, 9), dtype=np.int64)
    for bad in (ok[:, :8], ok[0], ok.astype(np.float32), ok.tolist()):
        with pytest.raises(ValueError):
            ins.calculate_log_probability(bad)
    b = ok.copy()
    b[3, 4] = 2                                                          # model cell 4 holds the inactive spin: two states
    with pytest.raises(ValueError, match=r'states\[3, 4\]'):
        ins.calculate_log_probability(b)
    with pytest.raises(ValueError, match='rhoT'):
        ins.calculate_log_probability(ok, boundary='keep')
    assert not hasattr(ins, 'rhoT') and not hasattr(ins, 'scored_log2q')
    # the results of a search and of the thermal calls are not touched
    ins.search_ground_state(M=64, Dmax=64)
    ins.calculate_marginals(Dmax=64)
    keep = {k: np.copy(getattr(ins, k)) for k in ('energy', 'states', 'probability', 'degeneracy', 'discarded_probability',
                                                  'negative_probability', 'Xu', 'Xd', 'Xl', 'Xr', 'order', 'magnetization', 'marginal_row_log2')}
    rot = ins.rotation
    st = np.random.default_rng(1).integers(0, 2, size=(33, 9))
    ins.calculate_log_probability(st, boundary='keep', cells=True)
    assert ins.scored_log2q.shape == (33,) and ins.scored_cell_log2q.shape == (33, 9) and np.all(ins.scored_log2q < 0)
    for k, v in keep.items():
        assert same_bits(np.asarray(getattr(ins, k)), v), k
    assert ins.rotation == rot


def test_gibbs_score_workspace_contract():
    """tn_gibbs_score with exactly tn_gibbs_score_ws_bytes: guards intact for NaN- and random-filled workspaces, every result entry written,
    results bit-equal between the fills and equal to the driver's; 8 bytes less are rejected with -3 before any launch."""
    from tnac4o_amd import _lib, ops
    from tnac4o_amd.beam import CellTable
    L = _lib.lib()
    s = droplet()
    s._setup_rhoT(Dmax=8, **SWEEP)
    table = CellTable(s)
    assert table.misfit is None
    M, ncell = 96, 16
    B = int(max(np.max(s.ld), np.max(s.lr), 2))
    need = int(L.tn_gibbs_score_ws_bytes(4, 4, M, table.qmax, table.max_env, table.max_t1, table.max_w))
    rot = np.random.default_rng(3).integers(0, 256, (M, ncell))
    rot[5, 7], rot[6, 0] = 256, -1                                       # outside [0, q): -inf, walked on as state 0
    d_st = dv(rot.astype(np.int16))
    out = {}
    for fill in (0xFF, 'random'):
        ws = Guarded(need, fill, seed=1)
        E = Guarded.of(torch.float64, (M,), 0xFF, seed=3)
        lq = Guarded.of(torch.float64, (M,), 0xFF, seed=4)
        cl = Guarded.of(torch.float64, (M, ncell), 0xFF, seed=5)
        gmin, mg = ct.c_double(7.0), ct.c_int64(-1)
        rc = L.tn_gibbs_score(4, 4, ct.cast(table.cells, ct.c_void_p), M, B, d_st.data_ptr(), E.ptr, lq.ptr, cl.ptr, ct.byref(gmin), ct.byref(mg),
                              ws.ptr, need, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert ws.intact() and E.intact() and lq.intact() and cl.intact()
        out[fill] = (E.host(), lq.host(), cl.host(), gmin.value, mg.value)
        assert not np.isnan(out[fill][1]).any() and not np.isnan(out[fill][2]).any() and np.all(np.isfinite(out[fill][0]))
        assert np.all(out[fill][1] < 0) and 1 <= mg.value <= M and gmin.value <= 1.0
    for a, b in zip(out[0xFF][:3], out['random'][:3]):
        assert same_bits(a, b)
    assert out[0xFF][3:] == out['random'][3:]
    Eh, lqh, clh = out[0xFF][:3]
    assert lqh[5] == -np.inf and lqh[6] == -np.inf and clh[5, 7] == -np.inf and clh[6, 0] == -np.inf
    assert np.isfinite(np.delete(clh[5], 7)).all() and np.isfinite(np.delete(lqh, (5, 6))).all()
    # the two rows walked on as state 0: the same later increments and energy as with state 0 given
    rot0 = rot.copy()
    rot0[5, 7] = rot0[6, 0] = 0
    s.calculate_log_probability(rot0[:, np.asarray(s.order)], boundary='keep', cells=True)      # (rotation 0: the order is the identity)
    assert same_bits(s.scored_energy, Eh) and same_bits(np.delete(s.scored_log2q, (5, 6)), np.delete(lqh, (5, 6)))
    assert same_bits(np.delete(s.scored_cell_log2q[5], 7), np.delete(clh[5], 7))
    # a short workspace: -3, nothing written
    ws = Guarded(need - 8, 0xFF, seed=6)
    Eg = Guarded.of(torch.float64, (M,), 0xFF, seed=7)
    clg = Guarded.of(torch.float64, (M, ncell), 0xFF, seed=8)
    gmin = ct.c_double(7.0)
    rc = L.tn_gibbs_score(4, 4, ct.cast(table.cells, ct.c_void_p), M, B, d_st.data_ptr(), Eg.ptr, lq.ptr, clg.ptr, ct.byref(gmin), None, ws.ptr,
                          need - 8, ops._stream())
    torch.cuda.synchronize()
    assert rc == -3
    assert ws.untouched(0xFF) and Eg.untouched(0xFF) and clg.untouched(0xFF) and ws.intact() and gmin.value == 7.0
