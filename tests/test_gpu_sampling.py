"""tnac4o.sample_boltzmann on the GPU: the draw kernel against numpy on the table tn_calc_pn writes, the configurations of the
existing gibbs_sampling path, log-probabilities against the oracle's forced walk, exact log2 Z on small instances in every rotation,
chunk and order invariance, the distribution of the samples, and the workspace contract of tn_gibbs_sample."""
import ctypes as ct
import os

import numpy as np
import pytest

import golden_inputs as gi
import sampling_ref as sref
from guarded import Guarded, same_bits
from oracle import solver_ref as sr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

BETAS = (0.5, 1.0, 3.0)                     # the CASES x BETAS of tests/test_gpu_marginals.py
CASES = sref.CASES
G8 = [(0, 16, 64, 1234), (1, 8, 32, 99)]
SWEEP = dict(graduate_truncation=True, tolS=1e-15, tolV=1e-10, max_sweeps=20)      # the defaults of sample_boltzmann


def load(name):
    return np.load(os.path.join(gi.GOLDEN_DIR, name))


def droplet(rot=0, beta=3.0):
    import tnac4o_amd
    s = tnac4o_amd.tnac4o(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=beta)
    if rot:
        s.rotate_graph(rot)
    return s


def small(case, beta):
    import tnac4o_amd
    from tnac4o_amd import auxx
    import marginals_ref as mr
    if case == 'ising3x3':
        return tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=beta)
    if case == 'rmf3x3':
        return tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=3, J=auxx.synthetic_rmf(3, 3, 3, 17), beta=beta)
    return tnac4o_amd.tnac4o(mode='Ising', Nx=2, Ny=2, Nc=8, J=auxx.synthetic_chimera(2, 2, 29), beta=beta)


def dv(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t.to(dtype) if dtype is not None else t).cuda()


# ---------------------------------------------------------------------------------------------- 1. kernel against numpy
def _kernel_inputs(q, rng, npref=5, nsuf=4, p=6, Dr=7, br=5, nl=3, nu=3):
    T1 = rng.uniform(0.1, 1.0, (npref, p, Dr))
    T1[0, 0] *= -0.01                                   # prefix 0: states with dmap = 0 get small negative entries (the negative rule)
    RR = rng.uniform(0.1, 1.0, (nsuf, Dr, br))
    F = rng.uniform(0.0, 1.0, (q, nl, nu))
    F[rng.random((q, nl, nu)) < 0.3] = 0.0              # tables with zero entries
    F[:, 0, 0] = 0.0                                    # (l, u) = (0, 0): an all-zero table
    if q > 1:
        F[0, 1, 1] = 0.0                                # (l, u) = (1, 1): P[0] = 0
        F[q - 1, 1, 1] = 0.5
    dmap = rng.integers(0, p, q).astype(np.int32)
    rmap = rng.integers(0, br, q).astype(np.int32)
    return T1, RR, F, dmap, rmap


def _groups(sizes, rng, npref, nsuf, nl, nu):
    ng = len(sizes)
    rows = np.stack([rng.integers(0, npref, ng), rng.integers(0, nsuf, ng), rng.integers(0, nl, ng), rng.integers(0, nu, ng)], 1)
    rows[0] = (1, 0, 0, 0)                              # an all-zero table
    if ng > 1:
        rows[1] = (0, 1, 2, 2)                          # a table under the negative rule
    n = int(np.sum(sizes))
    perm = rng.permutation(n).astype(np.int32)          # members of the groups: any sample indices
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return rows.astype(np.int32), perm, starts, n


def _run_kernel(ops, T1, RR, F, dmap, rmap, rows, perm, starts, r, log2p0=None):
    args = [dv(T1), dv(RR), dv(F), dv(dmap), dv(rmap)] + [dv(rows[:, j].copy()) for j in range(4)]
    ng = rows.shape[0]
    P, mP, LP = ops.calc_pn(*args, parent_log2p=torch.zeros(ng, dtype=torch.float64, device='cuda'))
    lq = dv(log2p0) if log2p0 is not None else None
    child, log2p, mP2 = ops.sample_pn(*args, dv(perm), dv(starts), dv(r), log2p=lq)
    torch.cuda.synchronize()
    return P.cpu().numpy(), mP.cpu().numpy(), LP.cpu().numpy(), child.cpu().numpy(), log2p.cpu().numpy(), mP2.cpu().numpy()


@pytest.mark.parametrize('q', [1, 3, 64, 255, 256, 257, 1024, 5000])
def test_sample_pn_against_numpy(q):
    from tnac4o_amd import ops
    rng = np.random.default_rng(100 + q)
    T1, RR, F, dmap, rmap = _kernel_inputs(q, rng)
    sizes = [1, 3000, 1, 2, 255, 256, 257, 700, 5, 64]
    rows, perm, starts, n = _groups(sizes, rng, 5, 4, 3, 3)
    r = rng.random(n)
    P, mP, LP, child, log2p, mP2 = _run_kernel(ops, T1, RR, F, dmap, rmap, rows, perm, starts, r)
    assert same_bits(mP2, mP)
    assert mP[0] == -1.0 and np.all(P[0] == 1.0 / q)                     # the all-zero table came back uniform
    if q >= 64:                                                          # the negative rule was met, and lifted only part of the table
        raw = F[:, 2, 2] * (T1[0] @ RR[1])[dmap, rmap]
        assert raw.min() < 0 < raw.max() and abs(raw.min()) < raw.max()
        assert -1.0 < mP[1] < 0
    assert np.all((child >= 0) & (child < q))
    left_out = 0
    for g in range(len(sizes)):
        for k in perm[starts[g]:starts[g + 1]]:
            assert P[g, child[k]] > 0
            assert same_bits(log2p[k:k + 1], LP[g, child[k]:child[k] + 1]), (g, k)      # the increment: same table, same log2
            if sref.boundary_distance(P[g], r[k]) < 1e-9:                # a different summation order may flip these
                left_out += 1
                continue
            assert child[k] == sref.draw_np(P[g], r[k]), (g, k, r[k])
    print('q = %d: %d of %d draws within 1e-9 of a boundary' % (q, left_out, n))
    assert left_out <= 0.01 * n


def test_sample_pn_adds_to_the_log_probability_and_ignores_other_groups():
    """log2p is updated in place; a sample's draw does not depend on which other samples share the call."""
    from tnac4o_amd import ops
    rng = np.random.default_rng(5)
    q = 300
    T1, RR, F, dmap, rmap = _kernel_inputs(q, rng)
    rows, perm, starts, n = _groups([40, 9, 600], rng, 5, 4, 3, 3)
    r = rng.random(n)
    base = rng.normal(0.0, 5.0, n)
    _, _, LP, child, log2p, _ = _run_kernel(ops, T1, RR, F, dmap, rmap, rows, perm, starts, r, log2p0=base)
    for g in range(3):
        for k in perm[starts[g]:starts[g + 1]]:
            assert log2p[k] == base[k] + LP[g, child[k]]
    # group 2 alone, its members renumbered 0 .. 599
    mem = perm[starts[2]:starts[3]]
    _, _, _, child2, _, _ = _run_kernel(ops, T1, RR, F, dmap, rmap, rows[2:3], np.arange(600, dtype=np.int32), np.array([0, 600], dtype=np.int64),
                                        r[mem].copy())
    assert np.array_equal(child2, child[mem])


def test_sample_pn_edges():
    """The edge rules, where no draw has to be left out: r = 0.0 on a table with P[0] = 0, r = nextafter(1, 0), r above the last
    running sum, q = 1."""
    from tnac4o_amd import ops
    rng = np.random.default_rng(9)
    for q in (4, 300):
        T1, RR, F, dmap, rmap = _kernel_inputs(q, rng)
        rows = np.array([[1, 1, 1, 1]], dtype=np.int32)                  # (l, u) = (1, 1): P[0] = 0, P[q-1] > 0
        r = np.array([0.0, np.nextafter(1.0, 0.0), 1.5, 0.5])
        P, _, LP, child, log2p, _ = _run_kernel(ops, T1, RR, F, dmap, rmap, rows, np.arange(4, dtype=np.int32), np.array([0, 4], dtype=np.int64), r)
        assert P[0, 0] == 0.0 and P[0, q - 1] > 0
        pos = np.flatnonzero(P[0] > 0)
        assert child[0] == pos[0]                                        # forward to the first positive entry
        assert child[2] == pos[-1] == q - 1                              # back to the last positive entry
        assert child[1] == sref.draw_np(P[0], r[1]) == q - 1             # (the last entry holds > 1e-4 of the weight)
        assert child[3] == sref.draw_np(P[0], 0.5)
        assert np.all(np.isfinite(log2p)) and same_bits(log2p, LP[0, child])
    T1, RR, F, dmap, rmap = _kernel_inputs(1, rng)
    rows = np.array([[2, 1, 2, 2], [1, 0, 0, 0]], dtype=np.int32)        # a positive entry, and an all-zero table
    F[0, 2, 2] = 0.7
    r = np.array([0.0, 0.999, 1.5, 0.3])
    P, mP, _, child, log2p, _ = _run_kernel(ops, T1, RR, F, dmap, rmap, rows, np.arange(4, dtype=np.int32), np.array([0, 3, 4], dtype=np.int64), r)
    assert np.all(P == 1.0) and np.all(child == 0) and np.all(log2p == 0.0) and mP[1] == -1.0


# ---------------------------------------------------------------------------------------------- 2. the configurations of gibbs_sampling
@pytest.mark.parametrize('rot,chi,M,seed', G8)
def test_same_configurations_as_golden(rot, chi, M, seed):
    """A seeded run draws the reference's configurations (fixture G8): on the oracle the smallest distance between a uniform number
    and a running sum over all draws of these two cases is 3.1e-5 / 1.7e-5, and no draw overruns the last running sum."""
    from tnac4o_amd import auxx
    g = load('g8_gibbs.npz')
    tag = 'r%d_chi%d_M%d_seed%d' % (rot, chi, M, seed)
    s = droplet(rot)
    np.random.seed(seed)
    E = s.sample_boltzmann(M=M, Dmax=chi)
    assert E is s.energy and E.shape == (M,) and s.states.shape == (M, 16)
    assert np.array_equal(np.asarray(s.states).astype(np.int64), g[tag + '_states'].astype(np.int64))
    np.testing.assert_allclose(E, g[tag + '_energy'], rtol=0, atol=1e-10)
    assert np.array_equal(s.binary_states(), g[tag + '_bits'])
    assert np.abs(auxx.energy_Jij(gi.droplet_J(128, 1), s.binary_states()) - E).max() < 1e-6
    assert s.degeneracy == 0 and s.discarded_probability == 0
    assert s.probability.shape == (M,) and np.all(s.probability < 0) and np.all(np.isfinite(s.probability))
    assert np.array_equal(s.sample_log2Z, -s.beta * E / np.log(2.0) - s.probability)
    assert s.log2Z_lower == pytest.approx(float(np.mean(s.sample_log2Z)), abs=1e-9) and s.log2Z_lower <= s.log2Z_estimate
    assert 1 <= s.sample_max_groups <= M


@pytest.mark.parametrize('rot,chi,M,seed', G8)
def test_back_to_back_with_gibbs_sampling(rot, chi, M, seed, tmp_path):
    s = droplet(rot)
    np.random.seed(seed)
    Eg = np.copy(s.gibbs_sampling(M=M, Dmax=chi))
    stg, neg = np.copy(s.states), s.negative_probability
    np.random.seed(seed)
    Eb = s.sample_boltzmann(M=M, Dmax=chi)
    assert np.array_equal(np.asarray(s.states), stg) and s.states.dtype == stg.dtype
    np.testing.assert_allclose(Eb, Eg, rtol=0, atol=1e-10)
    assert s.negative_probability == pytest.approx(neg, abs=1e-12)
    s.show_solution()                                                    # the result is an ordinary one for the output methods
    f = str(tmp_path / 'samples')
    s.save(f)
    assert any(n.startswith('samples') for n in os.listdir(str(tmp_path)))


# ---------------------------------------------------------------------------------------------- 3. log-probabilities against the oracle
@pytest.mark.parametrize('rot,chi,M,seed', G8)
def test_log_probabilities_against_the_oracle(rot, chi, M, seed):
    """|probability[k] - oracle log2 q[k]| <= sum over the cells of (1e-10 + 1e-14 / P_cell) / ln 2: what follows from the rtol = 1e-10,
    atol = 1e-14 at which the conditional tables of a whole walk are held to the oracle's (tests/test_gpu_configs.py)."""
    s = droplet(rot)
    np.random.seed(seed)
    E = s.sample_boltzmann(M=M, Dmax=chi)
    o = sr.RefSolver(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=3.0)
    if rot:
        o.rotate_graph(rot)
    lq, Pc = sref.oracle_log2q(o, sref.rotated_states(s), Dmax=chi, **SWEEP)
    diff = np.abs(s.probability - lq)
    bound = sref.log2q_bound(Pc)
    k = int(np.argmax(diff / bound))
    print('rot %d chi %d: largest |log2 q - oracle| = %.3e (bound there %.3e), log2 q in [%.2f, %.2f], mean sample_log2Z = %.5f, spread %.2e'
          % (rot, chi, diff.max(), bound[k], lq.min(), lq.max(), float(np.mean(s.sample_log2Z)), float(np.ptp(s.sample_log2Z))))
    assert np.all(diff <= bound), (k, diff[k], bound[k])
    if chi == 16:                                                        # orientation values of the oracle
        assert -25.6 < lq.min() and lq.max() < -3.3
        assert float(np.mean(-3.0 * E / np.log(2.0) - lq)) == pytest.approx(916.34530, abs=1e-4)


# ---------------------------------------------------------------------------------------------- 4. exact on small instances
@pytest.mark.parametrize('beta', BETAS)
@pytest.mark.parametrize('case', CASES)
def test_exact_on_small_instances(case, beta):
    ins = small(case, beta)
    np.random.seed(4321)
    E = ins.sample_boltzmann(M=256, Dmax=64)
    exact = sref.exact_log2Z(case, beta)
    dev = float(np.max(np.abs(ins.sample_log2Z - exact)))
    print('%s beta %.1f: log2 Z = %.12f, largest deviation of a sample %.3e' % (case, beta, exact, dev))
    assert dev <= 1e-10
    assert ins.log2Z_lower <= ins.log2Z_estimate
    assert abs(ins.log2Z_lower - exact) <= 1e-10 and abs(ins.log2Z_estimate - exact) <= 1e-10
    assert float(np.max(np.abs(sref.model_energy(case, ins) - E))) <= 1e-9
    assert -1e-14 < ins.negative_probability <= 0


# ---------------------------------------------------------------------------------------------- 5. chunk and order invariance
def test_chunk_and_order_invariance():
    M = 512
    u = np.random.default_rng(2024).random((16, M))
    res = {}
    for chunk in (512, 64, 7):
        s = droplet()
        s.sample_boltzmann(M=M, Dmax=8, uniforms=u, chunk=chunk)
        res[chunk] = (np.copy(s.states), np.copy(s.energy), np.copy(s.probability))
    for chunk in (64, 7):
        for a, b in zip(res[512], res[chunk]):
            assert same_bits(a, b), chunk
    perm = np.random.default_rng(1).permutation(M)
    s = droplet()
    s.sample_boltzmann(M=M, Dmax=8, uniforms=np.ascontiguousarray(u[:, perm]))
    for a, b in zip(res[512], (s.states, s.energy, s.probability)):
        assert same_bits(a[perm], b)
    # a device tensor is taken as it is
    s = droplet()
    s.sample_boltzmann(M=M, Dmax=8, uniforms=torch.as_tensor(u).cuda(), chunk=200)
    for a, b in zip(res[512], (s.states, s.energy, s.probability)):
        assert same_bits(a, b)


# ---------------------------------------------------------------------------------------------- 6. rotation
@pytest.mark.parametrize('rot', [0, 1, 2, 3])
@pytest.mark.parametrize('case', CASES)
def test_rotation(case, rot):
    ins = small(case, 1.0)
    if rot:
        ins.rotate_graph(rot)
    np.random.seed(7 + rot)
    E = ins.sample_boltzmann(M=64, Dmax=64)
    exact = sref.exact_log2Z(case, 1.0)
    assert float(np.max(np.abs(ins.sample_log2Z - exact))) <= 1e-10
    assert float(np.max(np.abs(sref.model_energy(case, ins) - E))) <= 1e-9      # states come back in model order


# ---------------------------------------------------------------------------------------------- 7. distribution
def test_distribution_of_the_samples():
    """Empirical cell marginals of 2^16 samples against calculate_marginals of the same solver, per entry within 5 standard errors
    5 sqrt(p (1 - p) / M).  A statistical bound: entries with p M < 100 are left out (fewer than a quarter of them, or the test
    fails); with < 40 entries a false alarm has probability < 1e-4, and the seed is fixed."""
    M = 2 ** 16
    ins = small('ising3x3', 0.5)
    marg = [np.copy(m) for m in ins.calculate_marginals(Dmax=64)]
    np.random.seed(20240611)
    ins.sample_boltzmann(M=M, Dmax=64)
    total = skipped = 0
    worst = 0.0
    for k, p in enumerate(marg):
        emp = np.bincount(np.asarray(ins.states[:, k]).astype(np.int64), minlength=p.size) / M
        assert emp.size == p.size
        for a in range(p.size):
            total += 1
            if p[a] * M < 100:
                skipped += 1
                continue
            z = abs(emp[a] - p[a]) / np.sqrt(p[a] * (1.0 - p[a]) / M)
            worst = max(worst, z)
            assert z <= 5.0, (k, a, emp[a], p[a], z)
    print('%d entries, %d left out, worst deviation %.2f standard errors' % (total, skipped, worst))
    assert total < 40 and skipped < 0.25 * total


# ---------------------------------------------------------------------------------------------- 8. workspace contract
def test_gibbs_sample_workspace_contract():
    """tn_gibbs_sample with exactly tn_gibbs_sample_ws_bytes: guards intact for NaN- and random-filled workspaces, results bit-equal
    between the fills; 8 bytes less are rejected with -3 before any launch."""
    from tnac4o_amd import _lib, ops
    from tnac4o_amd.beam import CellTable
    L = _lib.lib()
    s = droplet()
    s._setup_rhoT(Dmax=8, **SWEEP)
    table = CellTable(s)
    assert table.misfit is None
    M, ncell = 96, 16
    B = int(max(np.max(s.ld), np.max(s.lr), 2))
    need = int(L.tn_gibbs_sample_ws_bytes(4, 4, M, table.qmax, table.max_env, table.max_t1, table.max_w))
    u = dv(np.random.default_rng(3).random((ncell, M)))
    out = {}
    for fill in (0xFF, 'random'):
        ws = Guarded(need, fill, seed=1)
        st = Guarded.of(torch.int16, (M, ncell), 0xFF, seed=2)
        E = Guarded.of(torch.float64, (M,), 0xFF, seed=3)
        lq = Guarded.of(torch.float64, (M,), 0xFF, seed=4)
        gmin, mg = ct.c_double(7.0), ct.c_int64(-1)
        rc = L.tn_gibbs_sample(4, 4, ct.cast(table.cells, ct.c_void_p), M, B, u.data_ptr(), M, st.ptr, E.ptr, lq.ptr, ct.byref(gmin), ct.byref(mg),
                               ws.ptr, need, ops._stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert ws.intact() and st.intact() and E.intact() and lq.intact()
        out[fill] = (st.host(), E.host(), lq.host(), gmin.value, mg.value)
        assert np.all(np.isfinite(out[fill][1])) and np.all(out[fill][2] < 0) and 1 <= mg.value <= M and gmin.value <= 1.0
    for a, b in zip(out[0xFF][:3], out['random'][:3]):
        assert same_bits(a, b)
    assert out[0xFF][3:] == out['random'][3:]
    # the driver gives the same numbers
    s.sample_boltzmann(M=M, Dmax=8, uniforms=u.cpu().numpy())
    assert same_bits(s.energy, out[0xFF][1]) and same_bits(s.probability, out[0xFF][2])
    # a short workspace: -3, nothing written
    ws = Guarded(need - 8, 0xFF, seed=5)
    st = Guarded.of(torch.int16, (M, ncell), 0xFF, seed=6)
    gmin = ct.c_double(7.0)
    rc = L.tn_gibbs_sample(4, 4, ct.cast(table.cells, ct.c_void_p), M, B, u.data_ptr(), M, st.ptr, E.ptr, lq.ptr, ct.byref(gmin), None, ws.ptr,
                           need - 8, ops._stream())
    torch.cuda.synchronize()
    assert rc == -3
    assert ws.untouched(0xFF) and st.untouched(0xFF) and ws.intact() and st.intact() and gmin.value == 7.0
