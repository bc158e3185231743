"""GPU parity tests added in round 2: the conditional-probability tables (the marginals, G6) and the PEPS builder
(G4) on the HIP path against the vectors captured from the reference, and the BASELINE.json configurations that had
no test: chimera L=512 at chi=64 over the 4 rotations (config 3), the chi=64, M=1024 search at L=2048 (config 4) and
the Random Markov Field 64 x 64, d=8, chi=128 (config 5) at full size.  Tolerances as in SURVEY.md §8c."""
import os

import numpy as np
import pytest

import golden_inputs as gi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def load(name):
    return np.load(os.path.join(gi.GOLDEN_DIR, name))


def gpu_solver(L=128, ins=1, rot=0, beta=3.0, pre=False, J=None):
    import tnac4o_amd
    n = {128: 4, 512: 8, 2048: 16}[L]
    s = tnac4o_amd.tnac4o(mode='Ising', Nx=n, Ny=n, Nc=8, J=J if J is not None else gi.droplet_J(L, ins), beta=beta)
    if rot:
        s.rotate_graph(rot)
    if pre:
        s.precondition(mode='balancing')
    return s


# ------------------------------------------------------------------------------------------------ G6 on the HIP path
G6_CASES = [(0, 8), (3, 8), (0, 32)]


def _oracle(rot):
    from oracle import solver_ref as sr
    o = sr.RefSolver(mode='Ising', Nx=4, Ny=4, Nc=8, J=gi.droplet_J(128, 1), beta=3.0)
    if rot:
        o.rotate_graph(rot)
    return o


class _beam_order:
    """TN_BEAM for the duration of a block: 'numpy' = host path in numpy's argpartition / argsort order (what the reference and the
    oracle run), 'host' = canonical order on the host, 'device' = canonical order resident on the GPU (tnac4o_amd/beam.py)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.saved = os.environ.get('TN_BEAM')
        os.environ['TN_BEAM'] = self.mode

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop('TN_BEAM', None)
        else:
            os.environ['TN_BEAM'] = self.saved


def _as_ref_chain(m):
    from oracle import mps_ref as mr
    r = mr.RefMPS(d=[int(a.shape[1]) for a in m.A], L=len(m.A), Dmax=1, canonise=None)
    r.A = [a.detach().cpu().numpy() for a in m.A]
    r.D = list(m.D)
    return r


@pytest.mark.parametrize('rot,chi', G6_CASES)
def test_g6_beam_kernels_vs_oracle_on_same_boundary(rot, chi):
    """The marginals machinery proper: _setup_RR (K9), _calculate_Pn incl. the negative-probability rule (K8) and the RL
    update (reference tnac4o.py:1768-1807, 528-535) on the GPU against the CPU oracle's restatement of the same lines, both
    reading the SAME boundary MPS (the GPU's, handed to the oracle through its sweep hook).  Every conditional table of the
    whole search (16 site-steps, up to 1024 branches x 256 states) at 1e-10 relative; min-probability flags likewise.
    Measured on the MI355X: <= 3e-13 relative."""
    s = gpu_solver(rot=rot)
    tr = []
    with _beam_order('numpy'):              # row-for-row comparison with the oracle needs the reference's own (numpy) branch order
        s.search_ground_state(M=1024, relative_P_cutoff=1e-8, Dmax=chi, trace=tr)
    o = _oracle(rot)

    def hook(solver, run):
        solver.rhoT = [_as_ref_chain(m) for m in s.rhoT]
        solver.rhoT_overlap, solver.rhoT_discarded = list(s.rhoT_overlap), list(s.rhoT_discarded)
    tro = []
    o.search_ground_state(M=1024, relative_P_cutoff=1e-8, Dmax=chi, trace=tro, sweep_hook=hook)
    assert len(tr) == len(tro) == 16
    for a, b in zip(tr, tro):
        assert a[2].shape == b[2].shape and np.array_equal(a[4], b[4])          # same branches, same boundary indices
        np.testing.assert_allclose(a[2], b[2], rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(a[3], b[3], rtol=1e-8, atol=1e-14)
    assert s.energy[0] == o.energy[0] and np.array_equal(s.states, o.states)
    assert s.probability[0] == pytest.approx(o.probability[0], abs=1e-12)
    assert s.negative_probability == pytest.approx(o.negative_probability, rel=1e-8, abs=1e-14)


_G6_SPREAD = {}


def g6_reference_spread(rot, chi):
    """Per recorded site-step: how far the reference algorithm's OWN tables move under rounding-level changes -- every QR
    input perturbed by 1e-16 relative, and LAPACK's gesdd swapped for gesvd (the survey's probe).  The
    truncated boundary MPS is an ill-conditioned function of its input wherever kept and discarded Schmidt values are
    close, so some entries amplify eps by ~1e7; this measures that amplification on the instance at hand."""
    import scipy.linalg
    from oracle import mps_ref as mr
    key = (rot, chi)
    if key in _G6_SPREAD:
        return _G6_SPREAD[key]
    g = load('g6_pn.npz')
    tag = 'L128_r%d_chi%d' % (rot, chi)
    spread = {}
    for probe in ('qr', 'svd', 'svdin'):
        orig_qr, orig_svd = mr.qr_pos, scipy.linalg.svd
        if probe == 'qr':
            rng = np.random.default_rng(0)
            mr.qr_pos = lambda T: orig_qr(T * (1 + 1e-16 * rng.standard_normal(T.shape)))
        elif probe == 'svd':
            scipy.linalg.svd = lambda a, *args, **kw: orig_svd(a, *args, **dict(kw, lapack_driver='gesvd'))
        else:               # every centre matrix perturbed by 1e-16 relative before its SVD (what another backward-stable SVD amounts to)
            rng2 = np.random.default_rng(1)
            scipy.linalg.svd = lambda a, *args, **kw: orig_svd(a * (1 + 1e-16 * rng2.standard_normal(np.shape(a))), *args, **kw)
        try:
            o = _oracle(rot)
            tr = []
            o.search_ground_state(M=1024, relative_P_cutoff=1e-8, Dmax=chi, trace=tr)
        finally:
            mr.qr_pos, scipy.linalg.svd = orig_qr, orig_svd
        for k in g[tag + '_steps']:
            st = int(g[tag + '_stride%d' % k][0])
            d = float(np.abs(tr[k][2][::st] - g[tag + '_P%d' % k]).max())
            spread[int(k)] = max(spread.get(int(k), 0.0), d)
    _G6_SPREAD[key] = spread
    return spread


@pytest.mark.parametrize('rot,chi', G6_CASES)
def test_g6_marginals_hip_vs_reference_golden(rot, chi):
    """End to end (GPU sweep + GPU beam) against the `newprob` tables captured from the reference at 9-10 site-steps, incl.
    the rot=3 run whose tables contain negative entries.  Tolerance per table: 1e-10 relative or, in
    absolute terms on the normalised table, 10x the movement of the reference algorithm's own tables under eps-level
    probes (g6_reference_spread: QR inputs, SVD inputs, SVD driver) with a floor of 1e-12.  The beam kernels themselves agree with
    the oracle to 3e-13 on a common boundary MPS (previous test): what is left here is the conditioning of the truncated sweep.
    The measured margins (largest |difference| / allowance per table) are printed."""
    g = load('g6_pn.npz')
    tag = 'L128_r%d_chi%d' % (rot, chi)
    trace = []
    s = gpu_solver(rot=rot)
    with _beam_order('numpy'):              # the golden tables are in the reference's branch order
        s.search_ground_state(M=1024, relative_P_cutoff=1e-8, Dmax=chi, trace=trace)
    assert [t[2].shape[0] for t in trace] == list(g[tag + '_nbranch'])
    spread = g6_reference_spread(rot, chi)
    worst = 0.0
    for k in g[tag + '_steps']:
        st = int(g[tag + '_stride%d' % k][0])
        atol = max(1e-12, 10.0 * spread[int(k)])
        want = g[tag + '_P%d' % k]
        margin = float((np.abs(trace[k][2][::st] - want) / (atol + 1e-10 * np.abs(want))).max())
        worst = max(worst, margin)
        print('G6 %s step %d: max |dP| %.2e, probe spread %.2e, allowance used %.2f' % (tag, k, float(np.abs(trace[k][2][::st] - want).max()),
                                                                                     spread[int(k)], margin))
        np.testing.assert_allclose(trace[k][2][::st], want, rtol=1e-10, atol=atol)
        np.testing.assert_allclose(trace[k][3][::st], g[tag + '_min%d' % k], rtol=1e-6, atol=atol)
    print('G6 %s: worst margin %.2f of the allowance' % (tag, worst))
    assert s.negative_probability == pytest.approx(g[tag + '_neg'][0], rel=1e-6, abs=1e-13)


# ------------------------------------------------------------------------------------------------ K7 vs G4
@pytest.mark.parametrize('pre', [False, True])
def test_k7_mpo_site_vs_reference_g4(pre):
    """tn_peps_factor + tn_mpo_from_factor against W = sum_s _peps_tensor captured from the reference (tnac4o.py:1562-1672,
    1686), with and without the preconditioning gauges (taken from the golden file, so that only the builder is tested)."""
    g = load('g4_peps.npz')
    s = gpu_solver()
    if pre:
        s.Xu, s.Xd = g['L128_pre1_Xu'].copy(), g['L128_pre1_Xd'].copy()
    for (ny, nx) in [(0, 0), (1, 1), (3, 3), (0, 3), (2, 0)]:
        tag = 'L128_pre%d_%d_%d' % (int(pre), ny, nx)
        W = s._mpo_site_dev(ny, nx).cpu().numpy()
        q, bl, pd, br, pu = (int(x) for x in g[tag + '_shape'])
        assert W.shape == (bl, pd, br, pu)
        if tag + '_W' in g.files:
            np.testing.assert_allclose(W, g[tag + '_W'], rtol=1e-13)
        np.testing.assert_allclose([W.sum(), (W ** 2).sum(), W.max(), W[W > 0].min()], g[tag + '_Wsum'], rtol=1e-12)
        np.testing.assert_allclose(W.reshape(-1)[::997], g[tag + '_probe'], rtol=1e-13)


def test_k7_rmf_factor_vs_reference_g4():
    """RMF branch of the builder (tnac4o.py:1609-1670): the dense 5-leg tensor of the reference rebuilt from the device
    factor, T[s,l,d,r,u] = F[s,l,u] [d = dmap[s]] [r = rmap[s]]."""
    import tnac4o_amd
    g = load('g4_peps.npz')
    J = gi.minimal_rmf()
    s = tnac4o_amd.tnac4o(mode='RMF', Nx=J['Nx'], Ny=J['Ny'], J=J, beta=2.0)
    for (ny, nx) in [(0, 0), (1, 2), (2, 4)]:
        F, dm, rm, pd, br = s._peps_factor_dev(ny, nx)
        F, dm, rm = F.cpu().numpy(), dm.cpu().numpy(), rm.cpu().numpy()
        q, nl, nu = F.shape
        T = np.zeros((q, nl, pd, br, nu))
        for st in range(q):
            T[st, :, dm[st], rm[st], :] = F[st]
        np.testing.assert_allclose(T, g['rmf_%d_%d_T' % (ny, nx)], rtol=1e-13)


# ------------------------------------------------------------------------------------------------ config 3
def test_config3_L512_chi64_four_rotations_golden():
    """BASELINE config 3: chimera L=512 (droplet #1) at chi=64, the 4 lattice rotations of examples/e06:97-109 solved
    concurrently on one GPU through solve_rotations: the reference's golden energy -846.96 and bit string from every
    rotation, plus the sweep diagnostics at chi=64."""
    import tnac4o_amd
    from tnac4o_amd.parallel import solve_rotations
    J = gi.droplet_J(512, 1)
    E, bits = gi.golden_groundstate(512, 1)
    solvers = []

    def make():
        s = tnac4o_amd.tnac4o(mode='Ising', Nx=8, Ny=8, Nc=8, J=J, beta=3.0)
        solvers.append(s)
        return s
    res = solve_rotations(make, rotations=(0, 1, 2, 3), concurrent=True, M=1024, relative_P_cutoff=1e-8, Dmax=64)
    assert res['energy'] == pytest.approx(E, abs=1e-5)
    assert len(res['records']) == 4
    for r in res['records']:
        assert r['energy'] == pytest.approx(res['energy'], abs=1e-10)       # every rotation finds the ground state
        assert r['degeneracy'] == res['degeneracy']
    for s in solvers:
        assert np.array_equal(s.binary_states()[0], bits)
        assert tnac4o_amd.energy_Jij(J, s.binary_states()[:1])[0] == pytest.approx(s.energy[0], abs=1e-9)
        assert min(s.rhoT_overlap) > 1 - 1e-10 and max(s.rhoT_discarded) < 1e-8
        assert max(max(m.D) for m in s.rhoT) <= 64
    # chi=64 against chi=32 (pinned by the reference's G7 vector): same state, log2 P within the truncation error
    lp = [float(s.probability[0]) for s in solvers if s.rotation == 0][0]
    import json
    with open(os.path.join(gi.GOLDEN_DIR, 'g7_search.json')) as f:
        want = json.load(f)['L512_i1_r0_chi32_pre0']
    assert lp == pytest.approx(want['probability'], abs=1e-4)


# ------------------------------------------------------------------------------------------------ config 4
def test_config4_L2048_chi64_M1024_search_two_rotations():
    """BASELINE config 4 on one GPU: the full chi=64, M=1024 search on the synthetic chimera instance bench.py times
    (seed 20260004), from two lattice rotations interleaved on the device: both must return the same energy, which must
    be the energy the couplings give to the returned bit string, and the droplet-2048 golden energy at chi=64."""
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_chimera
    from tnac4o_amd.parallel import solve_rotations
    J = synthetic_chimera(16, 16, 20260004)
    solvers = []

    def make():
        s = tnac4o_amd.tnac4o(mode='Ising', Nx=16, Ny=16, Nc=8, J=J, beta=3.0)
        solvers.append(s)
        return s
    res = solve_rotations(make, rotations=(0, 1), concurrent=True, M=1024, relative_P_cutoff=1e-8, Dmax=64)
    e = [r['energy'] for r in res['records']]
    assert e[0] == pytest.approx(e[1], abs=1e-10)
    for s in solvers:
        assert tnac4o_amd.energy_Jij(J, s.binary_states()[:1])[0] == pytest.approx(s.energy[0], abs=1e-8)
        assert min(s.rhoT_overlap) > 1 - 1e-10
        assert max(max(m.D) for m in s.rhoT) == 64
    # same state from both directions unless the ground state is degenerate
    if res['degeneracy'] == 1:
        assert np.array_equal(solvers[0].binary_states()[0], solvers[1].binary_states()[0])


def test_config4_droplet2048_chi64_golden_energy():
    """The reference's largest bundled instance at the headline bond dimension chi=64 (round 1 pinned it at chi=32)."""
    import tnac4o_amd
    s = gpu_solver(L=2048)
    s.search_ground_state(M=1024, relative_P_cutoff=1e-8, Dmax=64)
    E, bits = gi.golden_groundstate(2048, 1)
    assert s.energy[0] == pytest.approx(E, abs=1e-5)
    J = gi.droplet_J(2048, 1)
    assert tnac4o_amd.energy_Jij(J, s.binary_states()[:1])[0] == pytest.approx(s.energy[0], abs=1e-8)
    assert tnac4o_amd.energy_Jij(J, bits[None, :])[0] == pytest.approx(s.energy[0], abs=1e-8)


# ------------------------------------------------------------------------------------------------ config 5
def test_config5_rmf64_d8_chi128_fullsize():
    """BASELINE config 5 at full size: Random Markov Field 64 x 64, d=8, chi=128 (absorbed bond 1024 with p=b=8; 64 rows
    of 64 sites).  The oracle would need hours, so the checks are size-independent properties: compression overlaps,
    canonical form and bond caps of the boundary MPS, and energy_RMF consistency of the state found."""
    import tnac4o_amd
    from tnac4o_amd.auxx import synthetic_rmf, energy_RMF
    J = synthetic_rmf(64, 64, 8, 20260005)
    s = tnac4o_amd.tnac4o(mode='RMF', Nx=64, Ny=64, J=J, beta=1.0)
    s.search_ground_state(M=64, relative_P_cutoff=1e-8, Dmax=128)
    assert min(s.rhoT_overlap) > 1 - 1e-9 and max(s.rhoT_overlap) < 1 + 1e-9
    assert max(max(m.D) for m in s.rhoT) <= 128
    for ny in (1, 31, 60):
        psi = s.rhoT[ny]
        assert psi.D[0] == psi.D[-1] == 1
        for A in psi.A[::9]:
            M = A.reshape(-1, A.shape[2])
            G = tnac4o_amd.ops.mm(M.t(), M)
            assert float((G - torch.eye(M.shape[1], dtype=torch.float64, device='cuda')).abs().max()) < 1e-11
    assert s.states.shape[1] == 64 * 64
    assert energy_RMF(J, s.states[:1])[0] == pytest.approx(s.energy[0], abs=1e-8)
    assert np.isfinite(s.probability[0]) and s.probability[0] < 0 and abs(s.negative_probability) < 1e-8


# ------------------------------------------------------------------------------------------------ a12 on the device
def _solve_with(mode, make, **kw):
    with _beam_order(mode):
        s = make()
        s.search_ground_state(**kw)
        return s


@pytest.mark.parametrize('case', ['L128_1', 'L128_2_rot1', 'L128_3_chi32', 'L512', 'J124', 'rmf', 'L128_nocut', 'L128_M1'])
def test_beam_on_device_bit_identical_to_host_merge(case):
    """a12 (reference tnac4o.py:437-537: cut-off, merge of equal boundary indices, top-M) resident on the GPU -- walked by the library
    (tn_beam_search: hipCUB radix sorts, tn_merge_groups) and by the torch driver of tnac4o_amd/beam.py (torch.unique on rank keys,
    tn_merge_groups, stable sorts) -- against the same canonical order evaluated with numpy on the host:
    energies, degeneracies, log-probabilities, discarded / negative probabilities and the state table must agree bit for bit --
    also on the degenerate J124 instance (degeneracy 1152, ties inside merge groups) and on the dense RMF path."""
    import tnac4o_amd
    import golden_inputs as gi
    kw = dict(M=1024, relative_P_cutoff=1e-8, Dmax=8)
    if case == 'L128_1':
        make = lambda: gpu_solver()
    elif case == 'L128_2_rot1':
        make = lambda: gpu_solver(ins=2, rot=1)
    elif case == 'L128_nocut':                                    # no probability cut-off: every candidate reaches the merge, top-M does the pruning
        make, kw = (lambda: gpu_solver(ins=2, rot=3)), dict(M=48, relative_P_cutoff=0.0, Dmax=8)
    elif case == 'L128_M1':                                       # greedy descent: one branch
        make, kw = (lambda: gpu_solver()), dict(M=1, relative_P_cutoff=1e-3, Dmax=8)
    elif case == 'L128_3_chi32':
        make, kw = (lambda: gpu_solver(ins=3, rot=2)), dict(M=1024, relative_P_cutoff=1e-8, Dmax=32)
    elif case == 'L512':
        make, kw = (lambda: gpu_solver(L=512)), dict(M=1024, relative_P_cutoff=1e-8, Dmax=32)
    elif case == 'J124':
        def make():
            s = tnac4o_amd.tnac4o(mode='Ising', Nx=8, Ny=8, Nc=8, J=gi.j124_J(1), beta=0.75)
            s.precondition(mode='balancing')
            return s
        kw = dict(M=4096, relative_P_cutoff=1e-8, Dmax=8)
    else:
        from tnac4o_amd.auxx import synthetic_rmf
        make = lambda: tnac4o_amd.tnac4o(mode='RMF', Nx=6, Ny=5, J=synthetic_rmf(6, 5, 4, 77), beta=1.0)
        kw = dict(M=64, relative_P_cutoff=1e-8, Dmax=16)
    from tnac4o_amd import beam
    calls = []
    orig = beam.search_native

    def spy(*args, **kwargs):
        out = orig(*args, **kwargs)
        calls.append(out is not None)
        return out
    beam.search_native = spy
    try:
        a = _solve_with('device', make, **kw)                    # tn_beam_search (csrc/beamsearch.hip): the whole loop in the library
    finally:
        beam.search_native = orig
    assert calls == [True], 'the library walk was not the path that ran'
    saved, beam.NATIVE_BEAM = beam.NATIVE_BEAM, False
    try:
        t = _solve_with('device', make, **kw)                    # the torch driver of tnac4o_amd/beam.py (what a beam group runs)
    finally:
        beam.NATIVE_BEAM = saved
    b = _solve_with('host', make, **kw)
    for x in (a, t):
        assert np.array_equal(x.energy, b.energy) and np.array_equal(x.probability, b.probability)
        assert int(x.degeneracy) == int(b.degeneracy) and np.array_equal(x.states, b.states) and x.states.dtype == b.states.dtype
        assert x.discarded_probability == b.discarded_probability and x.negative_probability == b.negative_probability
    if case == 'J124':
        assert a.energy[0] == pytest.approx(-2309.0, abs=1e-9) and int(a.degeneracy) == 1152
