"""tnac4o.relax_samples without a GPU: the move the device kernel is pinned to (tests/relax_ref.py) leaves the Boltzmann law invariant;
the seeded cases shared with the GPU tests keep every draw away from a boundary of the running sum; the quench reference descends,
stops at fixed points and breaks ties to the smallest state; the argument checks raise before any device work; and the reference's own
chain passes the statistic the GPU chain is held to."""
import numpy as np
import pytest

import relax_ref as rr


def test_sweep_leaves_the_boltzmann_law_invariant():
    """2 x 2 cells of q = 4 (256 configurations), random real couplings, beta = 0.7: pi P = pi for the exact sweep matrix."""
    cells, beta = rr.law_problem()
    P = rr.sweep_matrix(cells, 2, 2, beta)
    _, pi = rr.boltzmann(cells, 2, 2, beta)
    assert P.shape == (256, 256) and float(np.max(np.abs(P.sum(axis=1) - 1.0))) <= 1e-13
    dev = float(np.sum(np.abs(pi @ P - pi)))
    print('|| pi P - pi ||_1 = %.3e' % dev)
    assert dev <= 1e-13
    assert float(np.sum(np.abs(np.full(256, 1.0 / 256) @ P - pi))) > 1e-3          # (not because P is trivial: one sweep does not mix)


def test_sweep_matrix_is_the_law_of_the_reference_move():
    """The matrix and the sampled move are the same object: from one fixed configuration, the frequencies of 2^14 reference sweeps with
    seeded uniforms against that row of P."""
    cells, beta = rr.law_problem()
    P = rr.sweep_matrix(cells, 2, 2, beta)
    rng = np.random.default_rng(5)
    start = np.tile(np.array([[1, 3, 0, 2]]), (2 ** 14, 1))
    out = rr.run(cells, 2, 2, start, 0, 1, beta, rng.random((1, 4, 2 ** 14)))
    ok, z, bins = rr.law_statistic(rr.configuration_index(out['states']), P[int(rr.configuration_index(start[:1])[0])])
    print('largest deviation %.2f sigma over %d bins' % (z, bins))
    assert ok


@pytest.mark.parametrize('case', rr.CASES, ids=lambda c: '%s-%s-M%d%s' % (c[0], 'maps' if c[1] else 'nomaps', c[2], '-int' if c[4] else ''))
def test_margin_condition(case):
    """A condition on the inputs, not a measurement: every heat-bath draw of every shared case lies at least 1e-9 W away from every
    running sum, so the device's exp and summation order (about q 2^-52 <= 1e-11 relative) cannot move a draw across a boundary."""
    ref = rr.case_reference(case, 0)
    print('smallest margin %.3e' % ref['margin'])
    assert ref['margin'] >= 1e-9


def test_quench_reference():
    for case in rr.CASES:
        Ny, Nx, cells, states, _ = rr.case_inputs(case)
        ref = rr.case_reference(case, 1)
        E = ref['energies']
        assert np.all(E[1:] <= E[:-1])                                             # non-increasing per sweep, sample by sample
        fixed = ref['last_moves'] == 0
        again = rr.run(cells, Nx, Ny, ref['states'], 1, 1)
        assert np.array_equal(again['states'][fixed], ref['states'][fixed]) and np.all(again['moves'][fixed] == 0)
        # a converged state: no cell has a strictly better state
        for k in range(Nx * Ny):
            e = rr.cond_energy(cells, Nx, Ny, ref['states'][fixed], k)
            cur = e[np.arange(e.shape[0]), ref['states'][fixed][:, k]]
            assert np.all(e.min(axis=1) >= cur)
    assert any(np.any(rr.case_reference(c, 1)['moves'] > 0) for c in rr.CASES)


def test_quench_ties_go_to_the_smallest_state():
    e = np.array([[3.0, 1.0, 1.0, 2.0],       # two minima: the smaller index
                  [1.0, 1.0, 1.0, 1.0],       # the current state already attains the minimum: it stays
                  [2.0, 0.0, 5.0, 0.0]])
    assert np.array_equal(rr.quench_choice(e, [0, 2, 3]), [1, 2, 3])
    assert np.array_equal(rr.quench_choice(e, [3, 4, -1]), [1, 0, 1])              # outside the cell: +inf, always replaced
    # on a lattice with integer tables ties occur and the whole run obeys the rule
    case = rr.CASES[-1]
    assert case[4]
    Ny, Nx, cells, states, _ = rr.case_inputs(case)
    ties = 0
    for k in range(Nx * Ny):
        e = rr.cond_energy(cells, Nx, Ny, states, k)
        ties += int(np.sum((e == e.min(axis=1, keepdims=True)).sum(axis=1) > 1))
    assert ties > 0


def test_check_sweep_uniforms():
    from tnac4o_amd import relax
    good = np.random.default_rng(0).random((2, 9, 5))
    assert relax.check_sweep_uniforms(good, 2, 9, 5) is good
    np.random.seed(3)
    drawn = relax.check_sweep_uniforms(None, 2, 9, 5)
    np.random.seed(3)
    assert drawn.shape == (2, 9, 5) and np.array_equal(drawn, np.random.rand(2, 9, 5))
    bad_nan, bad_one = good.copy(), good.copy()
    bad_nan[1, 2, 3] = np.nan
    bad_one[0, 0, 0] = 1.0
    for bad in (good[:1], good[:, :8], good.reshape(2, 45), good.astype(np.float32), bad_nan, bad_one, -good, good.tolist(), 'x'):
        with pytest.raises(ValueError):
            relax.check_sweep_uniforms(bad, 2, 9, 5)
    torch = pytest.importorskip('torch')
    t = torch.as_tensor(good)
    assert relax.check_sweep_uniforms(t, 2, 9, 5) is t
    for bad in (torch.as_tensor(bad_nan), torch.as_tensor(bad_one), t.float(), t[:1]):
        with pytest.raises(ValueError):
            relax.check_sweep_uniforms(bad, 2, 9, 5)


def test_relax_samples_argument_checks_raise_before_any_device_work(monkeypatch):
    import marginals_ref as mr
    import tnac4o_amd
    from tnac4o_amd import relax

    def no_device(*a, **k):
        raise AssertionError('device work was started')
    monkeypatch.setattr(relax, 'relax_native', no_device)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=1.0)
    ok = np.zeros((5, 9), dtype=np.int64)
    u = np.random.default_rng(1).random((1, 9, 5))
    with pytest.raises(ValueError, match='mode'):
        ins.relax_samples(states=ok, mode='x')
    with pytest.raises(ValueError, match='uniforms'):
        ins.relax_samples(states=ok, mode='quench', uniforms=u)
    with pytest.raises(ValueError, match='sweeps'):
        ins.relax_samples(states=ok, sweeps=None)                                  # until nothing moves: quench only
    for sweeps in (-1, 1.5):
        with pytest.raises(ValueError, match='sweeps'):
            ins.relax_samples(states=ok, sweeps=sweeps)
    for beta in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match='beta'):
            ins.relax_samples(states=ok, beta=beta)
    with pytest.raises(ValueError, match='max_sweeps'):
        ins.relax_samples(states=ok, mode='quench', sweeps=None, max_sweeps=0)
    bad_one = u.copy()
    bad_one[0, 4, 2] = 1.0
    for bad in (u[:, :, :4], u.astype(np.float32), bad_one, np.full_like(u, np.nan)):
        with pytest.raises(ValueError, match='uniforms'):
            ins.relax_samples(states=ok, uniforms=bad)
    with pytest.raises(ValueError, match='uniforms'):
        ins.relax_samples(states=ok, sweeps=2, uniforms=u)                         # one sweep of numbers for two sweeps
    b = ok.copy()
    b[3, 4] = 2                                                                    # model cell 4 holds the inactive spin: two states
    with pytest.raises(ValueError, match=r'states\[3, 4\]'):
        ins.relax_samples(states=b)
    for bad in (ok[:, :8], ok.astype(np.float64), ok.tolist()):
        with pytest.raises(ValueError):
            ins.relax_samples(states=bad)
    with pytest.raises(ValueError):
        ins.relax_samples()                                                        # no stored states
    with pytest.raises(ValueError, match='chunk'):
        ins.relax_samples(states=ok, chunk=0)
    assert not hasattr(ins, 'relax_moves') and ins.states.shape[0] == 0


def test_statistic_passes_on_the_reference_chain():
    """The test the GPU chain is held to (tests/test_gpu_relax.py), on the reference's own chain and the same seed: 2^14 chains from
    uniformly random states, 5 sweeps, against the exact law mu0 P^5."""
    cells, beta, states, uniforms, law = rr.law_inputs()
    assert abs(float(law.sum()) - 1.0) <= 1e-13
    out = rr.run(cells, 2, 2, states, 0, rr.LAW_SWEEPS, beta, uniforms)
    assert out['margin'] >= 1e-9                                                   # (the margin condition holds for this input too)
    ok, z, bins = rr.law_statistic(rr.configuration_index(out['states']), law)
    print('largest deviation %.2f sigma over %d bins (margin %.2e)' % (z, bins, out['margin']))
    assert ok and bins > 50
