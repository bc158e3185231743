"""The numpy reference of tn_line_sweep / tnac4o.relax_lines (tests/lines_ref.py) against enumeration, the margin floor of the shared
cases, and the host-side argument rules of relax_lines (no GPU)."""
import numpy as np
import pytest

import lines_ref as lr
import relax_ref as rr

# (Ny, Nx, q of every cell, maps, seed, integer tables): lattices small enough to enumerate a line
SMALL = [(2, 3, [3, 4, 2, 5, 3, 4], True, 5, False), (3, 2, [4, 3, 2, 5, 3, 2], False, 6, False), (2, 2, [4, 3, 5, 2], True, 7, False),
         (2, 3, [3, 4, 2, 5, 3, 4], True, 8, True), (2, 2, [4, 3, 5, 2], False, 9, True)]
SMALL_IDS = ['%dx%d-%s%s' % (c[0], c[1], 'maps' if c[3] else 'nomaps', '-int' if c[5] else '') for c in SMALL]


def _small(case, M=6):
    Ny, Nx, qs, maps, seed, integer = case
    cells = rr.make_cells(Ny, Nx, qs, maps, seed, integer)
    states = np.random.default_rng(seed + 1).integers(0, np.asarray(qs)[None, :], size=(M, len(qs)))
    return Ny, Nx, cells, states


@pytest.mark.parametrize('case', SMALL[:3], ids=SMALL_IDS[:3])
def test_recursion_gives_the_enumerated_conditional_law(case):
    """Forward filtering / backward sampling assigns every configuration of a row, and of a column, the enumerated conditional
    Boltzmann probability, to 1e-13."""
    Ny, Nx, cells, states = _small(case)
    cT, perm = lr.transpose(cells, Nx, Ny)
    worst = 0.0
    for st in states[:3]:
        for ny in range(Ny):
            _, p = lr.line_law(cells, Nx, Ny, st, ny, 0.8)
            _, pc = lr.line_conditional(cells, Nx, Ny, st, ny, 0.8)
            worst = max(worst, float(np.abs(p - pc).max()))
        for nx in range(Nx):                                               # a column: a row of the transposed lattice
            _, p = lr.line_law(cT, Ny, Nx, st[perm], nx, 0.8)
            _, pc = lr.line_conditional(cT, Ny, Nx, st[perm], nx, 0.8)
            worst = max(worst, float(np.abs(p - pc).max()))
    print('largest deviation %.2e' % worst)
    assert worst <= 1e-13


def test_transposed_energy_is_the_energy():
    """total_energy of the transposed lattice on the permuted states: the same sum in another order."""
    Ny, Nx, cells, states = _small(SMALL[0])
    cT, perm = lr.transpose(cells, Nx, Ny)
    assert np.allclose(rr.total_energy(cT, Ny, Nx, states[:, perm]), rr.total_energy(cells, Nx, Ny, states), rtol=0, atol=1e-12)


@pytest.mark.parametrize('lines', ['rows', 'columns', 'both'])
def test_sweep_leaves_the_boltzmann_law_invariant(lines):
    """pi P = pi and P 1 = 1 for the sweep matrix built from enumerated line conditionals."""
    cells, beta = rr.law_problem()
    P = lr.sweep_matrix(cells, 2, 2, beta, lines)
    _, pi = rr.boltzmann(cells, 2, 2, beta)
    assert np.abs(P.sum(axis=1) - 1.0).max() <= 1e-13
    assert np.abs(pi @ P - pi).max() <= 1e-14


def test_sweep_matrix_is_the_law_of_the_reference_move():
    """One 'both' sweep of the reference from every configuration of a 2 x 2 lattice of small cells, many draws: the frequencies follow
    the rows of the enumerated sweep matrix (6 sigma, bins below 20 pooled)."""
    cells = rr.make_cells(2, 2, [2, 3, 2, 2], False, 31)
    beta = 0.7
    P = lr.sweep_matrix(cells, 2, 2, beta, 'both')
    X = rr.all_configurations(cells)
    qs = np.array([c['q'] for c in cells])
    radix = np.concatenate([np.cumprod(qs[::-1])[::-1][1:], [1]])
    M = 4000
    rng = np.random.default_rng(5)
    for i in (0, 7, X.shape[0] - 1):
        st, _, _, _ = lr.sweep(cells, 2, 2, np.repeat(X[i][None, :], M, axis=0), 0, 'both', beta, rng.random((2, 4, M)))
        ok, z, _ = rr.law_statistic(st @ radix, P[i])
        assert ok, (i, z)


@pytest.mark.parametrize('case', SMALL, ids=SMALL_IDS)
def test_quench_is_the_brute_force_minimum(case):
    """quench_row against enumeration with the tie rule (smallest in the order (s_{Nx-1}, ..., s_0); the line stays unless E* < c),
    rows and columns, integer tables -- where minima tie -- included; a second application moves nothing."""
    Ny, Nx, cells, states = _small(case, M=12)
    cT, perm = lr.transpose(cells, Nx, Ny)
    for lat, nx_, ny_, sts in ((cells, Nx, Ny, states), (cT, Ny, Nx, states[:, perm])):
        for ny in range(ny_):
            new, _ = lr.quench_row(lat, nx_, ny_, sts, ny)
            for m in range(sts.shape[0]):
                best, Estar, c = lr.brute_line_minimum(lat, nx_, ny_, sts[m], ny)
                assert np.array_equal(new[m], best), (ny, m)
                assert Estar <= c
            again = sts.copy()
            again[:, ny * nx_:(ny + 1) * nx_] = new
            assert np.array_equal(lr.quench_row(lat, nx_, ny_, again, ny)[0], new)


def test_quench_ties_go_to_the_smallest_from_the_far_end():
    """All tables zero: every line configuration ties, the current line attains the minimum and stays; from a state outside its cell
    (+inf) the line moves to (0, .., 0)."""
    cells = rr.make_cells(1, 3, [3, 2, 4], False, 1, integer=True)
    for c in cells:
        for key in ('Es', 'E1', 'E4'):
            if c[key] is not None:
                c[key] = np.zeros_like(c[key])
    st = np.array([[2, 1, 3], [2, 5, 3], [-1, 0, 0]])
    new, _ = lr.quench_row(cells, 3, 1, st, 0)
    assert np.array_equal(new, [[2, 1, 3], [0, 0, 0], [0, 0, 0]])


@pytest.mark.parametrize('case', lr.CASES, ids=lr.CASE_IDS)
def test_margin_floor_and_descent(case):
    """Every heat-bath draw of a shared case lies at least 1e-9 of the total weight away from a boundary of the running sum, every
    real-table quench decision is at least 1e-9 wide, and the quench never raises the energy."""
    heat, quench = lr.case_reference(case, 0), lr.case_reference(case, 1)
    print('margin %.2e gap %.2e' % (heat['margin'], quench['gap']))
    assert heat['margin'] >= lr.MARGIN_FLOOR
    if not case[4]:
        assert quench['gap'] >= lr.MARGIN_FLOOR
    assert np.all(np.diff(quench['energies'], axis=0) <= 0)
    assert np.all(np.isfinite(heat['energy']))


def test_steep_case_lies_under_the_guard():
    Ny, Nx, cells, beta, states, u = lr.steep_inputs()
    r = beta * lr.chain_ranges(cells, Nx, Ny, 'both')
    assert 200.0 <= r <= 300.0
    ref = lr.run(cells, Nx, Ny, states, 0, 1, 'both', beta, u)
    assert ref['margin'] >= lr.MARGIN_FLOOR


def test_statistic_passes_on_the_reference_chain():
    """The law test the GPU chain is held to, on the reference's own chain and the same seed; the pooled bin holds less than 10 % of
    the mass."""
    cells, beta, states, u, law_rows, law_both = lr.law_inputs()
    for lines, sweeps, law in (('rows', 1, law_rows), ('both', 2, law_both)):
        ref = lr.run(cells, 2, 2, states, 0, sweeps, lines, beta, u[:sweeps, :len(lr.PASSES[lines])])
        ok, z, bins = rr.law_statistic(rr.configuration_index(ref['states']), law)
        assert ok, (lines, z, bins)
        assert law[lr.LAW_M * law < 20.0].sum() < 0.1


def test_rng_relax_line_rows_are_reproducible():
    from tnac4o_amd import rng
    assert rng.RELAX_LINE == 12
    a = rng.rows_host(5, rng.RELAX_LINE, 0, 2 * 2 * 4, 0, 9)
    b = rng.rows_host(5, rng.RELAX_LINE, 3, 2, 4, 5)
    assert np.array_equal(a[3:5, 4:9], b) and np.all((a >= 0) & (a < 1))
    assert not np.array_equal(a, rng.rows_host(5, rng.RELAX_SWEEP, 0, 16, 0, 9))
    assert not np.array_equal(a, rng.rows_host(6, rng.RELAX_LINE, 0, 16, 0, 9))


def test_check_line_uniforms():
    from tnac4o_amd import lines
    u = np.random.default_rng(1).random((2, 2, 9, 5))
    assert lines.check_line_uniforms(u, 2, 2, 9, 5) is u
    np.random.seed(3)
    d = lines.check_line_uniforms(None, 1, 1, 4, 3)
    np.random.seed(3)
    assert np.array_equal(d, np.random.rand(1, 1, 4, 3))
    bad_one = u.copy()
    bad_one[1, 0, 4, 2] = 1.0
    for bad in (u[:, :1], u[..., :4], u.astype(np.float32), bad_one, np.full_like(u, np.nan), u.tolist(), u.reshape(4, 9, 5)):
        with pytest.raises(ValueError, match='uniforms'):
            lines.check_line_uniforms(bad, 2, 2, 9, 5)


def test_relax_lines_argument_checks_raise_before_any_device_work(monkeypatch):
    import marginals_ref as mr
    import tnac4o_amd
    from tnac4o_amd import lines

    def no_device(*a, **k):
        raise AssertionError('device work was started')
    monkeypatch.setattr(lines, 'lines_native', no_device)
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=1.0)
    ok = np.zeros((5, 9), dtype=np.int64)
    u = np.random.default_rng(1).random((1, 2, 9, 5))
    for bad in ('diagonals', 2, None):
        with pytest.raises(ValueError, match='lines'):
            ins.relax_lines(states=ok, lines=bad)
    with pytest.raises(ValueError, match='mode'):
        ins.relax_lines(states=ok, mode='x')
    with pytest.raises(ValueError, match='uniforms'):
        ins.relax_lines(states=ok, mode='quench', uniforms=u)
    with pytest.raises(ValueError, match='seed'):
        ins.relax_lines(states=ok, mode='quench', seed=1)
    with pytest.raises(ValueError, match='seed'):
        ins.relax_lines(states=ok, uniforms=u, seed=1)
    with pytest.raises(ValueError, match='seed'):
        ins.relax_lines(states=ok, seed=-1)
    with pytest.raises(ValueError, match='sweeps'):
        ins.relax_lines(states=ok, sweeps=None)                                    # until nothing moves: quench only
    for sweeps in (-1, 1.5):
        with pytest.raises(ValueError, match='sweeps'):
            ins.relax_lines(states=ok, sweeps=sweeps)
    for beta in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match='beta'):
            ins.relax_lines(states=ok, beta=beta)
    with pytest.raises(ValueError, match='max_sweeps'):
        ins.relax_lines(states=ok, mode='quench', sweeps=None, max_sweeps=0)
    bad_one = u.copy()
    bad_one[0, 1, 4, 2] = 1.0
    for bad in (u[:, :1], u[..., :4], u.astype(np.float32), bad_one, np.full_like(u, np.nan)):
        with pytest.raises(ValueError, match='uniforms'):
            ins.relax_lines(states=ok, uniforms=bad)
    with pytest.raises(ValueError, match='uniforms'):
        ins.relax_lines(states=ok, lines='rows', uniforms=u)                       # two passes of numbers for one pass
    with pytest.raises(ValueError, match='uniforms'):
        ins.relax_lines(states=ok, sweeps=2, uniforms=u)
    # the range guard: beta x (max - min) of a chain table above 300
    r = lines.chain_range(ins, 'both')
    assert r > 0 and lines.chain_range(ins, 'rows') <= r and lines.chain_range(ins, 'columns') <= r
    with pytest.raises(ValueError, match='range guard'):
        ins.relax_lines(states=ok, beta=301.0 / r, seed=1)
    lines.check_range_guard(ins, 'both', 299.0 / r)
    with pytest.raises(AssertionError, match='device work'):
        ins.relax_lines(states=ok, mode='quench', beta=1e6 / r)                    # the quench has no such limit
    b = ok.copy()
    b[3, 4] = 2                                                                    # model cell 4 holds the inactive spin: two states
    with pytest.raises(ValueError, match=r'states\[3, 4\]'):
        ins.relax_lines(states=b)
    with pytest.raises(ValueError):
        ins.relax_lines()                                                          # no stored states
    with pytest.raises(ValueError, match='chunk'):
        ins.relax_lines(states=ok, chunk=0)
    assert not hasattr(ins, 'relax_moves') and ins.states.shape[0] == 0
