"""Host reference of tn_line_sweep / tnac4o.relax_lines (numpy, no GPU).  Lattices, make_cells, total_energy, boltzmann, law_statistic
and configuration_index are those of relax_ref.

With the rows above and below given, one lattice row is a chain of cells: side energy a_x(s) = ((1.0 Es[s] + E4_x[s, U]) + B.E4[sb,
B.up_map(s)]) (absent terms absent), coupling E1_x[s_x, r_{x-1}(s_{x-1})] with r_{x-1}(s') = left_map_x ? left_map_x[s'] : s'.
- heat_row: forward filtering (lambda_x, column messages F_x normalised to a largest entry of 1), backward sampling, every draw by
  draw_weights -- relax_ref.heat_bath_draw's rule on given weights -- with its margin.
- quench_row: the same recursion in (min, +); the line moves to the minimiser that is smallest in the order (s_{Nx-1}, ..., s_0) when the
  minimum lies strictly below the line's energy; gap = the smallest difference between the best and the runner-up of any decision.
- A column pass is the row pass on the transposed lattice (transpose).  row_pass / column_pass / sweep / run: a pass (even lines, then
  odd lines), a sweep under lines = 'rows' | 'columns' | 'both', a whole call.
- line_law: the probability the recursion gives every configuration of one line; line_conditional: the same by enumeration.
- sweep_matrix: the exact one-sweep transition matrix from ENUMERATED line conditionals (not from the recursion).
- brute_line_minimum: the line minimum and its tie rule by enumeration.
- CASES: relax_ref's, with uniforms of shape (HEAT_SWEEPS, 2, ncell, M) for lines = 'both'.
"""
import functools
import itertools

import numpy as np

import relax_ref as rr

LINES = {'rows': 0, 'columns': 1, 'both': 2}
PASSES = {'rows': ('rows',), 'columns': ('columns',), 'both': ('rows', 'columns')}


# ---------------------------------------------------------------------------------------------- the chain of one row
def transpose(cells, Nx, Ny):
    """(cells of the transposed lattice -- Nx rows of Ny cells, E1 <-> E4 and left_map <-> up_map exchanged --, perm with perm[kT] = k)."""
    out, perm = [], []
    for nx in range(Nx):
        for ny in range(Ny):
            c = cells[ny * Nx + nx]
            out.append(dict(q=c['q'], Es=c['Es'], E1=c['E4'], E4=c['E1'], left_map=c['up_map'], up_map=c['left_map']))
            perm.append(ny * Nx + nx)
    return out, np.array(perm, dtype=np.int64)


def side_energy(cells, Nx, Ny, states, k):
    """a (M, q) of cell k: ((1.0 Es[s] + E4[s, U]) + B.E4[sb, B.up_map(s)]), a term absent at a lattice edge."""
    ny, nx = divmod(k, Nx)
    c = cells[k]
    q = c['q']
    s = np.arange(q)
    M = states.shape[0]
    e = np.broadcast_to(1.0 * np.asarray(c['Es'], dtype=np.float64)[None, :], (M, q))
    if ny > 0:
        su = rr._inside(states[:, k - Nx], cells[k - Nx]['q'])
        U = c['up_map'][su] if c['up_map'] is not None else su
        e = e + c['E4'][:, U].T
    if ny + 1 < Ny:
        B = cells[k + Nx]
        sb = rr._inside(states[:, k + Nx], B['q'])
        col = B['up_map'][s] if B['up_map'] is not None else s
        e = e + B['E4'][sb[:, None], col[None, :]]
    return np.array(e)


def chain_column(cells, k):
    """r (q of cell k,): the column of cells[k + 1].E1 every state of cell k selects."""
    nxt = cells[k + 1]
    return nxt['left_map'] if nxt['left_map'] is not None else np.arange(cells[k]['q'])


def transfer(c, beta):
    """T = exp(-beta (E1 - min E1)) of a cell right of column 0."""
    return np.exp(-beta * (c['E1'] - c['E1'].min()))


def draw_weights(w, u):
    """relax_ref.heat_bath_draw's rule on given weights w (M, q): c = cumsum(w), t = u c[-1]; the first s with c_s >= t and w_s > 0,
    otherwise the last s with w_s > 0.  (new state (M,), margin (M,) = min_s |t - c_s| / c[-1])."""
    c = np.cumsum(w, axis=1)
    W = c[:, -1]
    t = u * W
    ok = (c >= t[:, None]) & (w > 0)
    first = np.argmax(ok, axis=1)
    last = w.shape[1] - 1 - np.argmax((w > 0)[:, ::-1], axis=1)
    new = np.where(ok.any(axis=1), first, last)
    return new, np.min(np.abs(t[:, None] - c), axis=1) / W


def forward(cells, Nx, Ny, states, ny, beta):
    """lambda_x (M, q_x) for every cell of row ny."""
    lam, F = [], None
    M = states.shape[0]
    for x in range(Nx):
        k = ny * Nx + x
        a = side_energy(cells, Nx, Ny, states, k)
        w = np.exp(-beta * (a - a.min(axis=1, keepdims=True)))
        lam.append(w if x == 0 else w * (F @ transfer(cells[k], beta).T))
        if x + 1 < Nx:
            F = np.zeros((M, cells[k + 1]['E1'].shape[1]))
            np.add.at(F.T, chain_column(cells, k), (lam[-1] / lam[-1].max(axis=1, keepdims=True)).T)
    return lam


def heat_row(cells, Nx, Ny, states, ny, beta, u):
    """Row ny of every sample drawn from its conditional law given the other rows; u (ncell, M).  (new (M, Nx), margins (M, Nx))."""
    lam = forward(cells, Nx, Ny, states, ny, beta)
    M = states.shape[0]
    new = np.zeros((M, Nx), dtype=np.int64)
    margins = np.zeros((M, Nx))
    for x in range(Nx - 1, -1, -1):
        k = ny * Nx + x
        w = lam[x]
        if x + 1 < Nx:
            w = w * transfer(cells[k + 1], beta)[new[:, x + 1][:, None], chain_column(cells, k)[None, :]]
        new[:, x], margins[:, x] = draw_weights(w, u[k])
    return new, margins


def min_plus(mu, E):
    """(M, q): min_r (mu[m, r] + E[s, r]), in slices of samples."""
    M, q = mu.shape[0], E.shape[0]
    out = np.empty((M, q))
    step = max(1, (1 << 22) // max(1, E.size))
    for lo in range(0, M, step):
        out[lo:lo + step] = (mu[lo:lo + step, None, :] + E[None, :, :]).min(axis=2)
    return out


def _gap(vals):
    """The smallest difference between the least and the next value of every row of vals (inf with one column)."""
    if vals.shape[1] < 2:
        return np.inf
    two = np.partition(vals, 1, axis=1)[:, :2]
    d = two[:, 1] - two[:, 0]
    return float(np.min(d[np.isfinite(d)], initial=np.inf))


def line_energy(cells, Nx, Ny, states, ny, line):
    """c (M,) of the states `line` (M, Nx) in row ny: c_0 = a_0(s_0), c_x = a_x(s_x) + (c_{x-1} + E1_x[s_x, r]); +inf when a state lies
    outside its cell."""
    M = states.shape[0]
    rows = np.arange(M)
    c = np.zeros(M)
    bad = np.zeros(M, dtype=bool)
    for x in range(Nx):
        k = ny * Nx + x
        q = cells[k]['q']
        s = np.asarray(line[:, x], dtype=np.int64)
        bad |= (s < 0) | (s >= q)
        s = rr._inside(s, q)
        a = side_energy(cells, Nx, Ny, states, k)[rows, s]
        if x == 0:
            c = a
        else:
            r = chain_column(cells, k - 1)[rr._inside(line[:, x - 1], cells[k - 1]['q'])]
            c = a + (c + cells[k]['E1'][s, r])
    return np.where(bad, np.inf, c)


def quench_row(cells, Nx, Ny, states, ny):
    """Row ny to its conditional minimum when that lies strictly below the row's energy.  (new (M, Nx), gap)."""
    M = states.shape[0]
    Lam = []
    for x in range(Nx):
        k = ny * Nx + x
        a = side_energy(cells, Nx, Ny, states, k)
        if x == 0:
            Lam.append(a)
            continue
        E1 = cells[k]['E1']
        mu = np.full((M, E1.shape[1]), np.inf)
        np.minimum.at(mu.T, chain_column(cells, k - 1), Lam[-1].T)
        Lam.append(a + min_plus(mu, E1))
    cur = states[:, ny * Nx:(ny + 1) * Nx]
    c = line_energy(cells, Nx, Ny, states, ny, cur)
    best = np.zeros((M, Nx), dtype=np.int64)
    gap = _gap(Lam[-1])
    best[:, -1] = np.argmin(Lam[-1], axis=1)
    Estar = Lam[-1].min(axis=1)
    assert np.all(Estar <= c)
    d = c - Estar
    gap = min(gap, float(np.min(d[(d > 0) & np.isfinite(d)], initial=np.inf)))
    for x in range(Nx - 2, -1, -1):
        k = ny * Nx + x
        vals = Lam[x] + cells[k + 1]['E1'][best[:, x + 1][:, None], chain_column(cells, k)[None, :]]
        gap = min(gap, _gap(vals))
        best[:, x] = np.argmin(vals, axis=1)
    return np.where((Estar < c)[:, None], best, cur), gap


# ---------------------------------------------------------------------------------------------- passes, sweeps, calls
def row_pass(cells, Nx, Ny, states, mode, beta=None, u=None):
    """Even rows, then odd rows, in place of a copy: (new states, moved cells (M,), smallest margin, smallest gap)."""
    st = np.array(states, dtype=np.int64)
    moved = np.zeros(st.shape[0], dtype=np.int64)
    margin, gap = np.inf, np.inf
    for parity in (0, 1):
        for ny in range(parity, Ny, 2):
            if mode == 0:
                new, mg = heat_row(cells, Nx, Ny, st, ny, beta, u)
                margin = min(margin, float(mg.min()))
            else:
                new, g = quench_row(cells, Nx, Ny, st, ny)
                gap = min(gap, g)
            moved += (new != st[:, ny * Nx:(ny + 1) * Nx]).sum(axis=1)
            st[:, ny * Nx:(ny + 1) * Nx] = new
    return st, moved, margin, gap


def column_pass(cells, Nx, Ny, states, mode, beta=None, u=None):
    """The row pass of the transposed lattice."""
    cT, perm = transpose(cells, Nx, Ny)
    st, moved, margin, gap = row_pass(cT, Ny, Nx, np.asarray(states)[:, perm], mode, beta, None if u is None else u[perm])
    out = np.empty_like(st)
    out[:, perm] = st
    return out, moved, margin, gap


def sweep(cells, Nx, Ny, states, mode, lines, beta=None, u=None):
    """One sweep; u (P, ncell, M).  (new states, moves (M,), margin, gap)."""
    st = np.array(states, dtype=np.int64)
    moves = np.zeros(st.shape[0], dtype=np.int64)
    margin, gap = np.inf, np.inf
    for p, which in enumerate(PASSES[lines]):
        fn = row_pass if which == 'rows' else column_pass
        st, mv, mg, g = fn(cells, Nx, Ny, st, mode, beta, None if u is None else u[p])
        moves += mv
        margin, gap = min(margin, mg), min(gap, g)
    return st, moves, margin, gap


def run(cells, Nx, Ny, states, mode, sweeps, lines='both', beta=None, uniforms=None):
    """A whole call: dict(states, energy, moves, last_moves, margin (inf without a draw), gap (inf without a decision), energies
    (sweeps + 1, M)); uniforms (sweeps, P, ncell, M)."""
    st = np.array(states, dtype=np.int64)
    moves = np.zeros(st.shape[0], dtype=np.int64)
    last = np.zeros(st.shape[0], dtype=np.int64)
    margin, gap = np.inf, np.inf
    energies = [rr.total_energy(cells, Nx, Ny, st)]
    for j in range(sweeps):
        st, last, mg, g = sweep(cells, Nx, Ny, st, mode, lines, beta, None if uniforms is None else uniforms[j])
        moves += last
        margin, gap = min(margin, mg), min(gap, g)
        energies.append(rr.total_energy(cells, Nx, Ny, st))
    return dict(states=st, energy=energies[-1], moves=moves, last_moves=last, margin=margin, gap=gap, energies=np.stack(energies))


def chain_ranges(cells, Nx, Ny, lines):
    """The largest max - min of a chain table the passes of `lines` read (E1 for rows, E4 for columns); 0 without one."""
    r = 0.0
    for k, c in enumerate(cells):
        ny, nx = divmod(k, Nx)
        if lines in ('rows', 'both') and nx > 0:
            r = max(r, float(c['E1'].max() - c['E1'].min()))
        if lines in ('columns', 'both') and ny > 0:
            r = max(r, float(c['E4'].max() - c['E4'].min()))
    return r


# ---------------------------------------------------------------------------------------------- exact laws by enumeration
def line_law(cells, Nx, Ny, state, ny, beta):
    """(line configurations (n, Nx), their probability under the recursion (n,)) for row ny of ONE configuration `state` (ncell,)."""
    st = np.asarray(state, dtype=np.int64)[None, :]
    lam = forward(cells, Nx, Ny, st, ny, beta)
    X = np.array(list(itertools.product(*[range(cells[ny * Nx + x]['q']) for x in range(Nx)])), dtype=np.int64)
    p = np.empty(X.shape[0])
    for i, line in enumerate(X):
        w = lam[-1][0]
        pr = w[line[-1]] / w.sum()
        for x in range(Nx - 2, -1, -1):
            k = ny * Nx + x
            w = lam[x][0] * transfer(cells[k + 1], beta)[line[x + 1], chain_column(cells, k)]
            pr = pr * w[line[x]] / w.sum()
        p[i] = pr
    return X, p


def line_conditional(cells, Nx, Ny, state, ny, beta):
    """The same law by enumeration: the Boltzmann weights of the whole configurations with row ny replaced."""
    X = np.array(list(itertools.product(*[range(cells[ny * Nx + x]['q']) for x in range(Nx)])), dtype=np.int64)
    full = np.repeat(np.asarray(state, dtype=np.int64)[None, :], X.shape[0], axis=0)
    full[:, ny * Nx:(ny + 1) * Nx] = X
    E = rr.total_energy(cells, Nx, Ny, full)
    w = np.exp(-beta * (E - E.min()))
    return X, w / w.sum()


def _line_matrix(cells, Nx, Ny, beta, X, radix, ks):
    """The transition matrix of resampling the cells ks jointly from their enumerated conditional law."""
    n = X.shape[0]
    base = X @ radix
    choices = list(itertools.product(*[range(cells[k]['q']) for k in ks]))
    E = np.empty((n, len(choices)))
    tgt = np.empty((n, len(choices)), dtype=np.int64)
    for j, choice in enumerate(choices):
        Y = X.copy()
        t = base.copy()
        for k, s in zip(ks, choice):
            Y[:, k] = s
            t = t + (s - X[:, k]) * radix[k]
        E[:, j] = rr.total_energy(cells, Nx, Ny, Y)
        tgt[:, j] = t
    w = np.exp(-beta * (E - E.min(axis=1, keepdims=True)))
    w = w / w.sum(axis=1, keepdims=True)
    P = np.zeros((n, n))
    np.add.at(P, (np.repeat(np.arange(n), len(choices)), tgt.ravel()), w.ravel())
    return P


def sweep_matrix(cells, Nx, Ny, beta, lines):
    """P (n x n) of one sweep in the order of relax_ref.all_configurations, from enumerated line conditionals."""
    X = rr.all_configurations(cells)
    qs = np.array([c['q'] for c in cells])
    radix = np.concatenate([np.cumprod(qs[::-1])[::-1][1:], [1]])
    P = np.eye(X.shape[0])
    for which in PASSES[lines]:
        for parity in (0, 1):
            if which == 'rows':
                groups = [[ny * Nx + x for x in range(Nx)] for ny in range(parity, Ny, 2)]
            else:
                groups = [[y * Nx + nx for y in range(Ny)] for nx in range(parity, Nx, 2)]
            for ks in groups:
                P = P @ _line_matrix(cells, Nx, Ny, beta, X, radix, ks)
    return P


def brute_line_minimum(cells, Nx, Ny, state, ny):
    """Row ny of ONE configuration by enumeration: (new line (Nx,), E*, c): the minimiser smallest in the order (s_{Nx-1}, ..., s_0) when
    E* < c strictly, else the line as it stands."""
    st = np.asarray(state, dtype=np.int64)
    X = np.array(list(itertools.product(*[range(cells[ny * Nx + x]['q']) for x in range(Nx)])), dtype=np.int64)
    full = np.repeat(st[None, :], X.shape[0], axis=0)
    E = line_energy(cells, Nx, Ny, full, ny, X)
    cur = st[ny * Nx:(ny + 1) * Nx]
    c = float(line_energy(cells, Nx, Ny, st[None, :], ny, cur[None, :])[0])
    ties = X[E == E.min()]
    best = ties[np.lexsort(ties.T)[0]]                       # lexsort: the LAST key (s_{Nx-1}) is the primary one
    return (best if E.min() < c else cur), float(E.min()), c


# ---------------------------------------------------------------------------------------------- seeded inputs
BETA = rr.BETA
HEAT_SWEEPS, QUENCH_SWEEPS = rr.HEAT_SWEEPS, rr.QUENCH_SWEEPS
CASES = list(rr.CASES)
CASE_IDS = ['%s-%s-M%d%s' % (c[0], 'maps' if c[1] else 'nomaps', c[2], '-int' if c[4] else '') for c in CASES]
MARGIN_FLOOR = 1e-9


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(Ny, Nx, cells, states (M, ncell), uniforms (HEAT_SWEEPS, 2, ncell, M)): relax_ref's lattice and states, uniforms from seed + 2."""
    Ny, Nx, cells, states, _ = rr.case_inputs(case)
    M, ncell = states.shape
    uniforms = np.random.default_rng(case[3] + 2).random((HEAT_SWEEPS, 2, ncell, M))
    uniforms.setflags(write=False)
    return Ny, Nx, cells, states, uniforms


@functools.lru_cache(maxsize=None)
def case_reference(case, mode, lines='both'):
    """run() of a case (heat bath: mode 0, quench: mode 1); computed once and shared.  lines != 'both' uses pass 0 of the uniforms."""
    Ny, Nx, cells, states, uniforms = case_inputs(case)
    if mode == 0:
        u = uniforms if lines == 'both' else uniforms[:, :1]
        return run(cells, Nx, Ny, states, 0, HEAT_SWEEPS, lines, BETA, u)
    return run(cells, Nx, Ny, states, 1, QUENCH_SWEEPS, lines)


# a heat bath whose beta x (range of a chain table) lies between 200 and 300: 2 x 3 lattice, small cells, real tables
STEEP_SEED, STEEP_M = 501, 65


@functools.lru_cache(maxsize=None)
def steep_inputs():
    """(Ny, Nx, cells, beta, states, uniforms (1, 2, ncell, M)); beta = 250 / the largest chain-table range."""
    Ny, Nx, qs = 2, 3, [5, 70, 6, 9, 4, 300]
    cells = rr.make_cells(Ny, Nx, qs, False, STEEP_SEED)
    beta = 250.0 / chain_ranges(cells, Nx, Ny, 'both')
    rng = np.random.default_rng(STEEP_SEED + 1)
    states = rng.integers(0, np.asarray(qs)[None, :], size=(STEEP_M, len(qs)))
    uniforms = rng.random((1, 2, len(qs), STEEP_M))
    return Ny, Nx, cells, beta, states, uniforms


LAW_M, LAW_SEED = 2 ** 14, 199


@functools.lru_cache(maxsize=None)
def law_inputs():
    """(cells, beta, states (LAW_M, 4) uniformly random, uniforms (2, 2, 4, LAW_M), exact law after one 'rows' sweep, after two 'both'
    sweeps) on relax_ref.law_problem()."""
    cells, beta = rr.law_problem()
    rng = np.random.default_rng(LAW_SEED)
    states = rng.integers(0, 4, size=(LAW_M, 4))
    uniforms = rng.random((2, 2, 4, LAW_M))
    mu0 = np.full(256, 1.0 / 256)
    law_rows = mu0 @ sweep_matrix(cells, 2, 2, beta, 'rows')
    law_both = mu0 @ np.linalg.matrix_power(sweep_matrix(cells, 2, 2, beta, 'both'), 2)
    return cells, beta, states, uniforms, law_rows, law_both
