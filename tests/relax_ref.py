"""Host reference of tn_cell_sweep / tnac4o.relax_samples (numpy, no GPU).

A lattice is a list of cells in walk order (cell ny * Nx + nx), each a dict with q, Es (q), E1 (q x e1cols) or None in column 0,
E4 (q x e4cols) or None in row 0, left_map / up_map (int64 over the states of the left / upper neighbour) or None.

- cond_energy: the conditional energy of every state of a cell, for all samples, with the additions of include/tnpeps.h in their order.
- colour_step / sweep / run: one colour, one sweep, a whole call in both modes; run also returns the margin of every heat-bath draw,
  min_s |t - c_s| / W with c = np.cumsum in index order: how far the draw is from a boundary that another summation order could move.
- total_energy: the energy tn_gibbs_score's energy_out adds up.
- sweep_matrix: the exact one-sweep transition matrix of a lattice small enough to enumerate, and boltzmann of the same lattice.
- law_statistic: the pooled-bin test of empirical frequencies against an exact law.
- CASES: the seeded inputs shared by the host and the GPU tests.
"""
import functools
import itertools

import numpy as np


# ---------------------------------------------------------------------------------------------- the move
def _inside(s, q):
    """States outside [0, q) are read as 0."""
    s = np.asarray(s, dtype=np.int64)
    return np.where((s >= 0) & (s < q), s, 0)


def cond_energy(cells, Nx, Ny, states, k):
    """e (M, q): e[m, s] = energy of cell k in state s given the neighbours of sample m,
    (((1.0 Es[s] + E1[s, L]) + E4[s, U]) + R.E1[sr, R.left_map(s)]) + Bc.E4[sb, Bc.up_map(s)], absent terms absent."""
    ny, nx = divmod(k, Nx)
    c = cells[k]
    q = c['q']
    s = np.arange(q)
    M = states.shape[0]
    e = np.broadcast_to(1.0 * np.asarray(c['Es'], dtype=np.float64)[None, :], (M, q))
    if nx > 0:
        sl = _inside(states[:, k - 1], cells[k - 1]['q'])
        L = c['left_map'][sl] if c['left_map'] is not None else sl
        e = e + c['E1'][:, L].T
    if ny > 0:
        su = _inside(states[:, k - Nx], cells[k - Nx]['q'])
        U = c['up_map'][su] if c['up_map'] is not None else su
        e = e + c['E4'][:, U].T
    if nx + 1 < Nx:
        R = cells[k + 1]
        sr = _inside(states[:, k + 1], R['q'])
        col = R['left_map'][s] if R['left_map'] is not None else s
        e = e + R['E1'][sr[:, None], col[None, :]]
    if ny + 1 < Ny:
        B = cells[k + Nx]
        sb = _inside(states[:, k + Nx], B['q'])
        col = B['up_map'][s] if B['up_map'] is not None else s
        e = e + B['E4'][sb[:, None], col[None, :]]
    return np.array(e)


def heat_bath_draw(e, beta, u):
    """(new state (M,), margin (M,)) of the draw rule: w = exp(-beta (e - min e)), c = cumsum(w), t = u c[-1]; the first s with c_s >= t
    and w_s > 0, otherwise the last s with w_s > 0."""
    w = np.exp(-beta * (e - e.min(axis=1, keepdims=True)))
    c = np.cumsum(w, axis=1)
    W = c[:, -1]
    t = u * W
    ok = (c >= t[:, None]) & (w > 0)
    first = np.argmax(ok, axis=1)
    last = e.shape[1] - 1 - np.argmax((w > 0)[:, ::-1], axis=1)
    new = np.where(ok.any(axis=1), first, last)
    margin = np.min(np.abs(t[:, None] - c), axis=1) / W
    return new, margin


def quench_choice(e, cur):
    """The smallest state attaining min e when that minimum lies strictly below e[current] (+inf for a current state outside the
    cell), otherwise the current state."""
    q = e.shape[1]
    cur = np.asarray(cur, dtype=np.int64)
    inside = (cur >= 0) & (cur < q)
    ecur = np.where(inside, e[np.arange(e.shape[0]), np.where(inside, cur, 0)], np.inf)
    emin = e.min(axis=1)
    return np.where(emin < ecur, np.argmin(e, axis=1), cur)


def colour_step(cells, Nx, Ny, states, colour, mode, beta=None, u=None):
    """All cells of one colour from the states as they stand: (new states, changed (M,) count, margins (M, cells of the colour))."""
    new = states.copy()
    moved = np.zeros(states.shape[0], dtype=np.int64)
    margins = []
    for k in range(Nx * Ny):
        ny, nx = divmod(k, Nx)
        if (ny + nx) % 2 != colour:
            continue
        e = cond_energy(cells, Nx, Ny, states, k)
        if mode == 0:
            s, mg = heat_bath_draw(e, beta, u[k])
            margins.append(mg)
        else:
            s = quench_choice(e, states[:, k])
        moved += s != states[:, k]
        new[:, k] = s
    return new, moved, (np.stack(margins, axis=1) if margins else np.zeros((states.shape[0], 0)))


def sweep(cells, Nx, Ny, states, mode, beta=None, u=None):
    """Colour 0, then colour 1: (new states, moves (M,), margins (M, Nx*Ny) -- empty for a quench)."""
    s0, m0, g0 = colour_step(cells, Nx, Ny, states, 0, mode, beta, u)
    s1, m1, g1 = colour_step(cells, Nx, Ny, s0, 1, mode, beta, u)
    return s1, m0 + m1, np.concatenate([g0, g1], axis=1)


def total_energy(cells, Nx, Ny, states):
    """Cell by cell in walk order, E = E + ((1.0 Es[s] + E1[s, L]) + E4[s, U]): the additions of the walks' energy_out."""
    st = np.stack([_inside(states[:, k], cells[k]['q']) for k in range(Nx * Ny)], axis=1)
    E = np.zeros(st.shape[0])
    for k in range(Nx * Ny):
        ny, nx = divmod(k, Nx)
        c = cells[k]
        dE = 1.0 * np.asarray(c['Es'], dtype=np.float64)[st[:, k]]
        if nx > 0:
            sl = st[:, k - 1]
            dE = dE + c['E1'][st[:, k], c['left_map'][sl] if c['left_map'] is not None else sl]
        if ny > 0:
            su = st[:, k - Nx]
            dE = dE + c['E4'][st[:, k], c['up_map'][su] if c['up_map'] is not None else su]
        E = E + dE
    return E


def run(cells, Nx, Ny, states, mode, sweeps, beta=None, uniforms=None):
    """A whole call: dict(states, energy, moves, last_moves, margin = the smallest margin of any draw (inf without one), energies =
    the energy after every sweep (sweeps + 1, M))."""
    st = np.array(states, dtype=np.int64)
    moves = np.zeros(st.shape[0], dtype=np.int64)
    last = np.zeros(st.shape[0], dtype=np.int64)
    margin = np.inf
    energies = [total_energy(cells, Nx, Ny, st)]
    for j in range(sweeps):
        st, last, mg = sweep(cells, Nx, Ny, st, mode, beta, None if uniforms is None else uniforms[j])
        moves += last
        if mg.size:
            margin = min(margin, float(mg.min()))
        energies.append(total_energy(cells, Nx, Ny, st))
    return dict(states=st, energy=energies[-1], moves=moves, last_moves=last, margin=margin, energies=np.stack(energies))


# ---------------------------------------------------------------------------------------------- exact law of a small lattice
def all_configurations(cells):
    return np.array(list(itertools.product(*[range(c['q']) for c in cells])), dtype=np.int64)


def boltzmann(cells, Nx, Ny, beta):
    """(configurations (n, Nx*Ny), pi (n,)) by enumeration."""
    X = all_configurations(cells)
    E = total_energy(cells, Nx, Ny, X)
    w = np.exp(-beta * (E - E.min()))
    return X, w / w.sum()


def sweep_matrix(cells, Nx, Ny, beta):
    """P (n x n), row = configuration before a heat-bath sweep, column = after, in the order of all_configurations: the product of the
    two colour steps, each the product over its cells of w_s / W."""
    X = all_configurations(cells)
    n = X.shape[0]
    qs = np.array([c['q'] for c in cells])
    radix = np.concatenate([np.cumprod(qs[::-1])[::-1][1:], [1]])
    P = np.eye(n)
    for colour in (0, 1):
        ks = [k for k in range(Nx * Ny) if sum(divmod(k, Nx)) % 2 == colour]
        probs = {}
        for k in ks:
            e = cond_energy(cells, Nx, Ny, X, k)
            w = np.exp(-beta * (e - e.min(axis=1, keepdims=True)))
            probs[k] = w / w.sum(axis=1, keepdims=True)
        Pc = np.zeros((n, n))
        base = X @ radix
        for choice in itertools.product(*[range(qs[k]) for k in ks]):
            p = np.ones(n)
            tgt = base.copy()
            for k, s in zip(ks, choice):
                p = p * probs[k][:, s]
                tgt = tgt + (s - X[:, k]) * radix[k]
            Pc[np.arange(n), tgt] += p
        P = P @ Pc
    return P


def law_statistic(index, p, pool_below=20.0, sigmas=6.0):
    """Empirical frequencies of the configuration indices `index` (M,) against the exact law p: the bins with M p < pool_below are
    pooled into one; returns (passes, the largest |f - p| / sqrt(p (1 - p) / M) over the bins, their number).  Passes when every bin
    lies within `sigmas` standard deviations."""
    M = index.size
    counts = np.bincount(index, minlength=p.size).astype(np.float64)
    small = M * p < pool_below
    pp = np.concatenate([p[~small], [p[small].sum()]]) if small.any() else p
    ff = np.concatenate([counts[~small], [counts[small].sum()]]) / M if small.any() else counts / M
    keep = pp > 0
    z = np.abs(ff[keep] - pp[keep]) / np.sqrt(pp[keep] * (1.0 - pp[keep]) / M)
    ok = bool(np.all(z <= sigmas)) and bool(np.all(ff[~keep] == 0))
    return ok, float(z.max()), int(pp.size)


# ---------------------------------------------------------------------------------------------- seeded inputs
def make_cells(Ny, Nx, qs, maps, seed, integer=False):
    """Random real tables (integer: small integers, so that conditional energies tie).  maps: Ising-style left_map / up_map into few
    columns; otherwise the neighbour's state is the column and the tables have one spare column (e1cols, e4cols != q)."""
    rng = np.random.default_rng(seed)

    def table(*shape):
        return rng.integers(-2, 3, shape).astype(np.float64) if integer else rng.normal(0.0, 1.0, shape)

    cells = []
    for k, q in enumerate(qs):
        ny, nx = divmod(k, Nx)
        c = dict(q=int(q), Es=table(q), E1=None, E4=None, left_map=None, up_map=None)
        if nx > 0:
            ql = int(qs[k - 1])
            cols = 2 + k % 4 if maps else ql + 1 + (ql + 1 == q)
            c['E1'] = table(q, cols)
            c['left_map'] = rng.integers(0, cols, ql).astype(np.int64) if maps else None
        if ny > 0:
            qu = int(qs[k - Nx])
            cols = 2 + (k + 1) % 3 if maps else qu + 1 + (qu + 1 == q)
            c['E4'] = table(q, cols)
            c['up_map'] = rng.integers(0, cols, qu).astype(np.int64) if maps else None
        cells.append(c)
    return cells


LATTICES = {                                 # name -> (Ny, Nx, q of every cell in walk order)
    '1x1': (1, 1, [100]),
    '1x3': (1, 3, [1, 256, 3]),
    '3x1': (3, 1, [64, 1500, 100]),
    '3x3': (3, 3, [3, 256, 100, 1500, 64, 1, 256, 3, 1500]),
    '2x2': (2, 2, [100, 64, 1500, 256]),
}
BETA = 0.9
HEAT_SWEEPS, QUENCH_SWEEPS = 2, 3
# (lattice, maps, M, seed, integer tables); a seed whose margin falls below 1e-9 (tests/test_relax_host.py) is replaced, never excused
CASES = [(name, maps, M, 1000 + 37 * i + 11 * j + int(maps), False)
         for i, name in enumerate(LATTICES) for maps in (True, False) for j, M in enumerate((1, 65, 300))]
CASES.append(('2x2', True, 65, 7, True))


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(Ny, Nx, cells, states (M, ncell) int64, uniforms (HEAT_SWEEPS, ncell, M)) of a case; computed once, never modified."""
    name, maps, M, seed, integer = case
    Ny, Nx, qs = LATTICES[name]
    cells = make_cells(Ny, Nx, qs, maps, seed, integer)
    rng = np.random.default_rng(seed + 1)
    states = rng.integers(0, np.asarray(qs)[None, :], size=(M, len(qs)))
    uniforms = rng.random((HEAT_SWEEPS, len(qs), M))
    for a in (states, uniforms):
        a.setflags(write=False)
    return Ny, Nx, cells, states, uniforms


@functools.lru_cache(maxsize=None)
def case_reference(case, mode):
    """run() of a case in heat-bath (0) or quench (1) mode; computed once and shared."""
    Ny, Nx, cells, states, uniforms = case_inputs(case)
    if mode == 0:
        return run(cells, Nx, Ny, states, 0, HEAT_SWEEPS, BETA, uniforms)
    return run(cells, Nx, Ny, states, 1, QUENCH_SWEEPS)


def law_problem():
    """The 2 x 2 lattice of q = 4 cells with random real couplings at beta = 0.7 of the invariance and law tests: (cells, beta)."""
    return make_cells(2, 2, [4, 4, 4, 4], False, 4242), 0.7


LAW_M, LAW_SWEEPS, LAW_SEED = 2 ** 14, 5, 99


@functools.lru_cache(maxsize=None)
def law_inputs():
    """(cells, beta, states (LAW_M, 4) uniformly random, uniforms (LAW_SWEEPS, 4, LAW_M), exact law mu0 P^5 (256,))."""
    cells, beta = law_problem()
    rng = np.random.default_rng(LAW_SEED)
    states = rng.integers(0, 4, size=(LAW_M, 4))
    uniforms = rng.random((LAW_SWEEPS, 4, LAW_M))
    P = sweep_matrix(cells, 2, 2, beta)
    law = np.full(256, 1.0 / 256) @ np.linalg.matrix_power(P, LAW_SWEEPS)
    return cells, beta, states, uniforms, law


def configuration_index(states, q=4):
    """Index of (M, n) states in the order of all_configurations (first cell slowest)."""
    n = states.shape[1]
    return np.asarray(states, dtype=np.int64) @ (q ** np.arange(n - 1, -1, -1))
