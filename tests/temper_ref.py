"""Host reference of tn_temper / tnac4o.temper_samples (numpy, no GPU): a whole call composed of relax_ref.sweep per temperature group,
exchange_ref.move on the packed spin bits, relax_ref.total_energy and the swap rule of include/tnpeps.h (K12).

- to_bits / from_bits: the conversion between cell states and packed rows through cellbits / bitcell.
- run: one call; besides the outputs it returns the smallest draw margin, the smallest swap margin |u - exp(D)| over the decisions with
  D < 0, and E_a + E_b of every row pair before and after its cluster move.
- ising_lattice: the synthetic Ising lattice (b) with its bit tables and CSR; case_inputs / case_reference: the shared inputs.
- joint_round / law_inputs: the exact joint law of one chain of two temperatures on relax_ref.law_problem().
"""
import functools

import numpy as np

import exchange_ref as xr
import relax_ref as rr


# ---------------------------------------------------------------------------------------------- bits
def to_bits(cells, states, nbits, bitcell):
    """Rows as Python integers: bit p = 1 - bit j of the state of cell k, (k, j) = bitcell[p]; a state outside its cell is read as 0;
    an entry of bitcell out of range leaves the bit 0."""
    ncell = len(cells)
    rows = []
    for m in range(states.shape[0]):
        v = 0
        for p in range(nbits):
            k, j = int(bitcell[p, 0]), int(bitcell[p, 1])
            if not (0 <= k < ncell and 0 <= j < 15):
                continue
            s = int(rr._inside(states[m, k], cells[k]['q']))
            v |= (1 - ((s >> j) & 1)) << p
        rows.append(v)
    return rows


def from_bits(cells, states, rows, nbits, cellbits):
    """The states the rows give: bit j of cell k = 1 - row bit cellbits[k, j] (a position outside [0, nbits) is skipped); a cell is
    written only where that differs from what it was read as."""
    new = states.copy()
    for m in range(states.shape[0]):
        for k in range(len(cells)):
            old = int(rr._inside(states[m, k], cells[k]['q']))
            s = old
            for j in range(cellbits.shape[1]):
                p = int(cellbits[k, j])
                if 0 <= p < nbits:
                    s = (s & ~(1 << j)) | ((1 - ((rows[m] >> p) & 1)) << j)
            if s != old:
                new[m, k] = s
    return new


# ---------------------------------------------------------------------------------------------- a whole call
def run(cells, Nx, Ny, states, betas, tidx, slot, round0, rounds, sweeps, usweep=None, bits=None, cluster_from=0, cpairs=None, ucl=None,
        uswap=None, accepted=None, attempted=None):
    """tn_temper.  states (M, ncell); tidx (M,); slot (R, T); usweep (rounds, sweeps, ncell, M); bits: None or (nbits, cellbits,
    bitcell, rowptr, cols); cpairs (rounds, Pc, 2); ucl (rounds, Tc, Pc); uswap (rounds, R, T - 1); accepted / attempted (T - 1,) are
    added to.  Returns a dict: states, tidx, slot, energy, energy_trace, tidx_trace (rounds, M), accepted, attempted, sizes, differing
    (rounds, Tc, Pc), margin, swap_margin, pair_sums = [(E_a + E_b before, after)] of every cluster move."""
    betas = np.asarray(betas, dtype=np.float64)
    st = np.array(states, dtype=np.int64)
    M, T = st.shape[0], betas.size
    R = M // T
    tidx, slot = np.array(tidx, dtype=np.int64), np.array(slot, dtype=np.int64).reshape(R, T)
    acc = np.zeros(max(T - 1, 0), dtype=np.int64) if accepted is None else np.array(accepted, dtype=np.int64)
    att = np.zeros(max(T - 1, 0), dtype=np.int64) if attempted is None else np.array(attempted, dtype=np.int64)
    Tc = T - cluster_from if bits is not None else 0
    Pc = 0 if (bits is None or cpairs is None) else np.asarray(cpairs).shape[1]
    sizes, differing = np.zeros((rounds, Tc, Pc), dtype=np.int64), np.zeros((rounds, Tc, Pc), dtype=np.int64)
    etrace, ttrace = np.zeros((rounds, M)), np.zeros((rounds, M), dtype=np.int64)
    margin, swap_margin, pair_sums = np.inf, np.inf, []
    for r in range(rounds):
        for j in range(sweeps):
            new = st.copy()
            for t in range(T):
                rows = np.flatnonzero(tidx == t)
                if rows.size:
                    s, _, mg = rr.sweep(cells, Nx, Ny, st[rows], 0, betas[t], usweep[r, j][:, rows])
                    new[rows] = s
                    if mg.size:
                        margin = min(margin, float(mg.min()))
            st = new
        if bits is not None and Tc * Pc > 0:
            nbits, cellbits, bitcell, rowptr, cols = bits
            packed = to_bits(cells, st, nbits, bitcell)
            before = rr.total_energy(cells, Nx, Ny, st)
            moved = []
            for tt in range(Tc):
                for p in range(Pc):
                    ca, cb = int(cpairs[r, p, 0]), int(cpairs[r, p, 1])
                    a, b = int(slot[ca, cluster_from + tt]), int(slot[cb, cluster_from + tt])
                    packed[a], packed[b], sizes[r, tt, p], differing[r, tt, p] = xr.move(packed[a], packed[b], ucl[r, tt, p], nbits, rowptr, cols)
                    moved.append((a, b))
            st = from_bits(cells, st, packed, nbits, cellbits)
            after = rr.total_energy(cells, Nx, Ny, st)
            pair_sums += [(before[a] + before[b], after[a] + after[b]) for a, b in moved]
        E = rr.total_energy(cells, Nx, Ny, st)
        par = (round0 + r) & 1
        for c in range(R):
            for t in range(par, T - 1, 2):
                a, b = int(slot[c, t]), int(slot[c, t + 1])
                att[t] += 1
                db = betas[t + 1] - betas[t]
                dE = E[b] - E[a]
                delta = db * dE
                ok = bool(delta >= 0.0)
                if not ok and not np.isnan(delta):
                    x = float(np.exp(delta))
                    swap_margin = min(swap_margin, abs(float(uswap[r, c, t]) - x))
                    ok = bool(uswap[r, c, t] < x)
                if ok:
                    slot[c, t], slot[c, t + 1] = b, a
                    tidx[a], tidx[b] = t + 1, t
                    acc[t] += 1
        etrace[r], ttrace[r] = E, tidx
    return dict(states=st, tidx=tidx, slot=slot, energy=rr.total_energy(cells, Nx, Ny, st), energy_trace=etrace, tidx_trace=ttrace,
                accepted=acc, attempted=att, sizes=sizes, differing=differing, margin=margin, swap_margin=swap_margin, pair_sums=pair_sums)


def fresh_assignment(M, T):
    """(tidx (M,), slot (R, T)) of a fresh run: row m at temperature m % T."""
    return np.arange(M) % T, np.arange(M).reshape(M // T, T)


def assignment_consistent(tidx, slot):
    """slot[c] is a permutation of the rows of chain c and slot[c][tidx[m]] == m."""
    R, T = slot.shape
    rows = np.arange(R * T)
    return bool(np.array_equal(np.sort(slot, axis=1), rows.reshape(R, T)) and np.array_equal(slot[rows // T, tidx], rows))


# ---------------------------------------------------------------------------------------------- the synthetic Ising lattice (b)
SPINS = (1, 3, 5, 8)


@functools.lru_cache(maxsize=None)
def ising_lattice(seed=31):
    """4 x 4 cells of 1, 3, 5, 8 spins cycling (68 spins; q = 2, 8, 32, 256: three sweep classes), integer couplings inside the cells and
    between adjacent cells, integer fields; s_i = +1 for state bit 0.  The right (lower) neighbour couples to the first min(n, 2)
    spins of a cell: left_map / up_map = the state's low bits.  Returns dict(cells, Nx, Ny, nbits, cellbits (16, 8), bitcell (68, 2),
    rowptr, cols, J (68 x 68 upper triangle), h)."""
    rng = np.random.default_rng(seed)
    Nx = Ny = 4
    n = [SPINS[k % 4] for k in range(16)]
    off = np.concatenate([[0], np.cumsum(n)])
    N = int(off[-1])
    J, h = np.zeros((N, N), dtype=np.int64), rng.integers(-2, 3, N)

    def nz(shape):
        return rng.choice([-2, -1, 1, 2], shape)

    for k in range(16):
        for i in range(n[k]):
            for j in range(i + 1, n[k]):
                J[off[k] + i, off[k] + j] = nz(())
    link = lambda k: min(n[k], 2)                                        # noqa: E731  spins of cell k its right / lower neighbour sees
    for k in range(16):
        ny, nx = divmod(k, Nx)
        for other in ([k + 1] if nx + 1 < Nx else []) + ([k + Nx] if ny + 1 < Ny else []):
            J[off[k]:off[k] + link(k), off[other]:off[other] + n[other]] = nz((link(k), n[other]))

    def spins(k, s):
        return 1 - 2 * ((np.asarray(s)[..., None] >> np.arange(n[k])) & 1)           # (..., n_k) of +-1

    cells = []
    for k in range(16):
        ny, nx = divmod(k, Nx)
        q = 1 << n[k]
        sk = spins(k, np.arange(q))
        blk = J[off[k]:off[k + 1], off[k]:off[k + 1]]
        c = dict(q=q, Es=(np.einsum('si,ij,sj->s', sk, blk, sk) + sk @ h[off[k]:off[k + 1]]).astype(np.float64), E1=None, E4=None,
                 left_map=None, up_map=None)
        for name, mp, other in (('E1', 'left_map', k - 1 if nx > 0 else None), ('E4', 'up_map', k - Nx if ny > 0 else None)):
            if other is None:
                continue
            nl = link(other)
            so = spins(other, np.arange(1 << nl))[:, :nl] if nl < n[other] else spins(other, np.arange(1 << nl))
            blk = J[off[other]:off[other] + nl, off[k]:off[k + 1]]
            c[name] = np.einsum('li,ij,sj->sl', so[:, :nl], blk, sk).astype(np.float64)
            c[mp] = (np.arange(1 << n[other]) & ((1 << nl) - 1)).astype(np.int64)
        cells.append(c)
    cellbits = np.full((16, 8), -1, dtype=np.int32)
    bitcell = np.zeros((N, 2), dtype=np.int32)
    for k in range(16):
        cellbits[k, :n[k]] = off[k] + np.arange(n[k])
        bitcell[off[k]:off[k + 1], 0] = k
        bitcell[off[k]:off[k + 1], 1] = np.arange(n[k])
    rowptr, cols = xr.csr(N, np.argwhere(J != 0))
    return dict(cells=cells, Nx=Nx, Ny=Ny, nbits=N, cellbits=cellbits, bitcell=bitcell, rowptr=rowptr, cols=cols, J=J, h=h)


def ising_energy(lat, states):
    """E = sum J_ij s_i s_j + sum h_i s_i of (M, 16) cell states, straight from the couplings (int64)."""
    bits = np.array([[(int(states[m, k]) >> int(j)) & 1 for k, j in lat['bitcell']] for m in range(states.shape[0])])
    s = 1 - 2 * bits
    return np.einsum('mi,ij,mj->m', s, lat['J'], s) + s @ lat['h']


# ---------------------------------------------------------------------------------------------- shared inputs
ROUNDS, SWEEPS = 4, 2
BETAS_A, R_A = (0.3, 0.6, 0.9, 1.3), 65                                  # (a): T = 4, M = 260 crosses the 256-sample tile
BETAS_B, R_B, FROM_B = (0.05, 0.12, 0.25), 6, 1                             # (b): T = 3, M = 18, cluster moves at t >= 1
# (a): lattices of relax_ref.LATTICES with make_cells; a seed whose margins fall below the bound (tests/test_temper_host.py) is
# replaced, never excused
CASES_A = [('3x3', True, 5101), ('3x3', False, 5110), ('2x2', False, 5110), ('1x3', True, 5110)]
CASES = [('a',) + c for c in CASES_A] + [('b', 'ising4x4', True, 5201)]
CASE_IDS = ['%s-%s-%s' % (c[0], c[1], 'maps' if c[2] else 'nomaps') for c in CASES]


@functools.lru_cache(maxsize=None)
def case_inputs(case, rounds=ROUNDS):
    """dict(cells, Nx, Ny, betas, states, tidx, slot, usweep, bits, cluster_from, cpairs, ucl, uswap) of a shared case; computed once,
    never modified."""
    kind, name, maps, seed = case
    rng = np.random.default_rng(seed)
    if kind == 'a':
        Ny, Nx, qs = rr.LATTICES[name]
        cells = rr.make_cells(Ny, Nx, qs, maps, seed + 1000)
        betas, R, bits, cluster_from = np.array(BETAS_A), R_A, None, len(BETAS_A)
    else:
        lat = ising_lattice()
        Ny, Nx, cells = lat['Ny'], lat['Nx'], lat['cells']
        qs = [c['q'] for c in cells]
        betas, R, cluster_from = np.array(BETAS_B), R_B, FROM_B
        bits = (lat['nbits'], lat['cellbits'], lat['bitcell'], lat['rowptr'], lat['cols'])
    T = betas.size
    M = R * T
    Tc, Pc = T - cluster_from, (R // 2 if bits is not None else 0)
    states = rng.integers(0, np.asarray(qs)[None, :], size=(M, len(qs)))
    tidx, slot = fresh_assignment(M, T)
    d = dict(cells=cells, Nx=Nx, Ny=Ny, betas=betas, states=states, tidx=tidx, slot=slot, usweep=rng.random((rounds, SWEEPS, len(qs), M)),
             bits=bits, cluster_from=cluster_from,
             cpairs=np.array([rng.permutation(R)[:2 * Pc].reshape(Pc, 2) for _ in range(rounds)], dtype=np.int32).reshape(rounds, Pc, 2),
             ucl=rng.random((rounds, Tc, Pc)), uswap=rng.random((rounds, R, T - 1)))
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def run_case(c, round0=0, lo=0, hi=None, state=None):
    """run() on the rounds lo .. hi - 1 of a case's inputs, from `state` = a previous result (None: the case's start)."""
    hi = c['usweep'].shape[0] if hi is None else hi
    s = state or dict(states=c['states'], tidx=c['tidx'], slot=c['slot'], accepted=None, attempted=None)
    return run(c['cells'], c['Nx'], c['Ny'], s['states'], c['betas'], s['tidx'], s['slot'], round0 + lo, hi - lo, SWEEPS, c['usweep'][lo:hi], c['bits'],
               c['cluster_from'], c['cpairs'][lo:hi], c['ucl'][lo:hi], c['uswap'][lo:hi], s['accepted'], s['attempted'])


@functools.lru_cache(maxsize=None)
def case_reference(case):
    return run_case(case_inputs(case))


# ---------------------------------------------------------------------------------------------- the exact joint law of one chain, T = 2
LAW_BETAS = (0.35, 0.7)
LAW_R, LAW_ROUNDS, LAW_SEED = 2 ** 14, 3, 123


def swap_acceptance(cells, betas):
    """a[x, y] = min(1, exp((beta1 - beta0)(E(y) - E(x)))): x the configuration at temperature 0, y at temperature 1."""
    E = rr.total_energy(cells, 2, 2, rr.all_configurations(cells))
    return np.minimum(1.0, np.exp((betas[1] - betas[0]) * (E[None, :] - E[:, None])))


def joint_round(mu, P0, P1, a, swap, sweeps=1):
    """One round on the joint law mu[x, y]: mu <- (P0^T)^sweeps mu P1^sweeps, then (with swap) mu'(x, y) = mu(x, y)(1 - a(x, y)) +
    mu(y, x) a(y, x)."""
    for _ in range(sweeps):
        mu = P0.T @ mu @ P1
    if swap:
        mu = mu * (1.0 - a) + mu.T * a.T
    return mu


@functools.lru_cache(maxsize=None)
def law_inputs():
    """(cells, betas, states (2 LAW_R, 4) uniformly random, usweep (LAW_ROUNDS, 1, 4, M), uswap (LAW_ROUNDS, LAW_R, 1), the exact
    marginals [law at temperature 0, law at temperature 1] (256,) each after LAW_ROUNDS rounds from the uniform joint law)."""
    cells, _ = rr.law_problem()
    betas = np.array(LAW_BETAS)
    rng = np.random.default_rng(LAW_SEED)
    M = 2 * LAW_R
    states = rng.integers(0, 4, size=(M, 4))
    usweep, uswap = rng.random((LAW_ROUNDS, 1, 4, M)), rng.random((LAW_ROUNDS, LAW_R, 1))
    P0, P1 = rr.sweep_matrix(cells, 2, 2, betas[0]), rr.sweep_matrix(cells, 2, 2, betas[1])
    a = swap_acceptance(cells, betas)
    mu = np.full((256, 256), 1.0 / 65536)
    for r in range(LAW_ROUNDS):
        mu = joint_round(mu, P0, P1, a, r % 2 == 0)
    return cells, betas, states, usweep, uswap, [mu.sum(axis=1), mu.sum(axis=0)]


def law_check(states, tidx, marginals):
    """relax_ref.law_statistic of the rows at each temperature index against its exact marginal: [(passes, z, bins)] for t = 0, 1."""
    return [rr.law_statistic(rr.configuration_index(states[tidx == t]), marginals[t]) for t in (0, 1)]
