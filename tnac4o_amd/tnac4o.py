"""The ``tnac4o`` solver class on MI355X: same constructor, methods and result attributes as the reference's
``tnac4o.tnac4o`` (tnac4o/tnac4o.py:78-551) for the ground-state path, with the PEPS contraction on the GPU.

Split of work
  host (numpy, O(nnz) / O(M) integer work): coupling split, rotations, energy tables, the branch bookkeeping of
      search_ground_state (cut-off, merge of equal boundary indices, top-M) — restated from the reference so that
      tie-breaking agrees;
  GPU (libtnpeps): boundary-MPS sweeps (absorb, QR, Jacobi SVD, GEMMs) through ``tnac4o_amd.mps``; right
      environments for every distinct boundary suffix (batched GEMMs); left environments for every distinct prefix;
      conditional probabilities of all branches of a site-step in one launch (tn_calc_pn).

The 5-leg PEPS tensor (q,l,d,r,u) of the reference (tnac4o.py:1562-1672; 134 MB and 1/256 dense for chimera) is
never formed: T[s,l,d,r,u] = F[s,l,u] [d = dmap[s]] [r = rmap[s]].
"""
import itertools
import logging
import os

import numpy as np
import functools

import torch

from . import mps, ops


@functools.lru_cache(maxsize=64)
def _bits(n):
    # (memoised, read-only: a sweep asks for the same handful of tables four times per site)
    s = np.arange(2 ** n)[:, None]
    out = ((s >> np.arange(n)[None, :]) & 1).astype(np.int64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=64)
def _spins(n):
    out = 1 - 2 * _bits(n)
    out.setflags(write=False)
    return out


def _dev_f64(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64).cuda()


def _dev_i32(x):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def _unique_rows(a):
    """Sorted unique rows and the inverse map — the same result as np.unique(a, axis=0, return_inverse=True)
    (lexicographic row order) for non-negative integer rows, computed on packed 64-bit keys instead of a sort of
    multi-byte records (30x faster for the 262144 x 17 candidate tables of a site-step).  Handles zero-width keys."""
    n, w = a.shape
    if w == 0:
        return np.zeros((1, 0), dtype=a.dtype), np.zeros(n, dtype=np.int64)
    if n == 0 or a.min() < 0:
        u, inv = np.unique(a, axis=0, return_inverse=True)
        return u, inv.reshape(-1)
    bits = max(1, int(a.max()).bit_length())
    inv, c0 = None, 0
    while c0 < w:
        # the rank of the prefix processed so far (order preserving) goes in the high bits, as many new columns as fit below
        used = 0 if inv is None else max(1, int(inv.max()).bit_length())
        ncol = max(1, min(w - c0, (63 - used) // bits))
        key = np.zeros(n, dtype=np.uint64) if inv is None else inv.astype(np.uint64)
        for j in range(c0, c0 + ncol):
            key = (key << np.uint64(bits)) | a[:, j].astype(np.uint64)
        _, inv = np.unique(key, return_inverse=True)
        inv = inv.reshape(-1)
        c0 += ncol
    first = np.zeros(int(inv.max()) + 1, dtype=np.int64)
    first[inv[::-1]] = np.arange(n - 1, -1, -1)      # any representative row of each group
    return a[first], inv


def _rank_in(keys, rows):
    """Rank of every row of `rows` among the sorted unique rows `keys` (each of them must occur there)."""
    _, inv = _unique_rows(np.vstack([keys, rows]))
    return inv[len(keys):]


def _read_back(tensors):
    """Host arrays with the shapes of a list of float64 device tensors, through ONE device-to-host copy."""
    flat = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
    offs = np.cumsum([0] + [int(t.numel()) for t in tensors])
    return [flat[lo:hi].reshape(tuple(t.shape)).copy() for t, lo, hi in zip(tensors, offs[:-1], offs[1:])]


def _sweep_options(graduate_truncation, Dmax, tolS, tolV, max_sweeps):
    """The options of a boundary sweep, as _setup_rhoT / _setup_rhoB take them."""
    return dict(graduate_truncation=graduate_truncation, Dmax=Dmax, tolS=tolS, tolV=tolV, max_sweeps=max_sweeps)


def _merge_groups(inv, Eng, prob, deg, min_dEng, canonical=True):
    """The merge of branches with identical boundary indices (tnac4o.py:481-509), vectorised: per group the
    representative is the first minimal-energy member, the degeneracy is summed over members within min_dEng of the minimum
    and their log-probabilities are averaged.  canonical (default; see tnac4o_amd/beam.py): members in candidate order (stable
    sort), the mean added up in member order -- what tn_merge_groups does on the device.  canonical=False: numpy's own order
    (unstable argsort, np.mean), the order the reference happens to get."""
    order = inv.argsort(kind='stable') if canonical else inv.argsort()
    ginv = inv[order]
    n_grp = int(ginv[-1]) + 1
    starts = np.flatnonzero(np.r_[True, ginv[1:] != ginv[:-1]])
    E = Eng[order]
    Emin = np.minimum.reduceat(E, starts)
    pos = np.arange(E.size)
    is_min = E == Emin[ginv]
    first_min = np.minimum.reduceat(np.where(is_min, pos, E.size), starts)
    indn = order[first_min]
    near = (E - Emin[ginv]) <= min_dEng
    cnt = np.add.reduceat(near.astype(np.int64), starts)
    degn = np.add.reduceat(np.where(near, deg[order], 0), starts)
    probn = prob[indn].copy()
    # single-member case: deg/prob of that member (== the representative); several: mean in the reference's summation order
    for k in np.flatnonzero(cnt > 1):
        lo = starts[k]
        hi = starts[k + 1] if k + 1 < n_grp else E.size
        same = order[lo:hi][near[lo:hi]]
        if canonical:
            acc = 0.0
            for v in prob[same]:
                acc += float(v)
            probn[k] = acc / len(same)
        else:
            probn[k] = np.mean(prob[same])
    return indn, degn, probn, order, starts


class _RowWalk:
    """The environments of one row of a host walk (host path of search_ground_state, gibbs_sampling; tnac4o.py:434-436,
    528-542): right environments of every distinct suffix of the boundary rows `vind` at the start of the row, left
    environments of the distinct prefixes carried from site to site."""

    def __init__(self, solver, vind, ny):
        self.solver, self.ny = solver, ny
        self.levels = solver._setup_RR(vind, ny)
        self.top = solver.rhoT[ny + 1]
        self.pkeys = np.zeros((1, 0), dtype=vind.dtype)                      # distinct prefixes, sorted
        self.RL = torch.ones((1, 1), dtype=torch.float64, device=self.top.A[0].device)      # (nprefix, Dl)

    def site(self, nx, vind):
        """What ops.calc_pn takes at site nx for the boundary rows vind: (T1, RR, F, dmap, rmap, pref, suf) with pref / suf the
        rank of each row's prefix / suffix among the rows of T1 / RR."""
        F, dmap, rmap, _, _ = self.solver._peps_factor_dev(self.ny, nx)
        AT = self.top.A[nx]
        Dl, p, Dr = AT.shape
        # every prefix's left environment through the top site in one GEMM: T1[prefix, d, chi']
        self.T1 = ops.mm(self.RL, AT.view(Dl, p * Dr)).view(-1, p, Dr)
        skeys, RR = self.levels[len(self.levels) - nx - 1]
        return self.T1, RR, F, dmap, rmap, _rank_in(self.pkeys, vind[:, :nx]), _rank_in(skeys, vind[:, nx + 2:])

    def advance(self, nx, vind):
        """Left environments of the distinct prefixes vind[:, :nx+1] once site nx is decided: rows of T1 (tnac4o.py:528-535)."""
        nkeys, _ = _unique_rows(vind[:, :nx + 1])
        par = _rank_in(self.pkeys, nkeys[:, :nx])
        self.RL = ops.env_rl(self.T1, _dev_i32(par), _dev_i32(nkeys[:, nx]))
        self.pkeys = nkeys

    @staticmethod
    def end_row(vind):
        """The row's lower bonds become the next row's upper ones (tnac4o.py:540-542)."""
        vind[:, 1:] = vind[:, :-1]
        vind[:, 0] = 0


def model_marginals(P_rot, order, ind0=None, L=None):
    """Cell marginals of a (possibly rotated) lattice in model order, and the magnetisations they imply (host side of
    calculate_marginals).  P_rot[c] is the marginal of cell c of the rotated lattice (row-major); model cell k sits at rotated
    cell order[k] and keeps its state encoding.  With ind0 (the model's active spins per cell, Ising) and L, also
    m_i = sum_s P_k(s) sigma_i(s) with sigma = +1 where binary_states writes 1; inactive spins get 0.  Returns (marginals, m)
    with m None when ind0 is None."""
    marg = [np.asarray(P_rot[int(c)], dtype=np.float64) for c in order]
    if ind0 is None:
        return marg, None
    m = np.zeros(L)
    k = 0
    for row in ind0:
        for act in row:
            act = np.asarray(act, dtype=np.int64)
            if act.size:
                m[act] = marg[k] @ _spins(act.size)
            k += 1
    return marg, m


def model_correlations(Pl_rot, Pu_rot, order, Nx, Ny, J0=None, ind=None, ir=None, idn=None, keys=None, Nx_model=None):
    """Nearest-neighbour correlations in the model frame from the bond tables of a (possibly rotated) lattice (host side of
    calculate_correlations).  Pl_rot[c] (q, bl) / Pu_rot[c] (q, pu) is the joint law of rotated cell c (row-major, Nx x Ny) with
    its left / upper bond index; model cell k sits at rotated cell order[k] and keeps its state encoding, so rotated spin
    c*Nc + a is model spin order_i[c]*Nc + a.
      Ising (J0, the model's couplings, and the rotated frame's ind, ir, id): returns (bond_pairs (n, 2) int64, C (n,)) for every
      off-diagonal J0[i, j] != 0, i < j, sorted; C = <sigma_i sigma_j> with sigma = +1 where binary_states writes 1.  Intra-cell
      pairs come from the cell law p[s] = sum_l Pl[s, l].
      RMF (keys, the rotated frame's two-cell factor keys, and Nx_model): returns {model key: P[s1, s2]} with s1 the state of the
      key's first cell; the model key is the rotated key mapped back through order, i.e. the key as the model gave it."""
    order = np.asarray(order, dtype=np.int64)
    order_i = np.empty_like(order)
    order_i[order] = np.arange(order.size)

    def table(c1, c2):                  # P[s1, s2] of two neighbouring rotated cells, from the table at the right / lower one
        (y1, x1), (y2, x2) = divmod(c1, Nx), divmod(c2, Nx)
        if y1 == y2 and x2 == x1 + 1:
            return Pl_rot[c2].T
        if y1 == y2 and x1 == x2 + 1:
            return Pl_rot[c1]
        if x1 == x2 and y2 == y1 + 1:
            return Pu_rot[c2].T
        if x1 == x2 and y1 == y2 + 1:
            return Pu_rot[c1]
        raise ValueError('cells %d and %d of the rotated lattice are not nearest neighbours' % (c1, c2))

    if J0 is None:
        out = {}
        for key in keys:
            if len(key) != 4:
                continue
            c1, c2 = key[0] * Nx + key[1], key[2] * Nx + key[3]
            k1, k2 = int(order_i[c1]), int(order_i[c2])
            mkey = divmod(k1, Nx_model) + divmod(k2, Nx_model)
            out[mkey] = np.ascontiguousarray(table(c1, c2), dtype=np.float64)
        return out
    Nc = J0.shape[0] // (Nx * Ny)

    def model(x):
        return int(order_i[x // Nc]) * Nc + x % Nc

    C = {}

    def put(spins_a, spins_b, M):
        for a, i in enumerate(spins_a):
            for b, j in enumerate(spins_b):
                if i != j:
                    C[tuple(sorted((model(int(i)), model(int(j)))))] = float(M[a, b])

    for ny in range(Ny):
        for nx in range(Nx):
            c = ny * Nx + nx
            here = np.asarray(ind[ny][nx], dtype=np.int64)
            S = _spins(here.size)
            Pl = np.asarray(Pl_rot[c])
            p = Pl.sum(1)
            put(here, here, S.T @ (p[:, None] * S))
            if nx > 0 and len(ir[ny][nx - 1]):
                left = np.asarray(ind[ny][nx - 1])[ir[ny][nx - 1]]
                put(here, left, S.T @ Pl @ _spins(left.size))
            if ny > 0 and len(idn[ny - 1][nx]):
                up = np.asarray(ind[ny - 1][nx])[idn[ny - 1][nx]]
                put(here, up, S.T @ np.asarray(Pu_rot[c]) @ _spins(up.size))
    pairs = np.argwhere(np.triu(J0, 1) != 0).astype(np.int64)
    missing = [tuple(p) for p in pairs if tuple(int(v) for v in p) not in C]
    if missing:
        raise ValueError('couplings between cells that are not nearest neighbours: %s' % missing[:4])
    return pairs, np.array([C[(int(i), int(j))] for i, j in pairs], dtype=np.float64)


def model_line_correlations(tables, order, Nx, ind=None, Nc=None, Nx_model=None):
    """Two-point functions along lattice lines in the model frame from tables of a (possibly rotated) lattice (host side of
    calculate_correlation_function).  tables: {(c1, c2): M} for pairs of different cells c = ny*Nx + nx of the rotated lattice (row-major,
    Nx columns) that share a row or a column there; model cell k sits at rotated cell order[k] and keeps its state encoding, so
    rotated spin c*Nc + a is model spin order_i[c]*Nc + a.  The cell distance of a pair is the same in both frames.
      Ising (ind, the rotated frame's active spins per cell, and Nc): M[a, b] = <sigma_i sigma_j> of i = ind[c1][a], j = ind[c2][b];
      returns (line_pairs (n, 2) int64 of model spins i < j, sorted; line_distance (n,) int64; C (n,)).
      RMF (ind None, Nx_model): M = P[s1, s2]; returns {(y1, x1, y2, x2): P} in model coordinates, the cell that comes first in
      the model's row-major order first (M transposed where the rotation swaps the two)."""
    order = np.asarray(order, dtype=np.int64)
    order_i = np.empty_like(order)
    order_i[order] = np.arange(order.size)

    def distance(c1, c2):
        (y1, x1), (y2, x2) = divmod(c1, Nx), divmod(c2, Nx)
        if c1 == c2 or (y1 != y2 and x1 != x2):
            raise ValueError('cells %d and %d of the rotated lattice are not two cells of one line' % (c1, c2))
        return abs(y1 - y2) + abs(x1 - x2)

    if ind is None:
        out = {}
        for (c1, c2), M in tables.items():
            distance(c1, c2)
            k1, k2 = int(order_i[c1]), int(order_i[c2])
            M = np.asarray(M, dtype=np.float64)
            if k1 > k2:
                k1, k2, M = k2, k1, M.T
            out[divmod(k1, Nx_model) + divmod(k2, Nx_model)] = np.ascontiguousarray(M)
        return out
    rows = []
    for (c1, c2), M in tables.items():
        dist = distance(c1, c2)
        s1, s2 = np.asarray(ind[c1 // Nx][c1 % Nx], dtype=np.int64), np.asarray(ind[c2 // Nx][c2 % Nx], dtype=np.int64)
        M = np.asarray(M, dtype=np.float64).reshape(s1.size, s2.size)
        for a, i in enumerate(s1):
            for b, j in enumerate(s2):
                mi, mj = int(order_i[i // Nc]) * Nc + int(i % Nc), int(order_i[j // Nc]) * Nc + int(j % Nc)
                rows.append((min(mi, mj), max(mi, mj), dist, float(M[a, b])))
    rows.sort(key=lambda t: t[:2])
    pairs = np.array([t[:2] for t in rows], dtype=np.int64).reshape(-1, 2)
    return pairs, np.array([t[2] for t in rows], dtype=np.int64), np.array([t[3] for t in rows], dtype=np.float64)


def _plan_line_groups(nops, reach, cap):
    """Start cells 0 .. len(nops)-1 of one line cut into consecutive groups [(k0, k1)] so that a stack that carries the plain slot and
    the nops[k] slots of the group's start cells k within `reach` cells back, the step's own insertions included, never holds more
    than `cap` slots.  One (possibly empty) group at least.  MemoryError when one start cell alone does not fit."""
    def peak(k0, k1):
        return 1 + max(sum(nops[max(k0, m - reach):m + 1]) for m in range(k0, k1))
    groups, k0 = [], 0
    for k in range(len(nops)):
        if 1 + nops[k] > cap:
            raise MemoryError('the stack of one start cell has %d slots, the slot budget holds %d' % (1 + nops[k], max(int(cap), 0)))
        if peak(k0, k + 1) > cap:
            groups.append((k0, k))
            k0 = k
    groups.append((k0, len(nops)))
    return groups


def load(file_name):
    """Load a solution written by `tnac4o.save` -- by this package or by the reference (same .npy pickle of a dict,
    tnac4o.py:31-75).  Couplings are not stored, so the returned instance only carries the results (energy, states, ...)
    and what `binary_states` needs."""
    d = np.load(file_name, allow_pickle=True).item()
    ins = tnac4o(mode=d.get('mode'), Nx=d.get('Nx'), Ny=d.get('Ny'), Nc=d.get('Nc'), beta=d.get('beta'))
    for k in ('energy', 'probability', 'degeneracy', 'states', 'discarded_probability', 'negative_probability'):
        setattr(ins, k, d.get(k))
    if d.get('rotation') is not None:
        ins.rotation = d.get('rotation')
    if ins.mode == 'Ising':
        ins.ind0 = d.get('ind')
        ins.adj = np.zeros((0, 0))
    else:
        ins.ind0, ins.adj = [], []
    if d.get('excitations_encoding') is not None:          # droplet bookkeeping of the reference (:64-74): carried over
        for k in ('excitations_encoding', 'd', 'invd', 'el', 'free_d'):
            setattr(ins, k, d.get(k))
        if ins.excitations_encoding > 1:
            from . import droplets
            if ins.mode == 'Ising':
                adj = d.get('adj')
                ins.adj = np.asarray(adj.toarray() if hasattr(adj, 'toarray') else adj) != 0
                ins._conn = droplets.Connectivity('Ising', ins.Nx, ind=ins.ind0, adj=ins.adj | ins.adj.T)
            else:
                ins._conn = droplets.Connectivity('RMF', ins.Nx)
    return ins


class tnac4o:
    """Ising ('Ising') or Random-Markov-Field ('RMF') problem on an Nx x Ny lattice of cells (tnac4o.py:145-198)."""

    def __init__(self, mode='Ising', Nx=4, Ny=4, Nc=8, beta=1, J=None):
        self.mode, self.beta = mode, beta
        self.Nx_model, self.Ny_model = Nx, Ny
        self.Nx, self.Ny = Nx, Ny
        if mode == 'Ising':
            if Nc > 9:
                raise ValueError('Single cluster is too large.')
            self.Nc = Nc
            self.indtype = np.int8 if Nc <= 8 else np.int16
        elif mode == 'RMF':
            self.Nc = 1
            self.indtype = np.int8
        else:
            raise ValueError("mode must be 'Ising' or 'RMF'")
        self.L = Nx * Ny * self.Nc
        self.order = np.arange(Nx * Ny)
        self.order_i = np.arange(Nx * Ny)
        self.logger = logging.getLogger('tnac4o')
        self.energy = np.zeros(0)
        self.probability = np.zeros(0)
        self.rotation = 0
        self.degeneracy = 0
        self.states = np.zeros((0, Nx * Ny), dtype=self.indtype)
        self.discarded_probability = -np.inf
        self.negative_probability = 0.0
        self.ind0, self.J0 = [], []
        if J is not None:
            if mode == 'Ising':
                Jd = np.zeros((self.L, self.L))              # upper triangular accumulation (tnac4o.py:176-181)
                for i, j, v in J:
                    a, b = (i, j) if i <= j else (j, i)
                    Jd[a, b] += v
                self.J = Jd
                self.J0 = Jd.copy()
                self.ind0 = [[self._active(ny, nx) for nx in range(Nx)] for ny in range(Ny)]
                self.active = sum(len(self.ind0[ny][nx]) for ny in range(Ny) for nx in range(Nx))
            else:
                self.J = {'fun': J['fun'], 'fac': dict(J['fac']), 'N': J['N']}
                self.N = np.array(J['N']).copy()
            self._divide_couplings()

    # ------------------------------------------------------------------------------------ problem setup (host)
    def _active(self, ny, nx):
        ind = self.Nc * (self.Nx * ny + nx) + np.arange(self.Nc)
        w = np.abs(self.J[ind, :]).sum(1) + np.abs(self.J[:, ind]).sum(0)
        return ind[w > 1e-12]

    def _divide_couplings(self):
        """Per-cell coupling blocks and bond index sets (tnac4o.py:1391-1457)."""
        Ny, Nx = self.Ny, self.Nx
        self.lu = np.ones((Ny, Nx), dtype=int)
        self.lr = np.ones((Ny, Nx), dtype=int)
        self.ll = np.ones((Ny, Nx), dtype=int)
        self.ld = np.ones((Ny, Nx), dtype=int)
        if self.mode == 'Ising':
            self.ind = [[self._active(ny, nx) for nx in range(Nx)] for ny in range(Ny)]
            self.sN = np.array([[len(self.ind[ny][nx]) for nx in range(Nx)] for ny in range(Ny)])
            self.N = 2 ** self.sN
            self.Jin = [[None] * Nx for _ in range(Ny)]
            self.Jl = [[np.zeros((self.sN[ny][nx], 0)) for nx in range(Nx)] for ny in range(Ny)]
            self.Ju = [[np.zeros((self.sN[ny][nx], 0)) for nx in range(Nx)] for ny in range(Ny)]
            self.id = [[np.zeros(0, dtype=int) for _ in range(Nx)] for _ in range(Ny)]
            self.ir = [[np.zeros(0, dtype=int) for _ in range(Nx)] for _ in range(Ny)]
            self.sl, self.sd, self.sr, self.su = (np.zeros((Ny, Nx), dtype=int) for _ in range(4))
            for ny in range(Ny):
                for nx in range(Nx):
                    ind = self.ind[ny][nx]
                    self.Jin[ny][nx] = self.J[np.ix_(ind, ind)]
                    for (oy, ox, Jn, idx, s_here, s_there, ldim) in (
                            (ny, nx - 1, self.Jl, self.ir, self.sl, self.sr, self.lr),
                            (ny - 1, nx, self.Ju, self.id, self.su, self.sd, self.ld)):
                        if oy < 0 or ox < 0:
                            continue
                        JJ = self.J[np.ix_(self.ind[oy][ox], ind)]
                        rows = np.nonzero(np.abs(JJ).sum(1))[0]
                        Jn[ny][nx] = JJ[rows].T
                        idx[oy][ox] = rows
                        s_here[ny][nx] = s_there[oy][ox] = len(rows)
                        ldim[oy][ox] = 2 ** len(rows)
        else:
            fac = self.J['fac']
            for ny in range(Ny):
                for nx in range(Nx):
                    if (ny, nx - 1, ny, nx) in fac or (ny, nx, ny, nx - 1) in fac:
                        self.ll[ny, nx] = self.N[ny][nx - 1]
                    if (ny, nx, ny, nx + 1) in fac or (ny, nx + 1, ny, nx) in fac:
                        self.lr[ny, nx] = self.N[ny][nx + 1]
                    if (ny - 1, nx, ny, nx) in fac or (ny, nx, ny - 1, nx) in fac:
                        self.lu[ny, nx] = self.N[ny - 1][nx]
                    if (ny, nx, ny + 1, nx) in fac or (ny + 1, nx, ny, nx) in fac:
                        self.ld[ny, nx] = self.N[ny + 1][nx]
        self._reset_X()

    def _reset_X(self):
        """Gauge diagonals on the PEPS bonds (tnac4o.py:1811-1822)."""
        Ny, Nx = self.Ny, self.Nx
        self.Xu = np.ones((Ny, Nx, np.max(self.ld)))
        self.Xd = np.ones((Ny, Nx, np.max(self.ld)))
        self.Xl = np.ones((Ny, Nx, np.max(self.lr)))
        self.Xr = np.ones((Ny, Nx, np.max(self.lr)))
        self.overlaps_ud = np.empty((0, Ny - 1))

    def rotate_graph(self, rot=1):
        """Rotate the lattice by 90 degrees `rot` times: cell (ny,nx) -> (Nx-1-nx, ny) (tnac4o.py:290-340)."""
        for _ in range(rot):
            Nx, Ny, Nc = self.Nx, self.Ny, self.Nc
            order_i = np.arange(Nx * Ny)
            if self.mode == 'Ising':
                self.rotation += 1
                cells = np.arange(Nx * Ny).reshape(Ny, Nx)
                dst = ((Nx - 1 - np.arange(Nx))[None, :] * Ny + np.arange(Ny)[:, None])      # [ny, nx] -> new cell
                perm = np.empty(self.L, dtype=int)
                perm[(cells[:, :, None] * Nc + np.arange(Nc)).reshape(-1)] = (dst[:, :, None] * Nc + np.arange(Nc)).reshape(-1)
                order_i[dst.reshape(-1)] = cells.reshape(-1)
                Jp = self.J[np.ix_(perm, perm)]
                self.J = np.triu(Jp) + np.tril(Jp, -1).T
            else:
                new = {}
                for key, val in self.J['fac'].items():
                    if len(key) == 2:
                        new[(Nx - key[1] - 1, key[0])] = val
                    else:
                        new[(Nx - key[1] - 1, key[0], Nx - key[3] - 1, key[2])] = val
                Nn = np.zeros((Nx, Ny), dtype=int)
                for nx in range(Nx):
                    for ny in range(Ny):
                        Nn[Nx - nx - 1, ny] = self.N[ny, nx]
                        order_i[ny * Nx + nx] = (Nx - nx - 1) * Ny + ny
                self.J['fac'], self.N = new, Nn
            self.Nx, self.Ny = Ny, Nx
            self.order = order_i[self.order]
        self.order_i[self.order] = np.arange(self.Nx * self.Ny)
        self.rotation = self.rotation % 4
        self._divide_couplings()

    # ------------------------------------------------------------------------------------ local tables (host)
    def _cell_maps(self, ny, nx):
        """dmap[s], rmap[s], pd, br of a cell: the index every cell state s puts on the bond to the row below / to the cell on
        the right, and the dimensions of those two bonds (tnac4o.py:1469-1489, 1598-1607)."""
        if self.mode == 'Ising':
            bt = _bits(self.sN[ny][nx])
            rmap = bt[:, self.ir[ny][nx]] @ (2 ** np.arange(self.sr[ny][nx]))
            dmap = bt[:, self.id[ny][nx]] @ (2 ** np.arange(self.sd[ny][nx]))
            br, pd = 2 ** self.sr[ny][nx], 2 ** self.sd[ny][nx]
        else:
            q = int(self.N[ny][nx])
            s = np.arange(q)
            br, pd = int(self.lr[ny, nx]), int(self.ld[ny, nx])
            rmap = s % br if br > 1 else np.zeros(q, dtype=int)
            dmap = s % pd if pd > 1 else np.zeros(q, dtype=int)
        return dmap, rmap, int(pd), int(br)

    def _ind_bond_down(self, st, ny, nx):
        """tnac4o.py:1469-1478."""
        return self._cell_maps(ny, nx)[0][st]

    def _ind_bond_right(self, st, ny, nx):
        """tnac4o.py:1480-1489."""
        return self._cell_maps(ny, nx)[1][st]

    def _cell_energies(self, ny, nx):
        """Es[s], Ese1[s,l], Ese4[s,u] (Ising tnac4o.py:1570-1581, RMF 1613-1635)."""
        if self.mode == 'Ising':
            st = _spins(self.sN[ny][nx])
            Jin = self.Jin[ny][nx]
            Es = np.sum((st @ np.triu(Jin, 1)) * st, 1) + st @ Jin.diagonal()
            return Es, (st @ self.Jl[ny][nx]) @ _spins(self.sl[ny][nx]).T, (st @ self.Ju[ny][nx]) @ _spins(self.su[ny][nx]).T
        fac, fun, N = self.J['fac'], self.J['fun'], self.N[ny][nx]
        Es = np.reshape(fun[fac[(ny, nx)]], N) if (ny, nx) in fac else np.zeros(N)
        if (ny, nx - 1, ny, nx) in fac:
            E1 = fun[fac[(ny, nx - 1, ny, nx)]].T
        elif (ny, nx, ny, nx - 1) in fac:
            E1 = fun[fac[(ny, nx, ny, nx - 1)]]
        else:
            E1 = np.zeros((N, self.ll[ny, nx]))
        if (ny - 1, nx, ny, nx) in fac:
            E4 = fun[fac[(ny - 1, nx, ny, nx)]].T
        elif (ny, nx, ny - 1, nx) in fac:
            E4 = fun[fac[(ny, nx, ny - 1, nx)]]
        else:
            E4 = np.zeros((N, self.lu[ny, nx]))
        return Es, E1, E4

    def _update_Eng(self, states, ny, nx):
        """Energy added by cell (ny,nx) to partial configurations (tnac4o.py:1506-1558)."""
        Es, E1, E4 = self._cell_energies(ny, nx)
        pos = ny * self.Nx + nx
        dE = 1.0 * Es[states[:, pos]]
        if nx > 0:
            left = states[:, pos - 1]
            dE += E1[states[:, pos], self._ind_bond_right(left, ny, nx - 1) if self.mode == 'Ising' else left]
        if ny > 0:
            up = states[:, pos - self.Nx]
            dE += E4[states[:, pos], self._ind_bond_down(up, ny - 1, nx) if self.mode == 'Ising' else up]
        return dE

    def _peps_factor(self, ny, nx):
        """F[s,l,u], dmap[s], rmap[s], pd, br with T[s,l,d,r,u] = F[s,l,u][d=dmap[s]][r=rmap[s]]
        (tnac4o.py:1562-1672; same floating-point evaluation order as the reference)."""
        Es, E1, E4 = self._scaled_energies(ny, nx)
        F = np.exp((Es[:, None, None] + E1[:, :, None]) + E4[:, None, :])
        nl, nu = F.shape[1], F.shape[2]
        F = F * self.Xu[ny][nx][:nu][None, None, :]
        F = F * self.Xl[ny][nx][:nl][None, :, None]
        dmap, rmap, pd, br = self._cell_maps(ny, nx)
        F = F * self.Xr[ny][nx][rmap][:, None, None]
        F = F * self.Xd[ny][nx][dmap][:, None, None]
        return F, np.asarray(dmap, dtype=np.int64), np.asarray(rmap, dtype=np.int64), pd, br

    def _scaled_energies(self, ny, nx):
        """The three energy tables of a cell as the PEPS factor exponentiates them: beta (min E - E), each table shifted by
        its own minimum (tnac4o.py:1570-1583)."""
        b = self.beta
        Es, E1, E4 = self._cell_energies(ny, nx)
        return b * (np.min(Es) - Es), b * (np.min(E1) - E1), b * (np.min(E4) - E4)

    def _site_tables(self, ny, nx):
        """Host side of K7: the three beta-scaled, min-shifted energy tables and the index maps of a cell (O(q) work;
        tnac4o.py:1570-1583, 1598-1607).  The exponentials, gauge products and the sum over s run on the GPU."""
        Es, E1, E4 = self._scaled_energies(ny, nx)
        return (Es, np.ascontiguousarray(E1), np.ascontiguousarray(E4)) + self._cell_maps(ny, nx)

    def _peps_factors_dev(self, cells):
        """[(F, dmap, rmap, pd, br)] as device tensors for a list of cells (K7, tn_peps_factor).  The seven small float tables of ALL the
        cells travel in ONE host-to-device copy and their index maps in another (nine separate copies per cell cost the sweep 45 ms of
        host time per chain in round 3; two per cell still 11 ms); the kernels run per cell on views of the two buffers."""
        keep = getattr(self, '_factor_keep', None)                 # set for the duration of one search_ground_state call
        out = [keep.get(c) if keep is not None else None for c in cells]
        todo = [i for i, o in enumerate(out) if o is None]
        if not todo:
            return out
        fparts, iparts, meta = [], [], []
        for i in todo:
            ny, nx = cells[i]
            Es, E1, E4, dmap, rmap, pd, br = self._site_tables(ny, nx)
            nl, nu = E1.shape[1], E4.shape[1]
            parts = [np.ravel(Es), np.ravel(E1), np.ravel(E4), np.ravel(self.Xu[ny][nx][:nu]), np.ravel(self.Xl[ny][nx][:nl]),
                     np.ravel(self.Xr[ny][nx]), np.ravel(self.Xd[ny][nx])]
            sizes = [int(x.size) for x in parts]
            for x, n in zip(parts, sizes):                      # every table stays 16-byte aligned inside the packed buffer
                fparts.append(np.asarray(x, dtype=np.float64))
                if n % 2:
                    fparts.append(np.zeros(1))
            q = int(np.size(Es))
            iparts.append(np.asarray(dmap, dtype=np.int32))
            iparts.append(np.asarray(rmap, dtype=np.int32))
            meta.append((i, sizes, q, nl, nu, pd, br))
        dev = torch.as_tensor(np.concatenate(fparts)).cuda()
        maps = torch.as_tensor(np.concatenate(iparts)).cuda()
        off = ioff = 0
        for i, sizes, q, nl, nu, pd, br in meta:
            views = []
            for n in sizes:
                views.append(dev[off:off + n])
                off += n + (n % 2)
            dm, rm = maps[ioff:ioff + q], maps[ioff + q:ioff + 2 * q]
            ioff += 2 * q
            F = ops.peps_factor(views[0], views[1].view(q, nl), views[2].view(q, nu), views[3], views[4], views[5], views[6], dm, rm)
            out[i] = (F, dm, rm, pd, br)
            if keep is not None:
                keep[cells[i]] = out[i]
        return out

    def _peps_factor_dev(self, ny, nx):
        """(F, dmap, rmap, pd, br) of one cell as device tensors."""
        return self._peps_factors_dev([(ny, nx)])[0]

    def _mpo_site_dev(self, ny, nx):
        """Row-MPO site W[l,d,r,u] built on the device (K7, tn_mpo_from_factor)."""
        F, dm, rm, pd, br = self._peps_factor_dev(ny, nx)
        return ops.mpo_from_factor(F, dm, rm, pd, br)

    def _mpo_site(self, ny, nx):
        """W[l,d,r,u] = sum_s T[s,l,d,r,u] (tnac4o.py:1686) as a host array (host twin of _mpo_site_dev, used by tests)."""
        F, dmap, rmap, pd, br = self._peps_factor(ny, nx)
        q, nl, nu = F.shape
        W = np.zeros((pd, br, nl, nu))
        np.add.at(W, (dmap, rmap), F)                 # unbuffered, increasing s: the reference's summation order
        return np.ascontiguousarray(W.transpose(2, 0, 1, 3))

    def _row_mpo(self, ny):
        At = mps.MPO(L=self.Nx)
        for nx, (F, dm, rm, pd, br) in enumerate(self._peps_factors_dev([(ny, nx) for nx in range(self.Nx)])):
            At.set_direct(ops.mpo_from_factor(F, dm, rm, pd, br), nx)
        return At

    # ------------------------------------------------------------------------------------ sweeps (GPU)
    def _setup_rhoT(self, graduate_truncation=True, Dmax=32, tolS=1e-16, tolV=1e-10, max_sweeps=20):
        """Top boundary MPS of every row, built bottom-up (tnac4o.py:1674-1695)."""
        self._setup_boundary('rhoT', _sweep_options(graduate_truncation, Dmax, tolS, tolV, max_sweeps))

    def _setup_rhoB(self, graduate_truncation=True, Dmax=32, tolS=1e-16, tolV=1e-10, max_sweeps=20):
        """Bottom boundary MPS, built top-down (tnac4o.py:1697-1718)."""
        self._setup_boundary('rhoB', _sweep_options(graduate_truncation, Dmax, tolS, tolV, max_sweeps))

    def _setup_boundary(self, name, options):
        """The boundary MPS `name` of every row with their overlaps and discarded weights (name, name_overlap, name_discarded):
        'rhoT' starts below the last row and absorbs the conjugated row MPOs upwards, 'rhoB' starts above the first row and
        absorbs the row MPOs downwards."""
        Ny, up = self.Ny, name == 'rhoT'
        rho, overlap, discarded = [None] * (Ny + 1), [1] * (Ny + 1), [0] * (Ny + 1)
        setattr(self, name, rho)
        setattr(self, name + '_overlap', overlap)
        setattr(self, name + '_discarded', discarded)
        rho[Ny if up else 0] = mps.MPS(d=1, L=self.Nx, Dmax=1, initial='X')
        for ny in (range(Ny - 1, -1, -1) if up else range(Ny)):
            src, dst = (ny + 1, ny) if up else (ny, ny + 1)
            psi = rho[src].copy()
            overlap[dst] = psi.apply_mpo_compress(self._row_mpo(ny), Hconj=up, **options)
            discarded[dst] = max(psi.discarded)
            rho[dst] = psi

    # ------------------------------------------------------------------------------------ preconditioning
    def precondition(self, mode='balancing', steps=2, beta_cond=(), Dmax_cond=(), max_scale=1024,
                     graduate_truncation=False, tolS=1e-16, tolV=1e-10, max_sweeps=20):
        """'balancing' gauge fix of the vertical bonds at reduced beta (tnac4o.py:342-379)."""
        if mode != 'balancing':
            return
        beta_cond = list(beta_cond) or [self.beta * 2.0 ** (n - steps) for n in range(steps)]
        Dmax_cond = list(Dmax_cond) or [8] * len(beta_cond)
        main_beta = self.beta
        for b, D in zip(beta_cond, Dmax_cond):
            self.beta = b
            self.logger.info('Preconditioning with beta = %.2f', b)
            self._update_conditioning(Dmax=D, graduate_truncation=graduate_truncation, tolS=tolS, tolV=tolV,
                                      max_sweeps=max_sweeps, max_scale=max_scale)
        self.beta = main_beta

    def _balance_site(self, B, T, ny, nx, max_scale, pending):
        """One balancing step for the vertical bond above cell (ny,nx) (tnac4o.py:1844-1867), entirely on the GPU: the
        p x p bond environment, its dgebal scaling clamped to [1/max_scale, max_scale] (tn_balance), the two overlaps.
        Nothing is read back here: the scale vector and the overlaps are queued in `pending` and folded into the host-side
        gauge tables Xd / Xu and the diagnostics once per conditioning pass (_flush_balance)."""
        sc = ops.balance(B.bond_env_mix(T, nx), max_scale)
        nrm = torch.linalg.vector_norm
        o1 = B.expectation_mix_dev(T, nx) * torch.reciprocal(nrm(B.A[nx]) * nrm(T.A[nx]))
        B.scale_site_(nx, sc)
        T.scale_site_(nx, sc, inv=True)                     # powers of two: dividing is exactly multiplying by 1/sc
        o2 = B.expectation_mix_dev(T, nx) * torch.reciprocal(nrm(B.A[nx]) * nrm(T.A[nx]))
        pending.append((ny, nx, sc, o1.reshape(1), o2.reshape(1)))

    def _flush_balance(self, pending, overlaps):
        """One device-to-host copy for a whole conditioning pass, then the reference's bookkeeping in its order
        (tnac4o.py:1857-1865)."""
        if not pending:
            return
        host = _read_back([t for p in pending for t in p[2:]])
        for k, (ny, nx, _, _, _) in enumerate(pending):
            scale, o1, o2 = host[3 * k], float(host[3 * k + 1][0]), float(host[3 * k + 2][0])
            if o1 < overlaps[0, ny - 1]:
                overlaps[0, ny - 1] = o1
                overlaps[1, ny - 1] = max(o1, o2)
            kk = self.ld[ny - 1, nx]
            self.Xd[ny - 1, nx, :kk] *= scale
            self.Xu[ny, nx, :kk] *= 1 / scale

    def _update_conditioning(self, graduate_truncation=False, Dmax=8, tolS=1e-16, tolV=1e-10, max_sweeps=4,
                             max_scale=1024):
        """tnac4o.py:1824-1918 ('ud' direction; the 'lr' branch is dead code in the reference)."""
        max_scale = 2.0 ** np.floor(np.log2(np.sqrt(max_scale)))
        kw = _sweep_options(graduate_truncation, Dmax, tolS, tolV, max_sweeps)
        self._setup_rhoT(**kw)
        self._setup_rhoB(**kw)
        overlaps = np.ones((2, self.Ny - 1))
        Nx = self.Nx
        pending = []

        def renorm(B, k):                      # R *= 1 / ||R||  with the norm kept on the device
            B.R[k] = B.R[k] * torch.reciprocal(torch.linalg.vector_norm(B.R[k]))
        for ny in range(1, self.Ny):
            B, T = self.rhoB[ny], self.rhoT[ny]
            for nx in range(Nx):
                B.update_RL_mix(T, nx, keep_on_device=True)
                renorm(B, nx + 1)            # for nx = Nx-1 this touches the unused 1x1 slot R[Nx], as in the reference
            for nx in range(Nx - 1, -1, -1):
                self._balance_site(B, T, ny, nx, max_scale, pending)
                if nx > 0:
                    B.orth_right(nx)
                    B.attach_AC()
                    T.orth_right(nx)
                    T.attach_AC()
                    B.update_RR_mix(T, nx)
                    renorm(B, nx)
            for nx in range(Nx):
                self._balance_site(B, T, ny, nx, max_scale, pending)
                if nx < Nx - 1:
                    B.orth_left(nx)
                    B.attach_CA()
                    T.orth_left(nx)
                    T.attach_CA()
                    B.update_RL_mix(T, nx)
                    renorm(B, nx + 1)
        self._flush_balance(pending, overlaps)
        self.overlaps_ud = np.vstack([self.overlaps_ud, overlaps])
        self.rhoB = []

    # ------------------------------------------------------------------------------------ search (GPU + host)
    def _setup_RR(self, vind, ny):
        """Right environments for every distinct boundary-index suffix of the beam (tnac4o.py:1768-1784).

        Returns a list over levels j = 0 .. Nx-1 (level j belongs to site nx = Nx - j): (keys, RR) with keys the
        sorted unique suffixes vind[:, nx+1:] and RR a device tensor (nkeys, Dl(nx), bl(nx))."""
        top = self.rhoT[ny + 1]
        dev = top.A[0].device
        levels = [(np.zeros((1, 0), dtype=vind.dtype), torch.ones((1, 1, 1), dtype=torch.float64, device=dev))]
        for nx in range(self.Nx - 1, 0, -1):
            keys, _ = _unique_rows(vind[:, nx + 1:])
            pkeys, prr = levels[-1]
            # parent rows: suffix[1:] among pkeys, which are sorted-unique, so the rank indexes rows of prr directly
            parent = _rank_in(pkeys, keys[:, 1:])
            W = self._mpo_site_dev(ny, nx)                                   # (bl, p, br, pu)
            RR = ops.env_rr_any(top.A[nx].contiguous(), prr, W, _dev_i32(parent), _dev_i32(keys[:, 0]))
            levels.append((keys, RR))
        return levels

    def _setup_rhoT_shared(self, group, **kw):
        """The sweep on the first rank of `group`, then rhoT (and its diagnostics) broadcast to the partners
        (the sweep is a sequential chain; only the beam is split)."""
        import torch.distributed as dist
        from . import parallel
        owner = dist.get_rank(group) == 0
        if owner:
            self._setup_rhoT(**kw)
        rows = parallel.broadcast_site_tensors([m.A for m in self.rhoT] if owner else None, group)
        diag = parallel.broadcast_object((list(self.rhoT_overlap), list(self.rhoT_discarded)) if owner else None, group)
        if not owner:
            self.rhoT = []
            dev = torch.device('cuda', torch.cuda.current_device())
            for A in rows:
                m = mps.MPS(d=1, L=self.Nx, Dmax=1, initial='X')
                A = [torch.as_tensor(a, dtype=torch.float64).to(dev) for a in A]      # gloo hands back host arrays
                m.A = A
                m.D = [int(A[0].shape[0])] + [int(a.shape[2]) for a in A]
                self.rhoT.append(m)
            self.rhoT_overlap, self.rhoT_discarded = diag

    def search_low_energy_spectrum(self, excitations_encoding=1, M=2 ** 10, relative_P_cutoff=1e-6, max_dEng=0., lim_hd=0,
                                   min_dEng=1e-12, graduate_truncation=True, Dmax=32, tolS=1e-16, tolV=1e-10,
                                   max_sweeps=20):
        """Branch-and-bound search that also records the droplets of the branches it merges away, from which the
        low-energy spectrum up to max_dEng is rebuilt by `decode_low_energy_states` (tnac4o.py:652-915, encoding 1:
        droplet independence from the row-major order of the cells).  Returns the lowest energies found; stores the
        same result attributes as search_ground_state plus the excitation forest `el` and the shape table `d`."""
        from . import droplets
        if excitations_encoding not in (1, 2, 3):
            raise ValueError('Available droplets handling strategies are excitations_encoding = 1,2,3.')
        self.excitations_encoding = excitations_encoding
        if excitations_encoding == 1:
            rec = droplets.ExcitationRecorder(max_dEng, lim_hd, self.mode)
        else:                                       # independence from the interaction graph of the (rotated) lattice
            conn = droplets.Connectivity(self.mode, self.Nx, J=self.J if self.mode == 'Ising' else None,
                                         ind=self.ind if self.mode == 'Ising' else None)
            cls = droplets.AdjacencyRecorder if excitations_encoding == 2 else droplets.FlatRecorder
            rec = cls(max_dEng, lim_hd, self.mode, conn)
        Eng = self.search_ground_state(M=M, relative_P_cutoff=relative_P_cutoff, min_dEng=min_dEng,
                                       graduate_truncation=graduate_truncation, Dmax=Dmax, tolS=tolS, tolV=tolV,
                                       max_sweeps=max_sweeps, recorder=rec)
        self.el, self.d = rec.finish(self.order_i)
        self.invd = rec.shapes.semi_hash_index()
        self.free_d = rec.shapes.next_id
        if excitations_encoding > 1:                # decoding works in the unrotated cell order (tnac4o.py:1130, 1357)
            self._conn = droplets.Connectivity(self.mode, self.Nx_model, J=self.J0 if self.mode == 'Ising' else None,
                                               ind=self.ind0 if self.mode == 'Ising' else None)
            self.adj = self._conn.adj if self.mode == 'Ising' else []
        return Eng

    def add_noise(self, amplitude=1e-7):
        """Small random perturbation of the couplings (numpy's global generator, like the reference) that removes
        accidental degeneracies before a search with excitations_encoding 2 or 3 (tnac4o.py:917-941)."""
        self.logger.info('Adding noise to the coupling with ampliture %.2e', amplitude)
        if self.mode == 'Ising':
            rows, cols = self.J.nonzero()
            self.J[rows, cols] += (np.random.rand(len(rows)) * 2 - 1) * amplitude
        else:
            fun = {}
            for key, val in self.J['fun'].items():
                fun[key] = np.array(val, dtype=float, copy=True)
                if fun[key].ndim == 1:
                    fun[key] += (np.random.rand(fun[key].shape[0]) * 2 - 1) * amplitude
            self.J['fun'] = fun
        self._divide_couplings()

    def decode_low_energy_states(self, max_dEng=0., max_states=1024):
        """Turn the recorded excitation forest into explicit states, lowest energies first (tnac4o.py:1360-1389).
        Replaces energy / states by the decoded spectrum; returns the lowest excitation energy (0)."""
        from . import droplets
        enc = getattr(self, 'excitations_encoding', 1)
        if enc == 1:
            E, st = droplets.decode_states(self.states[0], self.el, self.d, self.Nx_model * self.Ny_model, max_dEng,
                                           max_states, self.indtype)
        else:
            E, st = droplets.decode_states_adjacent(self.states[0], self.el, self.d, self._conn, max_dEng, max_states,
                                                    self.indtype, one_layer=(enc == 3))
        self.energy = E + self.energy[0]
        self.states = st
        return E[0]

    def search_ground_state(self, M=2 ** 10, relative_P_cutoff=1e-6, min_dEng=1e-12, graduate_truncation=True,
                            Dmax=32, tolS=1e-16, tolV=1e-10, max_sweeps=20, trace=None, beam_group=None, recorder=None):
        """Row-major branch-and-bound for the most probable configuration (tnac4o.py:381-551).  Results are stored in
        energy, degeneracy, states, probability (log2), discarded_probability, negative_probability.
        ``recorder`` (droplets.ExcitationRecorder): told about every merge (search_low_energy_spectrum).
        ``trace`` (a list) receives (ny, nx, Pn table, minPn, vind) of every site-step when given (parity tests).
        ``beam_group`` (a torch.distributed group): the ranks of the group work on this one solve together -- the first
        computes the sweep, every site-step's branches are split between them (parallel.gather_branch_tables) and each
        rank ends with the complete, identical result."""
        from . import parallel
        self.logger.info('Searching ground state with beta = %.2f', self.beta)
        kw_sweep = _sweep_options(graduate_truncation, Dmax, tolS, tolV, max_sweeps)
        # the PEPS factor of a cell (K7) serves the row MPO of the sweep and, unchanged, the conditional tables of the search: kept
        # between the two for the duration of this call (134 MB at L = 2048) instead of being rebuilt
        self._factor_keep = {}
        try:
            return self._search_ground_state(M, relative_P_cutoff, min_dEng, kw_sweep, trace, beam_group, recorder)
        finally:
            self._factor_keep = None

    def _search_ground_state(self, M, relative_P_cutoff, min_dEng, kw_sweep, trace, beam_group, recorder):
        from . import parallel
        if beam_group is None:
            self._setup_rhoT(**kw_sweep)
        else:
            self._setup_rhoT_shared(beam_group, **kw_sweep)
        # TN_BEAM: 'device' (default) = the beam step resident on the GPU (tn_beam_search / tnac4o_amd/beam.py); 'host' = the same canonical order
        # with the bookkeeping in numpy (used whenever a droplet recorder or a trace wants the intermediate tables on the host);
        # 'numpy' = the host path in numpy's own (unspecified) argpartition / argsort order, as the reference happens to run
        beam_mode = os.environ.get('TN_BEAM', 'device')
        if beam_mode == 'device' and recorder is None and trace is None:
            from . import beam
            # the whole loop in the library: tn_beam_search for one rank on the rotation, tn_beam_search_team for a beam group (the
            # conditional tables of a site-step split over its ranks, completed through torch.distributed).  A site-step at which NO candidate passes the cut-off (every log2 p is -inf or
            # NaN: a degenerate contraction) is not handled on the device: the search is redone on the host path, which keeps the single
            # best candidate there like the reference's keep = max(count, 1) (tnac4o.py:460-462).
            try:
                if beam.NATIVE_BEAM and not (beam_group is not None and os.environ.get('TN_BEAM_TEAM', 'native') == 'torch'):
                    # (a beam group walks the search in the library too: tn_beam_search_team with the site-steps' conditional tables
                    #  split over the ranks; TN_BEAM_TEAM=torch keeps the torch driver with its pruned candidate exchange)
                    E = beam.search_native(self, M, relative_P_cutoff, min_dEng, beam_group=beam_group)
                    if E is not None:
                        return E
                return beam.search_device(self, M, relative_P_cutoff, min_dEng, beam_group=beam_group)
            except beam.NoCandidate:
                if beam_group is not None:
                    raise
                self.logger.warning('beam search: no candidate passed the cut-off at some site; redoing the search on the host path')
        canonical = beam_mode != 'numpy'
        Nx, Ny = self.Nx, self.Ny
        vind = np.zeros((1, Nx + 1), dtype=self.indtype)
        states = np.zeros((1, Nx * Ny), dtype=self.indtype)
        Eng, prob, deg = np.zeros(1), np.zeros(1), np.ones(1, dtype=int)
        pd_max, globalmin = -np.inf, 0.0

        for ny in range(Ny):
            self.logger.info('Row %d / %d', ny + 1, Ny)
            walk = _RowWalk(self, vind, ny)
            for nx in range(Nx):
                q, nb = int(self.N[ny][nx]), prob.size
                T1, RR, F, dmap, rmap, pref, suf = walk.site(nx, vind)
                def pn_slice(lo, hi):                                        # K8 on the branches lo..hi-1
                    if not canonical:
                        return ops.calc_pn(T1, RR, F, dmap, rmap, _dev_i32(pref[lo:hi]), _dev_i32(suf[lo:hi]),
                                           _dev_i32(vind[lo:hi, nx]), _dev_i32(vind[lo:hi, nx + 1]))
                    # canonical order: the expanded log-probabilities come from the same launch (the device's log2, so that
                    # this path and tnac4o_amd.beam see the same bits); they ride behind the table
                    P, mP_, LP = ops.calc_pn(T1, RR, F, dmap, rmap, _dev_i32(pref[lo:hi]), _dev_i32(suf[lo:hi]), _dev_i32(vind[lo:hi, nx]),
                                             _dev_i32(vind[lo:hi, nx + 1]), parent_log2p=_dev_f64(prob[lo:hi]))
                    return torch.cat([P, LP], dim=1), mP_
                newprob, mP = parallel.gather_branch_tables(pn_slice, nb, q if not canonical else 2 * q, beam_group)
                minprob = float(mP.min())
                if canonical:
                    newprob, logp = np.ascontiguousarray(newprob[:, :q]), np.ascontiguousarray(newprob[:, q:])
                if trace is not None:
                    trace.append((ny, nx, newprob.copy(), mP.copy(), vind.copy()))

                if canonical:
                    prob = logp.reshape(nb * q)
                else:
                    with np.errstate(divide='ignore'):
                        newprob = np.log2(newprob)
                    newprob += prob[:, None]
                    prob = newprob.reshape(nb * q)

                order = np.arange(prob.size)
                if relative_P_cutoff > 0:                                    # tnac4o.py:458-465
                    cutoff = np.max(prob) + np.log2(relative_P_cutoff)
                    keep = max(int((prob > cutoff).sum()), 1)
                    if keep < prob.size:
                        if canonical:                                        # ascending flat index; the largest value cut
                            kept = prob > cutoff
                            if not kept.any():                               # all -inf / NaN: the single best, as keep = 1 does in the reference
                                kept[int(np.argmax(prob))] = True
                            order = np.flatnonzero(kept)
                            pd_max = max(pd_max, float(np.max(prob[~kept])))
                        else:
                            order = prob.argpartition(-keep - 1)
                            pd_max = max(pd_max, prob[order[-keep - 1]])
                            order = order[-keep:]
                        prob = prob[order]

                inds, indc = order // q, np.mod(order, q)                    # tnac4o.py:469-478
                states = states[inds]
                states[:, ny * Nx + nx] = indc
                vind = vind[inds]
                deg = deg[inds]
                vind[:, nx] = self._ind_bond_down(indc, ny, nx)
                vind[:, nx + 1] = self._ind_bond_right(indc, ny, nx)
                Eng = Eng[inds]
                Eng += self._update_Eng(states, ny, nx)

                vindn, inv = _unique_rows(vind)                              # merge equal boundaries (:481-515)
                indn, degn, probn, gorder, gstarts = _merge_groups(inv, Eng, prob, deg, min_dEng, canonical=canonical)
                sel = None
                if probn.size > M:                                           # keep the M most probable (:518-526)
                    if canonical:                                            # ties to the smaller group index; survivors in group order
                        srt = np.argsort(-probn, kind='stable')
                        pd_max = max(pd_max, probn[srt[M]])
                        sel = np.sort(srt[:M])
                    else:
                        sel = probn.argpartition(-M - 1)
                        pd_max = max(pd_max, probn[sel[-M - 1]])
                        sel = sel[-M:]
                if recorder is not None:                                     # droplets of the merged-away branches
                    recorder.merge_step(ny * Nx + nx, inds, gorder, gstarts, Eng, prob, states, indn, probn,
                                        np.arange(probn.size) if sel is None else sel)
                vind, prob, deg = vindn, probn, degn
                states, Eng = states[indn], Eng[indn]
                if sel is not None:
                    vind, states, prob, Eng, deg = vind[sel], states[sel], prob[sel], Eng[sel], deg[sel]

                walk.advance(nx, vind)
                globalmin = min(globalmin, minprob)

            if recorder is not None and hasattr(recorder, 'end_row'):
                recorder.end_row()
            walk.end_row(vind)

        return self._store_result(Eng, states, prob, deg[0], pd_max, globalmin)

    def _store_result(self, energy, states, probability, degeneracy, discarded, globalmin):
        """The result attributes of a walk (search or sampling): `states` arrive in the cell order of the current rotation and
        are stored in model order; globalmin is the smallest conditional probability met.  Returns the energies."""
        self.energy = energy
        self.degeneracy = degeneracy
        self.states = states[:, self.order]
        self.probability = probability
        self.discarded_probability = discarded
        self.negative_probability = min(globalmin, 0)
        return energy

    def gibbs_sampling(self, M=2 ** 10, graduate_truncation=True, Dmax=32, tolS=1e-15, tolV=1e-10, max_sweeps=20):
        """Draw M configurations from the Boltzmann distribution, cell by cell from the conditional probabilities of the
        boundary-MPS contraction (tnac4o.py:553-650).  Uses numpy's global generator like the reference (np.random.rand,
        one vector of M numbers per cell), so a seeded run draws the same configurations.  Stores energy (M,), states
        (M, Nx*Ny), negative_probability; returns the sampled energies."""
        self.logger.info('Sampling with beta = %.2f', self.beta)
        self._setup_rhoT(graduate_truncation=graduate_truncation, Dmax=Dmax, tolS=tolS, tolV=tolV, max_sweeps=max_sweeps)
        Nx, Ny = self.Nx, self.Ny
        vind = np.zeros((M, Nx + 1), dtype=np.int64)           # plain ints here, as in the reference (:584-585)
        states = np.zeros((M, Nx * Ny), dtype=np.int64)
        Eng = np.zeros(M)
        globalmin = 1.0
        for ny in range(Ny):
            self.logger.info('Row %d / %d', ny + 1, Ny)
            walk = _RowWalk(self, vind, ny)
            for nx in range(Nx):
                # distinct boundary configurations only (the reference's `seen` dictionary, :601-612)
                uvind, uinv = _unique_rows(vind)
                T1, RR, F, dmap, rmap, pref, suf = walk.site(nx, uvind)
                P, mP = ops.calc_pn(T1, RR, F, dmap, rmap, _dev_i32(pref), _dev_i32(suf), _dev_i32(uvind[:, nx]),
                                    _dev_i32(uvind[:, nx + 1]))
                newprob = P.cpu().numpy()[uinv]
                minprob = float(mP.min().item())
                newprob = newprob.cumsum(axis=1)                             # :616-622
                rr = np.random.rand(M)
                indc = np.array([np.searchsorted(newprob[kk], rr[kk]) for kk in range(M)], dtype=np.int64)
                states[:, ny * Nx + nx] = indc
                vind[:, nx] = self._ind_bond_down(indc, ny, nx)
                vind[:, nx + 1] = self._ind_bond_right(indc, ny, nx)
                Eng += self._update_Eng(states, ny, nx)
                walk.advance(nx, vind)                                       # left environments (:628-636)
                globalmin = min(globalmin, minprob)
            walk.end_row(vind)
        return self._store_result(Eng, states, np.zeros(1), 0, 0, globalmin)

    def sample_boltzmann(self, M=2 ** 16, Dmax=32, tolS=1e-15, tolV=1e-10, max_sweeps=20, graduate_truncation=True, uniforms=None,
                         chunk=None, seed=None):
        """Draw M configurations from the Boltzmann distribution with the library's sampling walk (tn_gibbs_sample): the draws of
        gibbs_sampling -- a seeded run draws the same configurations -- without the host round trips per cell, and with the
        probability each configuration was drawn with.  Works in the rotation that is set, Ising and RMF.
        uniforms: None = np.random.rand(Ny*Nx, M) from numpy's global generator (the stream gibbs_sampling's one rand(M) per cell
        consumes), or a (Ny*Nx, M) float64 array / device tensor of numbers in [0, 1), row = cell in walk order of the current
        rotation, column = sample; anything else is a ValueError.  chunk: samples per call of the walk (default: the largest power
        of two <= M whose workspace fits half of the free device memory); sample k's result does not depend on it.
        seed: None, or an integer in [0, 2^64) (not a bool; not together with uniforms: ValueError): the numbers come from the
        library's counter-based generator (tnac4o_amd/rng.py), filled on the device slice by slice -- number (cell k,
        sample m) is U(seed, stream of (walk, k), m), so sample m does not depend on M or chunk, and nothing is drawn on the host.
        The same seed gives the same numbers in every call, as the same uniforms would: vary the seed.
        Stores energy (M,), states (M, Nx*Ny) in model cell order, degeneracy = 0, probability (M,) = log2 q(x) of every sample,
        discarded_probability = 0, negative_probability, and the estimates of the partition function that follow from q
        (tnac4o_amd/sampler.py): sample_log2Z (M,) = -beta energy / ln 2 - probability, the same number log2 Z for every sample when
        the contraction is exact; log2Z_lower = its mean (<= log2 Z in expectation), log2Z_estimate = log2 mean 2^sample_log2Z.
        Z is the partition function over the ACTIVE spins: a spin without any term is not part of the network and would add
        exactly 1 to log2 Z.  Raises NotImplementedError naming the limit when a cell does not fit the walk; there is no host
        fallback.  Returns the sampled energies."""
        from . import rng, sampler
        if int(M) < 1:
            raise ValueError('M must be positive')
        seed = rng.check_seed_alone(seed, uniforms)
        if seed is None:
            uniforms = sampler.check_uniforms(uniforms, self.Nx * self.Ny, int(M))   # (before any device work)
        if chunk is not None:
            sampler.chunk_slices(int(M), chunk)
        self.logger.info('Sampling (library walk) with beta = %.2f', self.beta)
        self._setup_rhoT(graduate_truncation=graduate_truncation, Dmax=Dmax, tolS=tolS, tolV=tolV, max_sweeps=max_sweeps)
        return sampler.sample_native(self, int(M), uniforms=uniforms, chunk=chunk, seed=seed)

    def _cell_sizes(self):
        """Number of states of every cell of the rotated lattice, row-major (host)."""
        if self.mode == 'Ising':
            return np.array([2 ** int(self.sN[ny][nx]) for ny in range(self.Ny) for nx in range(self.Nx)], dtype=np.int64)
        return np.array([int(self.N[ny][nx]) for ny in range(self.Ny) for nx in range(self.Nx)], dtype=np.int64)

    def calculate_log_probability(self, states=None, boundary='build', cells=False, Dmax=32, tolS=1e-15, tolV=1e-10, max_sweeps=20,
                                  graduate_truncation=True, chunk=None):
        """log2 q(x) of GIVEN configurations: the probability with which the sampling walk of sample_boltzmann would draw each of
        them, from the library's walk forced along them (tn_gibbs_score) -- for a configuration sample_boltzmann drew on the same
        boundaries, the very bits of its `probability` and `energy`.  q is a normalised distribution for any truncation; with
        calculate_free_energy, log2 q(x) + beta E(x) / ln 2 + log2 Z is the pointwise truncation error.
        states: an integer numpy array (M, Nx*Ny) in model cell order, in the encoding of `states` (spin read-outs of an Ising
        model: states_from_binary); None = the stored `states`.  A wrong shape or dtype, or an entry outside the states of its cell,
        is a ValueError raised before any device work.  boundary: 'build' runs the sweep for rhoT with the given options, 'keep'
        uses rhoT as it stands (ValueError when there is none).  chunk: configurations per call of the walk, as sample_boltzmann's.
        Stores scored_log2q (M,) (returned), scored_energy (M,) in the convention of `energy`, scored_negative (<= 0, the smallest
        conditional-table flag met) and, with cells=True, scored_cell_log2q (M, Nx*Ny) in model cell order, the log2 of the
        conditional probability the walk used at every cell (None otherwise).  A configuration with a conditional probability that is
        not positive scores -inf, never NaN.  Leaves states, energy, probability and every other search and sampling result alone.
        Raises NotImplementedError naming the limit when a cell does not fit the walk; there is no host fallback."""
        from . import sampler
        if boundary not in ('build', 'keep'):
            raise ValueError("boundary must be 'build' or 'keep'")
        st = sampler.check_states(self.states if states is None else states, self._cell_sizes()[self.order])
        if chunk is not None:
            sampler.chunk_slices(st.shape[0], chunk)
        if boundary == 'keep' and getattr(self, 'rhoT', None) is None:
            raise ValueError("boundary='keep' needs rhoT: run a search, a sampling or a thermal call first, or use boundary='build'")
        self.logger.info('Scoring %d configurations with beta = %.2f', st.shape[0], self.beta)
        if boundary == 'build':
            self._setup_rhoT(graduate_truncation=graduate_truncation, Dmax=Dmax, tolS=tolS, tolV=tolV, max_sweeps=max_sweeps)
        rot = np.empty_like(st)
        rot[:, self.order] = st                                  # the inverse of _store_result's states[:, order]
        log2q, energy, cell_lq, globalmin, _ = sampler.score_native(self, rot, chunk=chunk, cells=cells)
        self.scored_log2q, self.scored_energy = log2q, energy
        self.scored_cell_log2q = cell_lq[:, self.order] if cells else None
        self.scored_negative = min(globalmin, 0)
        return log2q

    def relax_samples(self, sweeps=1, mode='heat_bath', beta=None, states=None, uniforms=None, chunk=None, max_sweeps=64, seed=None):
        """Move configurations by sweeps of block updates of whole cells (tn_cell_sweep, tnac4o_amd/relax.py): every cell in turn --
        checkerboard colour ny + nx even first, then odd -- is given a new state from its conditional law given its four neighbours,
        a table of q numbers read off the cell energies.  Runs NO contraction and needs no boundary MPS; works in the rotation that
        is set, Ising and RMF.
        mode='heat_bath': the new state is drawn from the conditional Boltzmann law at `beta` (None = the solver's).  A sweep leaves
        the Boltzmann law invariant, so sweeps started from the samples of sample_boltzmann at a cheap Dmax can only bring their law
        closer to it.  uniforms: None = np.random.rand(sweeps, Ny*Nx, M), or a (sweeps, Ny*Nx, M) float64 array / device tensor in
        [0, 1): sweep, cell in walk order of the current rotation, sample; anything else is a ValueError.  seed: None, or an integer in
        [0, 2^64) as sample_boltzmann's (not with uniforms, not with mode='quench': ValueError): the numbers are filled on the device
        slice by slice, number (sweep j, cell k, configuration m) is U(seed, stream of (relax sweep, j Ny*Nx + k), m) -- configuration
        m's result depends neither on chunk nor on how many configurations follow it.  The same seed gives the same numbers in every
        call: vary it.
        mode='quench': every cell goes to the smallest state of minimal conditional energy when that lowers the energy strictly, and
        stays otherwise (zero-temperature descent; the energy never rises).  sweeps=None repeats sweeps until no cell of any
        configuration moves in the last one, at most max_sweeps; uniforms must be None.
        states: an integer numpy array (M, Nx*Ny) in model cell order, in the encoding of `states` (spin read-outs or annealer
        output: states_from_binary); None = the stored `states`.  A wrong shape or dtype, or an entry outside the states of its cell,
        is a ValueError raised before any device work.  chunk: configurations per call, as sample_boltzmann's; configuration k's
        result does not depend on it.
        Stores states (M, Nx*Ny) in model cell order and energy (M,) (returned), relax_energy_before (M,), relax_moves (M,) = cell
        updates that changed the configuration, relax_converged (M,) bool = nothing moved in the last sweep (meaningful for a quench:
        a minimum under the cell moves), relax_sweeps = sweeps run.  probability, sample_log2Z, log2Z_lower and log2Z_estimate are
        set to None: the configurations are no longer draws of q -- calculate_log_probability() gives log2 q of the new states.
        rhoT, degeneracy and every thermal and scored attribute are left alone."""
        from . import relax, rng, sampler
        lib_mode, nsw, b = relax.check_relax_arguments(mode, sweeps, self.beta if beta is None else beta, uniforms, max_sweeps, seed)
        seed = rng.check_seed(seed)
        st = sampler.check_states(self.states if states is None else states, self._cell_sizes()[self.order])
        M = st.shape[0]
        if lib_mode == 0 and seed is None:
            uniforms = relax.check_sweep_uniforms(uniforms, nsw, self.Nx * self.Ny, M)
        if chunk is not None:
            sampler.chunk_slices(M, chunk)
        self.logger.info('Relaxing %d configurations (%s) with beta = %.2f', M, mode, b)
        rot = np.empty_like(st)
        rot[:, self.order] = st                                  # the inverse of _store_result's states[:, order]
        new, energy, before, moves, last, swept = relax.relax_native(self, rot, lib_mode, b, nsw, uniforms=uniforms, chunk=chunk,
                                                                     max_sweeps=max_sweeps, seed=seed)
        self.states = new[:, self.order]
        self.energy = energy
        self.relax_energy_before, self.relax_moves = before, moves
        self.relax_converged = (last == 0) & (swept > 0)
        self.relax_sweeps = int(swept)
        self.probability = self.sample_log2Z = self.log2Z_lower = self.log2Z_estimate = None
        return energy

    def relax_lines(self, sweeps=1, mode='heat_bath', lines='both', beta=None, states=None, uniforms=None, chunk=None, max_sweeps=64, seed=None):
        """Move configurations by EXACT updates of whole lattice rows and columns (tn_line_sweep, tnac4o_amd/lines.py): with
        the rows above and below given a row is a chain of cells, so its conditional law is sampled exactly by one forward pass of
        messages and one backward pass of draws, and its conditional minimum found by the same recursion in (min, +); a column
        likewise.  The move flips droplets that span a line, which no sequence of cell moves of relax_samples does at low
        temperature.  Runs NO contraction and needs no boundary MPS; works in the rotation that is set, Ising and RMF.  Arguments,
        storage and side effects are relax_samples'; the differences:
        lines: 'rows' -- a sweep is one row pass: the rows of even ny, then those of odd ny --, 'columns' -- the columns of even nx,
        then odd --, or 'both': a row pass, then a column pass (P = 2 passes per sweep, else P = 1).  Anything else: ValueError.
        mode='heat_bath': every line is drawn from its conditional Boltzmann law at `beta`; a sweep leaves the Boltzmann law
        invariant.  uniforms: None = np.random.rand(sweeps, P, Ny*Nx, M), or a (sweeps, P, Ny*Nx, M) float64 array / device tensor in
        [0, 1): sweep, pass, cell in walk order of the current rotation, sample.  seed: the numbers are filled on the device, number
        (sweep j, pass p, cell k, configuration m) is U(seed, stream of (relax line, (j P + p) Ny*Nx + k), m).  The heat bath works in
        the linear domain and is safe while beta (max - min) <= 300 for every chain table (the cell's coupling table to its left
        neighbour for rows, to its upper neighbour for columns): beyond that a ValueError naming the range guard is raised before any
        device work.
        mode='quench': a line goes to its conditional minimum -- ties to the minimiser that is smallest from the far end of the line
        -- when that lowers the energy strictly, and stays otherwise; the energy never rises.  sweeps=None repeats sweeps until no
        line of any configuration moves in the last one, at most max_sweeps: the result is a minimum against every change confined
        to one row or one column (with lines='both'), in particular a fixed point of relax_samples' cell quench.
        Stores states, energy (returned), relax_energy_before, relax_moves (M,) = the cells whose state changed, relax_converged,
        relax_sweeps; probability, sample_log2Z, log2Z_lower and log2Z_estimate are set to None."""
        from . import lines as ln, rng, sampler
        lib_mode, lib_lines, nsw, b = ln.check_line_arguments(mode, lines, sweeps, self.beta if beta is None else beta, uniforms, max_sweeps, seed)
        seed = rng.check_seed(seed)
        st = sampler.check_states(self.states if states is None else states, self._cell_sizes()[self.order])
        M = st.shape[0]
        if lib_mode == 0:
            if seed is None:
                uniforms = ln.check_line_uniforms(uniforms, nsw, ln.passes(lines), self.Nx * self.Ny, M)
            ln.check_range_guard(self, lines, b)
        if chunk is not None:
            sampler.chunk_slices(M, chunk)
        self.logger.info('Relaxing %d configurations by lines (%s, %s) with beta = %.2f', M, mode, lines, b)
        rot = np.empty_like(st)
        rot[:, self.order] = st                                  # the inverse of _store_result's states[:, order]
        new, energy, before, moves, last, swept = ln.lines_native(self, rot, lib_mode, lib_lines, b, nsw, uniforms=uniforms, chunk=chunk,
                                                                  max_sweeps=max_sweeps, seed=seed)
        self.states = new[:, self.order]
        self.energy = energy
        self.relax_energy_before, self.relax_moves = before, moves
        self.relax_converged = (last == 0) & (swept > 0)
        self.relax_sweeps = int(swept)
        self.probability = self.sample_log2Z = self.log2Z_lower = self.log2Z_estimate = None
        return energy

    def exchange_clusters(self, rounds=1, pairs=None, uniforms=None, seed=None):
        """Move the stored configurations by isoenergetic cluster moves on pairs of them (Houdayer's move in its form for arbitrary
        graphs; tn_cluster_exchange, tnac4o_amd/exchange.py): for a pair of replicas a, b one of the spins in which they differ is
        picked at random, and the connected cluster of differing spins that contains it -- connected along the couplings of J -- is
        flipped in both.  Ising only (RMF: ValueError); needs at least two stored states; runs no contraction, needs no boundary
        MPS and does not depend on the rotation (the bits are in model order).
        The move is rejection-free and its own inverse with the same selection probability, so it leaves the law of a pair
        invariant WHEN THE STORED STATES ARE SAMPLES AT ONE COMMON TEMPERATURE (sample_boltzmann, relax_samples in heat-bath mode);
        alternated with relax_samples it is the usual ergodic combination.  It conserves E_a + E_b, fields included, and the
        partners' overlap q_ab (the set of differing spins stays as it is).  A cluster that equals ALL the differing spins merely
        swaps the two replicas: that is common at high temperature on these graphs, where the differing spins percolate.  Between
        two quenched states the move is an energy-conserving recombination: relax_samples(mode='quench', sweeps=None) after it can
        leave minima the cell quench alone cannot.
        rounds: rounds of moves; in a round every state is in at most one pair.  pairs: None = for each round
        np.random.permutation(M)[:2 P].reshape(P, 2) with P = M // 2 from numpy's global generator, or an integer numpy array
        (rounds, P, 2) of indices into `states`, none twice within a round.  uniforms: None = np.random.rand(rounds, P), or a
        (rounds, P) float64 array / device tensor in [0, 1): pair p of a round with cnt differing spins takes the
        min(floor(u cnt), cnt - 1)-th of them in model order as its seed.  Every pairing is drawn before any uniform; anything else
        is a ValueError raised before any device work.  seed: None, or an integer in [0, 2^64) as sample_boltzmann's (not with
        uniforms: ValueError): the seeds' numbers are filled on the device, number (round r, pair p) is U(seed, stream of (exchange
        seed, r), p); with pairs=None the pairing of round r is the first 2 P entries of the stable ascending argsort of the keys
        U(seed, stream of (exchange pairing, r), m), m < M, computed on the host; explicit pairs are allowed, only the uniforms then
        come from the generator.  numpy's global generator is not touched.  The same seed gives the same numbers in every call: vary it.
        Stores states (M, Nx*Ny) in model cell order, energy (M,) in the bits relax_samples and scored_energy produce,
        exchange_energy_before (M,), exchange_pairs (rounds, P, 2), exchange_cluster_sizes (rounds, P) (returned; 0 = the partners
        were equal) and exchange_differing (rounds, P) = the spins in which the partners differ.  probability, sample_log2Z,
        log2Z_lower and log2Z_estimate are set to None, as relax_samples does.  rhoT, degeneracy and every thermal and scored attribute
        are left alone.  More than 65534 active spins: NotImplementedError; there is no host fallback."""
        from . import exchange
        return exchange.exchange_clusters(self, rounds, pairs, uniforms, seed)

    def calculate_droplets(self, reference=None, max_droplets=64, labels=False, states=None, chunk=None):
        """Decompose configurations into their droplets relative to a reference state (tn_droplets, tnac4o_amd/droplets_of_states.py;
        DESIGN §23): the spins in which a state differs from the reference fall into connected clusters -- connected along the
        couplings of J --, and each cluster is one excitation of the reference, with a size and an excitation energy
        dE = E(reference with the cluster flipped) - E(reference) in the convention of auxx.energy_Jij.  The droplets of a state do not
        touch one another, so their energies add up to E(state) - E(reference).  Ising only (RMF: ValueError); runs no contraction,
        needs no boundary MPS and does not depend on the rotation (spins are in model order).
        reference: None = the stored state of lowest `energy` (the first on ties); an integer = that stored state; an integer numpy
        array of length L = bits as a row of binary_states() holds them (what the inactive spins hold is ignored).  states: None = the
        stored states, or an integer array (M, Nx*Ny) of cell states in model cell order, as relax_samples takes them.  max_droplets =
        K: the droplets recorded per state, the first K by ascending root (the smallest spin of a droplet); everything that is not
        per droplet counts ALL droplets.  chunk: states per library call (None: what fits half of the free device memory).  Anything
        else is a ValueError raised before any device work.
        Stores droplet_count (M,) (returned), droplet_hamming (M,) = the differing spins, droplet_largest (M,), droplet_energy_total
        (M,) = the sum of dE over all droplets of a state; droplet_roots, droplet_sizes, droplet_energies (M, K): roots are model spin
        indices, the slots behind a state's droplets hold -1, 0, 0.0; droplet_size_counts (n + 1,) int64, entry s = the droplets of s
        spins over all states, n = the active spins; droplet_truncated = the states with more than K droplets; droplet_reference (L,)
        bits (0 at inactive spins) and droplet_reference_energy; droplet_labels (M, L) int32 with labels=True -- the number of the
        droplet that holds a spin, -1 for a spin that equals the reference or is inactive --, else None.
        `states`, `energy` and everything else the solver holds are left alone.  Couplings that are exactly summable (integers) give
        exact energies; otherwise the order of the additions is fixed by the inputs alone: the result does not depend on chunk.
        More than 65534 active spins: NotImplementedError; there is no host fallback."""
        from . import droplets_of_states
        return droplets_of_states.droplets_of_states(self, reference, max_droplets, labels, states, chunk)

    def calculate_state_linkage(self, threshold=None, kind=None, symmetric=None, states=None):
        """Single-linkage hierarchical clustering of the configurations by Hamming distance (tn_state_linkage,
        tnac4o_amd/linkage.py): which of the M states belong together, how many valleys there are, how big they are and
        at what distance they merge.  The dendrogram is the minimum spanning tree of the complete graph on the states under the strict
        total order key(a, b) = (d(a, b), min(a, b), max(a, b)); cut at height t it gives the connected components of "differ in at
        most t".  The device finds the tree (all pairs, Boruvka rounds, exact integers: the result does not depend on the grid or the
        run); runs no contraction.
        kind: 'spin' d = the active spins that differ (Ising only; RMF: ValueError); 'cell' d = the cells in another state (any
        mode); None = 'spin' for Ising, 'cell' for RMF.  symmetric: fold the distance, d' = min(d, N - d), so that a state and its
        global spin flip are one point; 'spin' only; None = True exactly when the model has no fields (the diagonal of J0 is zero).
        states: None = the stored states, or an integer array (M, Nx*Ny) of cell states in model cell order, as calculate_droplets
        takes them.  threshold: None or an integer t >= 0.  Anything else, and no stored states, is a ValueError raised before any
        device work.
        Stores linkage_pairs (M-1, 2) int64 = the edges (lo < hi) in ascending key order, linkage_distance (M-1,) int64 = the merge
        heights, ascending (returned); nearest_state, nearest_distance (M,) = for every state the b != a that minimises (d, b) (-1 for
        a single state); linkage_cluster_counts (N+1,) int64, entry t = the clusters when all pairs at distance <= t are joined;
        linkage_matrix (M-1, 4) float64 in the format of scipy's linkage (merge i creates cluster M + i, the smaller id first; for
        scipy's dendrogram and fcluster); linkage_kind, linkage_symmetric, linkage_rounds (the rounds the device needed).  With a
        threshold also state_cluster_labels (M,) (clusters numbered by their ascending smallest member), state_cluster_sizes,
        state_cluster_first, and, when `energy` has one entry per state, state_cluster_representative (the member of lowest energy,
        the first on ties) and state_cluster_energy_min, else None for both; without a threshold these five are None.
        More than 65534 spins (cells) or more than 2^24 states: NotImplementedError naming the limit; there is no host fallback.
        Changes nothing else."""
        from . import linkage
        return linkage.state_linkage(self, threshold, kind, symmetric, states)

    def temper_samples(self, betas, rounds=10, sweeps=1, cluster_moves=True, cluster_beta_min=None, pairs=None, uniforms=None, record=False,
                       keep=None, rounds_per_call=None, seed=None, measure=None, measure_from=0, measure_bins=16, measure_pairs='all',
                       measure_links=True):
        """Parallel tempering with isoenergetic cluster moves (PT+ICM: Zhu, Ochoa, Katzgraber) over the stored configurations, whole
        rounds on the device in one library call (tn_temper, tnac4o_amd/temper.py).  Runs NO contraction and needs no
        boundary MPS; the solver's own beta plays no part.
        Input: the stored `states`, M = R T of them with T = len(betas); betas strictly increasing, positive, finite.  Row m belongs to
        chain m // T and STARTS at temperature index m % T.  A round is: `sweeps` heat-bath sweeps of relax_samples' move with every row
        at the beta it holds; with cluster_moves, exchange_clusters' move between the rows of two chains at the same temperature,
        for every temperature with betas >= cluster_beta_min (None: all) and every chain pair of the round; then swaps of the
        temperature labels of neighbouring temperatures inside a chain (even pairs in even rounds, odd pairs in odd rounds),
        accepted with min(1, exp((beta_{t+1} - beta_t)(E_{t+1} - E_t))).  cluster_moves=True needs an Ising model (RMF: ValueError),
        R >= 2 and at most 65534 active spins; with cluster_moves=False pairs and cluster_beta_min must be None.
        Randomness.  pairs: None = a random perfect matching of the R chains per round (exchange.check_pairs over R), or an integer
        numpy array (rounds, Pc, 2) of chain indices, none twice within a round.  uniforms: None, or a dict with the three keys
        'sweep' (rounds, sweeps, Ny*Nx, M) -- round, sweep, cell in walk order of the CURRENT rotation, row --, 'cluster'
        (rounds, Tc, Pc) with Tc the number of temperatures that make cluster moves, and 'swap' (rounds, R, T - 1): float64 numpy
        arrays or device tensors in [0, 1).  With None they come from numpy's global generator: all pairings first, then block by
        block of rounds_per_call rounds in the order sweep, cluster, swap -- the generator's stream then depends on rounds_per_call,
        the law does not, and with given uniforms neither does the result.  rounds_per_call: rounds per library call (None: planned
        from the free device memory; the sweep's uniform numbers, rounds sweeps Nx Ny M 8 bytes, are the large item).  Everything is
        validated before any device work (ValueError).  seed: None, or an integer in [0, 2^64) as sample_boltzmann's (not with
        uniforms: ValueError): the three arrays are filled on the device block by block, every number a function of the seed and its
        logical position with r the GLOBAL round -- sweep (r, j, k, m): U(seed, stream of (temper sweep, (r sweeps + j) Ny*Nx + k), m);
        cluster (r, t', p): stream of (temper cluster, r Tc + t'), p; swap (r, c, t): stream of (temper swap, r R + c), t -- so the
        result depends on rounds_per_call no more than with given uniforms; with pairs=None the chain pairing of round r comes from
        the keys U(seed, stream of (temper pairing, r), c), c < R, by exchange_clusters' rule, on the host; explicit pairs are allowed.
        numpy's global generator is not touched.  The same seed gives the same numbers in every call: vary it.
        Stores states (M, Nx*Ny) in model cell order and energy (M,) (returned) in the bits relax_samples gives, temper_betas (T,),
        temper_index (M,) = the temperature index every row ends at, temper_beta (M,) = its beta, temper_swap_accepted and
        temper_swap_attempted (T - 1,) over all rounds.  With record=True also temper_energy_trace (rounds, T, R) = the energy at
        every temperature of every chain after each round, and temper_cluster_sizes, temper_cluster_differing (rounds, Tc, Pc).
        probability, sample_log2Z, log2Z_lower and log2Z_estimate are set to None, as relax_samples does.
        keep: None leaves a MIXED population in states / energy -- rows at all T temperatures, told apart by temper_index, which the
        calculate_overlap_* calls would pool; keep=t leaves only the R rows that end at temperature index t (chains ascending) in
        states and energy, so that those calls see one temperature (temper_index and temper_beta still describe all M rows).
        measure: None (nothing below happens or is stored), or a positive integer: overlap histograms at EVERY temperature, accumulated
        on the device between the blocks of rounds (tn_ladder_measure, tnac4o_amd/ladder.py; Ising only, R >= 2, at most
        38815 active spins and 38815 couplings, else NotImplementedError).  A measurement follows global round r, after its swaps,
        iff r >= measure_from and (r - measure_from + 1) % measure == 0: n_meas = (rounds - measure_from) // measure of them (none, a
        non-positive measure or a measure_from outside [0, rounds]: ValueError); measurement i goes to time bin i B // n_meas with
        B = min(measure_bins, n_meas).  The library calls are cut at the measurement rounds; states, energy, temper_index and the
        counters are the bits of the same call without measure (with uniforms=None the global generator's stream follows the cut, as
        it follows rounds_per_call).  A measurement counts, for every temperature t and every chain pair, the Hamming distance d of
        the two rows at t over the active spins (q = 1 - 2 d / n) and, with measure_links, over the couplings of overlap.link_pairs
        (q_l = 1 - 2 d_l / n_l).  measure_pairs='all': every pair of chains; 'halves': only pairs with one chain below R // 2 and one
        at or above it -- the two-sets convention of PT+ICM; with cluster moves the given pairs= must then stay inside the halves
        (ladder.pairs_in_halves draws such pairings), else ValueError.
        Stores temper_measurements = n_meas; temper_overlap_hist (B, T, n + 1) and temper_link_hist (B, T, n_l + 1) int64 pair counts
        per time bin, temper_overlap_values / temper_link_values, temper_overlap_P / temper_link_P (T, n + 1) / (T, n_l + 1) summed
        over the bins and normalised (the three link results are None with measure_links=False); temper_overlap_moments, a dict of
        (T,) arrays q, abs_q, q2, q4, binder, chi_sg (conventions of overlap_moments) and ql = the mean link overlap;
        temper_overlap_errors, the same keys from a delete-one-bin jackknife over the B time bins (NaN when B < 2);
        temper_energy_sums (B, T, 3) = measurements, sum E, sum E^2 over the R rows at each temperature, temper_energy_mean (T,),
        temper_heat_capacity (T,) = beta^2 (<E^2> - <E>^2) / n and temper_energy_mean_error, temper_heat_capacity_error from the same
        jackknife.  The jackknife assumes bins longer than the autocorrelation time; with 'all' under cluster moves the pairs of
        chains are not independent, which it does not see."""
        from . import temper
        return temper.temper_samples(self, betas, rounds, sweeps, cluster_moves, cluster_beta_min, pairs, uniforms, record, keep, rounds_per_call,
                                     seed, measure, measure_from, measure_bins, measure_pairs, measure_links)

    def anneal_population(self, betas, sweeps=1, M=None, uniforms=None, record=False, log2Z0=None, steps_per_call=None, seed=None):
        """Population annealing (Hukushima, Iba; Machta; Wang, Machta, Katzgraber): a population of M configurations is taken along the
        schedule `betas`, whole steps on the device in one library call (tn_anneal, tnac4o_amd/anneal.py), and log2 Z is
        estimated at every beta of the schedule.  Runs NO contraction and needs no boundary MPS; the solver's own beta plays no part;
        Ising and RMF.
        betas: K >= 1 finite numbers, betas[0] >= 0, strictly increasing.  betas[0] is the inverse temperature whose law the incoming
        population samples; no sweep is made at it.  M=None anneals the stored `states`, taken as samples at betas[0].  With M given,
        betas[0] must be 0 and the population is drawn uniformly on the host, state = min(floor(u q_k), q_k - 1) with q_k the states
        of cell k.  A step from beta' to beta weights row m with exp(-(beta - beta')(E_m - Emin)), resamples the population to exactly
        M rows by systematic resampling with one uniform number (row m gets floor or ceil of M w_m / W copies), and makes `sweeps`
        heat-bath sweeps of relax_samples' move at beta.
        Randomness.  uniforms: None, or a dict with the keys 'resample' (K - 1,) and 'sweep' (K - 1, sweeps, Ny*Nx, M) -- step, sweep,
        cell in walk order of the CURRENT rotation, row -- and, when M is given, 'init' (M, Ny*Nx), cells in that walk order too:
        float64 numpy arrays or device tensors in [0, 1).  With None they come from numpy's global generator: init first, then block
        by block of steps_per_call steps in the order resample, sweep -- the generator's stream then depends on steps_per_call, the
        law does not, and with given uniforms neither does the result.  steps_per_call: steps per library call (None: planned from
        half the free device memory; the sweep's uniform numbers are the large item).  Everything is validated before any device
        work (ValueError).  seed: None, or an integer in [0, 2^64) as sample_boltzmann's (not with uniforms: ValueError): every array
        is filled on the device, every number a function of the seed and its logical position with s the GLOBAL step -- init (m, k):
        U(seed, stream of (anneal init, m), k), and the fresh population is made on the device by the same rule; resample (s):
        stream of (anneal resample, 0), s; sweep (s, j, k, m): stream of (anneal sweep, (s sweeps + j) Ny*Nx + k), m -- so the result
        depends on steps_per_call no more than with given uniforms, and row m's numbers do not depend on M.  numpy's global generator
        is not touched.  The same seed gives the same numbers in every call: vary it.
        Stores states (M, Nx*Ny) in model cell order and energy (M,) (returned) in the bits relax_samples gives, and
        anneal_betas (K,);
        anneal_log2Z (K,) = log2Z0 plus the running sum of log2(W_s / M) - (betas[s] - betas[s-1]) Emin_s / ln 2.  log2 Z here means
          log2 sum_x exp(-beta E(x)) over ALL configurations x of the cell states, E in the convention of `energy`.  The cell states of
          an Ising model enumerate exactly its active spins (sum_k log2 q_k = their number), so this is the quantity
          calculate_free_energy and sample_log2Z give, with no constant between them.  log2Z0 = None: with betas[0] = 0 it is
          sum_k log2 q_k, the exact value; with betas[0] > 0 it is 0, and anneal_log2Z then holds the RATIOS log2 Z(beta) / Z(betas[0])
          (give log2Z0 = the log2 Z of the incoming law, e.g. calculate_free_energy's, for absolute values).  A step whose weights
          all vanish contributes -inf;
        anneal_free_energy (K,) = -ln Z / beta where beta > 0, NaN at beta = 0;
        anneal_energy_mean, anneal_heat_capacity (K,) = the mean of E and beta^2 var E (population variance) over the population at
          every beta, after its sweeps (at betas[0]: of the incoming population);
        anneal_ess (K - 1,) = W^2 / sum w^2, the effective sample size of every reweighting; anneal_survivors (K - 1,) = the rows
          that kept at least one copy;
        anneal_family (M,) = for every final row the index of the row of the incoming population it descends from;
        anneal_rho_t = M sum_f (n_f / M)^2 and anneal_family_entropy = -sum_f (n_f / M) ln(n_f / M) over the families (Wang, Machta,
          Katzgraber: rho_t << M is the condition for trusting the run);
        with record=True anneal_energy_trace (K - 1, M) = the energies after every step and anneal_parent_trace (K - 1, M) = the row
          every row was copied from in that step's resampling.
        probability, sample_log2Z, log2Z_lower and log2Z_estimate are set to None, as temper_samples does.  rhoT, degeneracy and every
        thermal and scored attribute are left alone."""
        from . import anneal
        return anneal.anneal_population(self, betas, sweeps, M, uniforms, record, log2Z0, steps_per_call, seed)

    # ------------------------------------------------------------------------------------ thermal marginals (GPU)
    def calculate_marginals(self, Dmax=32, tolS=1e-16, tolV=1e-10, max_sweeps=20, graduate_truncation=True):
        """Boltzmann marginal of every cell and magnetisation of every spin at the solver's beta, from both boundary MPS.
        Each row is contracted between rhoB[ny] and rhoT[ny+1] with one cell left open (tn_env3 / tn_cluster_marginal): exact
        up to the truncation of the boundaries.  Stores and returns `marginals` (a list over model cells, k = ny*Nx + nx, of
        float64 vectors over the cell's states in the encoding of `states[:, k]`); stores `magnetization` (L,) (Ising; None for
        RMF), `marginals_negative` (<= 0, the negative-probability measure of search_ground_state) and `marginal_row_log2`
        (Ny, Nx) in the rotated frame: log2 of each row's contraction, the same for every cell of a row.  Leaves the search
        results, gauges and rotation alone; rebuilds rhoT and rhoB."""
        kw = _sweep_options(graduate_truncation, Dmax, tolS, tolV, max_sweeps)
        self.logger.info('Marginals with beta = %.2f', self.beta)
        self._setup_rhoT(**kw)
        self._setup_rhoB(**kw)
        P_rot, minP, log2z = self._marginal_pass()
        self.marginal_row_log2 = log2z
        self.marginals_negative = min(float(minP.min()), 0.0)
        if self.mode == 'Ising':
            self.marginals, self.magnetization = model_marginals(P_rot, self.order, self.ind0, self.L)
        else:
            self.marginals, self.magnetization = model_marginals(P_rot, self.order)[0], None
        return self.marginals

    def _open_cell_pass(self, kernel):
        """Every row of the rotated lattice contracted between rhoB[ny] and rhoT[ny+1] as they stand, with one cell left open at
        a time.  Per row: the right environments with their half-products and running log2 factors from the right end (tn_env3),
        then the left sweep, calling kernel(HL, HR, F, dmap, rmap, log2L, log2R) -> device tensors at every cell; a cell's HR is
        dropped once its kernel is enqueued.  One read-back at the end.  Returns, for each output of the kernel, the list of the
        cells' host arrays (row-major)."""
        Nx = self.Nx
        dev = self.rhoT[0].A[0].device
        one = torch.ones((1, 1, 1), dtype=torch.float64, device=dev)
        zero = torch.zeros(1, dtype=torch.float64, device=dev)
        outs = []
        for ny in range(self.Ny):
            top, bot = self.rhoT[ny + 1].A, self.rhoB[ny].A
            fac = self._peps_factors_dev([(ny, nx) for nx in range(Nx)])
            Ws = [ops.mpo_from_factor(F, dm, rm, pd, br) for (F, dm, rm, pd, br) in fac]
            At = [a.contiguous() for a in top]
            Ab = [a.contiguous() for a in bot]
            ER, lgR, HR = one, zero, [None] * Nx
            lgRs = [None] * (Nx + 1)
            lgRs[Nx] = zero
            for nx in range(Nx - 1, -1, -1):
                ER, lgR, HR[nx] = ops.env3(1, ER, At[nx], Ws[nx], Ab[nx], lgR, keep_half=True)
                lgRs[nx] = lgR
            EL, lgL = one, zero
            for nx in range(Nx):
                F, dm, rm, _, _ = fac[nx]
                ELn, lgLn, HL = ops.env3(0, EL, At[nx], Ws[nx], Ab[nx], lgL, keep_half=True)
                outs.append(kernel(HL, HR[nx], F, dm, rm, lgL, lgRs[nx + 1]))
                HR[nx] = None
                EL, lgL = ELn, lgLn
        n = len(outs)
        host = _read_back([t for kind in zip(*outs) for t in kind])
        return [host[k:k + n] for k in range(0, len(host), n)]

    def _marginal_pass(self):
        """Cell marginals of the rotated lattice from rhoT / rhoB as they stand: _open_cell_pass with tn_cluster_marginal per cell.
        Returns (list of per-cell vectors, row-major; minP (Ny*Nx,); log2 row contractions (Ny, Nx))."""
        P_rot, minP, log2z = self._open_cell_pass(ops.cluster_marginal)
        return P_rot, np.concatenate(minP), np.concatenate(log2z).reshape(self.Ny, self.Nx)

    # ------------------------------------------------------------------------------------ thermal correlations (GPU)
    def calculate_correlations(self, Dmax=32, tolS=1e-16, tolV=1e-10, max_sweeps=20, graduate_truncation=True):
        """Nearest-neighbour correlations and the mean energy at the solver's beta, from both boundary MPS.  Each row is
        contracted between rhoB[ny] and rhoT[ny+1] with one cell left open, keeping the cell's state jointly with its left and
        upper bond index (tn_cluster_bond_marginal): exact up to the truncation of the boundaries.
          Ising: stores `bond_pairs` (n, 2), the model spins i < j of every off-diagonal J0[i, j] != 0 (sorted), and
          `correlations` (n,), <sigma_i sigma_j> with sigma = +1 where binary_states writes 1; returns `correlations`.
          RMF: stores `pair_marginals`, {two-cell factor key of the model: P[s1, s2] in the key's order}; returns it.
        Both store `energy_mean` (<E> in the convention of `energy`), `correlations_negative` (<= 0, the smallest table entry)
        and `correlation_row_log2` (Ny, Nx) in the rotated frame (log2 of each row's contraction, as marginal_row_log2).
        Leaves the search results, marginals, gauges and rotation alone; rebuilds rhoT and rhoB."""
        kw = _sweep_options(graduate_truncation, Dmax, tolS, tolV, max_sweeps)
        self.logger.info('Correlations with beta = %.2f', self.beta)
        self._setup_rhoT(**kw)
        self._setup_rhoB(**kw)
        Pl, Pu, minB, log2z = self._correlation_pass()
        self.correlation_row_log2 = log2z
        self.correlations_negative = min(float(minB.min()), 0.0)
        self.energy_mean = self._bond_energy(Pl, Pu)
        if self.mode == 'Ising':
            self.bond_pairs, self.correlations = model_correlations(Pl, Pu, self.order, self.Nx, self.Ny, J0=self.J0, ind=self.ind,
                                                                    ir=self.ir, idn=self.id)
            self.pair_marginals = None
            return self.correlations
        self.pair_marginals = model_correlations(Pl, Pu, self.order, self.Nx, self.Ny, keys=list(self.J['fac']), Nx_model=self.Nx_model)
        self.bond_pairs = self.correlations = None
        return self.pair_marginals

    # ------------------------------------------------------------------------------------ partition function (GPU)
    def calculate_free_energy(self, Dmax=32, tolS=1e-16, tolV=1e-10, max_sweeps=20, graduate_truncation=True, boundary='build'):
        """log2 Z, free energy and entropy at the solver's beta from both boundary MPS: the row contractions r_ny = <rhoB[ny]| row ny
        |rhoT[ny+1]> of calculate_correlations over the overlaps o_ny = <rhoB[ny]|rhoT[ny]> of the boundaries at the Ny - 1 cuts,
            log2 Z = sum_ny log2 |r_ny| - sum_ny log2 |o_ny| - (beta / ln 2) sum_cells (min Es + min E1 + min E4),
        the last term putting back what the PEPS factors take out of the energy tables.  Exact when nothing is truncated; otherwise
        an estimate that uses both boundaries symmetrically: the norm and sign of every interior boundary occur once above and once
        below the line.  Z runs over the ACTIVE spins, E in the convention of `energy`: the number sample_log2Z estimates.
        boundary: 'build' runs both sweeps with the given options, 'keep' uses rhoT and rhoB as they stand (ValueError when one is
        missing).  Stores log2Z (returned), free_energy = -ln Z / beta, entropy = ln Z + beta energy_mean (nats), energy_mean,
        log2Z_rows (Ny,) = log2 |r_ny| (taken at the first cell of the row), log2Z_overlaps (Ny-1,) = log2 |o_ny| and
        free_energy_row_spread: the largest deviation of the row contraction along a row, |log2 r at a cell - log2 r at the first| /
        max(|log2 r|, 1) -- every cell of a row contracts the same network, so this is rounding (1e-10 is the bar of the thermal
        calls).  Leaves the search results, gauges and rotation alone."""
        from . import sampler
        if boundary not in ('build', 'keep'):
            raise ValueError("boundary must be 'build' or 'keep'")
        if boundary == 'keep' and (getattr(self, 'rhoT', None) is None or getattr(self, 'rhoB', None) is None):
            raise ValueError("boundary='keep' needs rhoT and rhoB: run a thermal call first, or use boundary='build'")
        self.logger.info('Free energy with beta = %.2f', self.beta)
        if boundary == 'build':
            kw = _sweep_options(graduate_truncation, Dmax, tolS, tolV, max_sweeps)
            self._setup_rhoT(**kw)
            self._setup_rhoB(**kw)
        Ny, Nx = self.Ny, self.Nx
        Pl, Pu, _, log2r = self._correlation_pass()
        neg = np.flatnonzero(np.isnan(log2r).any(axis=1))
        if neg.size:
            # a row contraction below zero (a boundary that carries a sign; the kernel's log2 is NaN there): the same pass with the
            # sign taken out of the first site of a copy of the boundary above those rows
            kept = self.rhoT
            try:
                self.rhoT = list(kept)
                for ny in neg:
                    flipped = kept[ny + 1].copy()
                    flipped.A[0] = -flipped.A[0]
                    self.rhoT[ny + 1] = flipped
                Pl, Pu, _, log2r = self._correlation_pass()
            finally:
                self.rhoT = kept
        ends, o, log2o = self._boundary_overlaps()
        shifts = [[np.min(t) for t in self._cell_energies(ny, nx)] for ny in range(Ny) for nx in range(Nx)]
        self.log2Z, self.log2Z_rows, self.log2Z_overlaps = sampler.log2z_from_rows(
            np.ones(Ny), o, shifts, self.beta, rows_log2=log2r[:, 0], overlaps_log2=log2o, ends=ends)
        self.free_energy_row_spread = float(np.max(np.abs(log2r - log2r[:, :1]) / np.maximum(np.abs(log2r[:, :1]), 1.0)))
        self.energy_mean = self._bond_energy(Pl, Pu)
        lnZ = self.log2Z * sampler.LN2
        self.free_energy = -lnZ / self.beta
        self.entropy = lnZ + self.beta * self.energy_mean
        return self.log2Z

    def _boundary_overlaps(self):
        """The two-layer overlaps o_ny = <rhoB[ny]|rhoT[ny]> at the cuts ny = 1 .. Ny-1 from the boundaries as they stand, walked left
        to right on the device (tn_env_mix), every environment divided by a power of two (tn_normalize_pow2) so that no overlap of
        two different states has to stay inside the double range; and what the two trivial boundaries beyond the lattice, rhoB[0]
        and rhoT[Ny], contract to.  One read-back.  Returns ((e_B, e_T), mantissas (Ny-1,), log2 factors (Ny-1,)): o_ny =
        mantissa 2^factor."""
        Ny, Nx = self.Ny, self.Nx
        dev = self.rhoT[0].A[0].device
        outs = []
        for psi in (self.rhoB[0], self.rhoT[Ny]):
            if any(tuple(a.shape) != (1, 1, 1) for a in psi.A):
                raise ValueError('the boundary beyond the lattice must be the trivial one (d = 1, D = 1)')
            outs.append(torch.cat([a.reshape(-1) for a in psi.A]))
        for ny in range(1, Ny):
            E, nfs = torch.ones((1, 1), dtype=torch.float64, device=dev), []
            for nx in range(Nx):
                E = ops.env_mix(0, E, self.rhoT[ny].A[nx].contiguous(), self.rhoB[ny].A[nx].contiguous())
                nfs.append(ops.normalize_pow2_(E)[:1])
            outs += [E.reshape(-1), torch.cat(nfs)]
        host = _read_back(outs)
        ends = (float(np.prod(host[0])), float(np.prod(host[1])))
        o = np.array([host[2 + 2 * i][0] for i in range(Ny - 1)])
        log2o = np.array([np.sum(np.log2(host[3 + 2 * i])) for i in range(Ny - 1)])
        return ends, o, log2o

    def _bond_energy(self, Pl, Pu):
        """<E> = sum_k [sum_s p_k Es_k + sum_{s,l} Pl_k E1_k + sum_{s,u} Pu_k E4_k] from the bond tables of the rotated frame
        (p_k[s] = sum_l Pl_k[s, l]); the energy tables are those of _cell_energies, unshifted and unscaled (host)."""
        Em = 0.0
        for ny in range(self.Ny):
            for nx in range(self.Nx):
                c = ny * self.Nx + nx
                Es, E1, E4 = self._cell_energies(ny, nx)
                Em += float(Pl[c].sum(1) @ Es) + float(np.sum(Pl[c] * E1)) + float(np.sum(Pu[c] * E4))
        return Em

    def _correlation_pass(self):
        """Bond tables of the rotated lattice from rhoT / rhoB as they stand: _open_cell_pass with tn_cluster_bond_marginal per
        cell.  Returns (Pl list (q, bl), Pu list (q, pu), row-major over cells; minB (Ny*Nx,); log2 row contractions (Ny, Nx))."""
        Pl, Pu, minB, log2z = self._open_cell_pass(ops.cluster_bond_marginal)
        return Pl, Pu, np.concatenate(minB), np.concatenate(log2z).reshape(self.Ny, self.Nx)


    # ------------------------------------------------------------------------------------ in-line two-point functions (GPU)
    def calculate_correlation_function(self, max_distance=None, lines='both', Dmax=32, tolS=1e-16, tolV=1e-10, max_sweeps=20,
                                       graduate_truncation=True, slot_budget=None):
        """Two-point functions at the solver's beta between cells of one lattice row or column at every cell distance 1 ..
        max_distance (None: the whole line), from both boundary MPS: an operator is inserted into the left environment of the row
        network <rhoB[ny]| row ny |rhoT[ny+1]> at one cell, carried through ordinary environment steps and closed at another
        (tn_env3_stack / tn_stack_cell_law, all carried environments in one stack): exact up to the truncation of the boundaries.
        lines: 'rows' = pairs of cells in one row of the current frame, 'columns' = the same after rotate_graph(1), 'both'.
        slot_budget: bytes the stack and its products may take (default: half of the free device memory); a smaller budget walks
        the start cells in several left sweeps and changes the result by rounding only.
          Ising: stores `line_pairs` (n, 2) int64, the model spins i < j (sorted) of every pair of active spins in two different cells of
          one line within max_distance, `line_distance` (n,) their cell distance, `line_correlations` (n,) = <sigma_i sigma_j> with
          sigma = +1 where binary_states writes 1 (returned), and `line_magnetization` (L,) from the same networks (0 for inactive
          spins): the connected part is line_correlations - m[i] m[j].
          RMF: stores and returns `line_pair_marginals`, {(y1, x1, y2, x2) in model coordinates, first cell first in row-major order:
          P[s1, s2]}.
        Both store `line_negative` (<= 0: RMF the smallest joint entry, Ising min(0, min(1 - |C|))) and `line_row_log2` (Ny, Nx), log2
        of each row's contraction at every cell in the frame of the rows pass (of the columns pass for lines='columns').  Leaves the
        frame, rotation, order, gauges, boundaries, search results and the outputs of the other thermal calls alone."""
        if lines not in ('rows', 'columns', 'both'):
            raise ValueError("lines must be 'rows', 'columns' or 'both'")
        if max_distance is not None and (int(max_distance) != max_distance or max_distance < 1):
            raise ValueError('max_distance must be a positive integer or None')
        kw = _sweep_options(graduate_truncation, Dmax, tolS, tolV, max_sweeps)
        self.logger.info('Correlation functions with beta = %.2f', self.beta)
        names = ('rhoT', 'rhoT_overlap', 'rhoT_discarded', 'rhoB', 'rhoB_overlap', 'rhoB_discarded', 'Xu', 'Xd', 'Xl', 'Xr', 'overlaps_ud')
        saved = {k: getattr(self, k) for k in names if hasattr(self, k)}
        ising = self.mode == 'Ising'
        parts, law_frame = [], None
        try:
            for turned in ((True, False) if lines == 'both' else (lines == 'columns',)):       # columns first: rows end in the caller's frame
                if turned:
                    self.rotate_graph(1)
                try:
                    self._setup_rhoT(**kw)
                    self._setup_rhoB(**kw)
                    laws, joints, log2z = self._line_pass(max_distance, slot_budget)
                    if ising:
                        tables = {key: M @ self._line_operators(*divmod(key[1], self.Nx)).T for key, M in joints.items()}
                        parts.append(model_line_correlations(tables, self.order, self.Nx, ind=self.ind, Nc=self.Nc))
                    else:
                        parts.append(model_line_correlations(joints, self.order, self.Nx, Nx_model=self.Nx_model))
                    law_frame = (laws, self.order.copy(), log2z)
                finally:
                    if turned:
                        self.rotate_graph(3)
        finally:
            for k in names:
                if k in saved:
                    setattr(self, k, saved[k])
                elif hasattr(self, k):
                    delattr(self, k)
        laws, order, self.line_row_log2 = law_frame
        if ising:
            pairs = np.concatenate([p[0] for p in parts])
            dist, C = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
            idx = np.lexsort((pairs[:, 1], pairs[:, 0]))
            self.line_pairs, self.line_distance, self.line_correlations = pairs[idx], dist[idx], C[idx]
            self.line_magnetization = model_marginals(laws, order, self.ind0, self.L)[1]
            self.line_pair_marginals = None
            self.line_negative = min(0.0, float(np.min(1.0 - np.abs(C)))) if C.size else 0.0
            return self.line_correlations
        self.line_pair_marginals = {}
        for p in parts:
            self.line_pair_marginals.update(p)
        self.line_pairs = self.line_distance = self.line_correlations = self.line_magnetization = None
        self.line_negative = min([0.0] + [float(P.min()) for P in self.line_pair_marginals.values()])
        return self.line_pair_marginals

    def _line_operators(self, ny, nx):
        """Operator table O (nop, q) on the states of a cell of the rotated lattice: Ising one row sigma_a(s) per active spin (+1 where
        binary_states writes 1), RMF the q state indicators (the closing then yields the joint law)."""
        if self.mode == 'Ising':
            return np.ascontiguousarray(_spins(self.sN[ny][nx]).T, dtype=np.float64)
        return np.eye(int(self.N[ny][nx]))

    def _line_slot_bytes(self, ny):
        """Bytes one slot of the stack of row ny takes at its widest cell: the environment before and after the step, its two
        products and the closing's X (what slot_budget is divided by)."""
        need, bl = 0, 1
        for nx in range(self.Nx):
            (Dt, pd, Dt2), (Db, pu, Db2), br = self.rhoT[ny + 1].A[nx].shape, self.rhoB[ny].A[nx].shape, self._cell_maps(ny, nx)[3]
            need = max(need, 8 * (bl * Dt * Db + br * Dt2 * Db2 + bl * pd * Dt2 * Db + br * Dt2 * Db * pu + bl * pd * pu * br))
            bl = br
        return need

    def _line_pass(self, max_distance=None, slot_budget=None):
        """Every row of the rotated lattice contracted between rhoB[ny] and rhoT[ny+1] as they stand, with an operator of one cell
        inserted and another cell left open.  Per row: the right environments with their half-products as _open_cell_pass keeps
        them, then the left sweep with a stack of environments (slot 0 plain): at every cell the stack is stepped (tn_env3_stack,
        which opens one slot per operator of the cell), every carried slot is closed on the step's first products
        (tn_stack_cell_law), and the slots whose start cell falls max_distance cells back are dropped.  slot_budget (bytes) caps the
        stack: the start cells are cut into groups walked in successive left sweeps from the plain environments the first one
        keeps.  One read-back per row.  Returns (laws, joints, log2z): laws[c] (q,) the law of cell c = ny*Nx + nx from slot 0,
        joints {(c1, c2): (nop_c1, q_c2)} = <O_a(c1) [s_c2 = s]> for c1 left of c2 in a row, log2z (Ny, Nx) as _marginal_pass."""
        Nx, Ny = self.Nx, self.Ny
        reach = max(Nx - 1, 1) if max_distance is None else max(1, min(int(max_distance), Nx - 1))
        if slot_budget is None:
            slot_budget = torch.cuda.mem_get_info()[0] // 2
        dev = self.rhoT[0].A[0].device
        one = torch.ones((1, 1, 1, 1), dtype=torch.float64, device=dev)
        zero = torch.zeros(1, dtype=torch.float64, device=dev)
        laws, joints, log2z = [None] * (Nx * Ny), {}, np.zeros((Ny, Nx))
        for ny in range(Ny):
            fac = self._peps_factors_dev([(ny, nx) for nx in range(Nx)])
            At = [a.contiguous() for a in self.rhoT[ny + 1].A]
            Ab = [a.contiguous() for a in self.rhoB[ny].A]
            ER, lgR, HR = one[0], zero, [None] * Nx
            lgRs = [None] * (Nx + 1)
            lgRs[Nx] = zero
            for nx in range(Nx - 1, -1, -1):
                F, dm, rm, pd, br = fac[nx]
                ER, lgR, HR[nx] = ops.env3(1, ER, At[nx], ops.mpo_from_factor(F, dm, rm, pd, br), Ab[nx], lgR, keep_half=True)
                lgRs[nx] = lgR
            Os = [self._line_operators(ny, nx) for nx in range(Nx)]
            nops = [int(O.shape[0]) for O in Os]
            Od = [_dev_f64(O) if O.shape[0] else None for O in Os]
            groups = _plan_line_groups(nops[:Nx - 1], reach, int(slot_budget) // self._line_slot_bytes(ny))
            plain = [None] * (Nx + 1)
            plain[0] = (one, zero)
            recs = []
            for g, (k0, k1) in enumerate(groups):
                first = g == 0                                   # the first sweep runs to the end of the row and keeps the plain slots
                start, stop = (0, Nx - 1) if first else (k0, min(Nx - 1, k1 - 1 + reach))
                (E, lgL), starts = plain[start], []
                for nx in range(start, stop + 1):
                    F, dm, rm, pd, br = fac[nx]
                    insert = k0 <= nx < k1 and nops[nx] > 0
                    Wops = ops.mpo_from_factor_ops(F, dm, rm, pd, br, Od[nx] if insert else None)
                    out, lg, HL = ops.env3_stack(E, At[nx], Wops, Ab[nx], lgL, keep_half=True)
                    recs.append((nx, tuple(starts), first, ops.stack_cell_law(HL, HR[nx], F, dm, rm), lgL, lgRs[nx + 1]))
                    if first:
                        plain[nx + 1] = (out[:1].clone() if out.shape[0] > 1 else out, lg)
                    if insert:
                        starts.append(nx)
                    gone = sum(nops[k] for k in starts if k < nx + 1 - reach)
                    starts = [k for k in starts if k >= nx + 1 - reach]
                    E, lgL = (out if gone == 0 else torch.cat([out[:1], out[1 + gone:]])), lg
            host = _read_back([t for rec in recs for t in rec[3:]])
            for i, (nx, starts, first, _, _, _) in enumerate(recs):
                D, lgl, lgr = host[3 * i:3 * i + 3]
                T = D[0].sum()
                if first:
                    laws[ny * Nx + nx] = D[0] / T
                    log2z[ny, nx] = np.log2(T) + lgl[0] + lgr[0]
                e = 1
                for k in starts:
                    joints[(ny * Nx + k, ny * Nx + nx)] = D[e:e + nops[k]] / T
                    e += nops[k]
        return laws, joints, log2z

    # ------------------------------------------------------------------------------------ overlap distributions of the stored states (GPU)
    def calculate_overlap_distribution(self, kind=None, weights='uniform'):
        """Distribution of the overlap between two replicas, estimated from all pairs of distinct rows of `states`, whatever wrote
        them (sample_boltzmann, gibbs_sampling, search_ground_state, decode_low_energy_states): P(q) = sum_{a<b} w_a w_b
        [q_ab = q] / sum_{a<b} w_a w_b, the pair histogram on the device in exact integers (tn_pair_hist; tnac4o_amd/overlap.py).
        kind: 'spin' q = 1 - 2 d / N over the N active spins (d = Hamming distance); 'link' q_l = 1 - 2 d / N_b over the N_b
        couplings (every i < j with J0[i, j] != 0, one bit [s_i == s_j] each); 'cell' the fraction of cells in the same state,
        1 - d / (Nx Ny).  None = 'spin' for Ising, 'cell' for RMF; 'spin' and 'link' on RMF are a ValueError.
        weights: 'uniform'; 'importance' w_k = 2^(sample_log2Z_k - max), the self-normalised correction for a truncated contraction
        -- meaningful after sample_boltzmann only, a ValueError unless sample_log2Z exists with the length of `states`; or M
        non-negative finite numbers.  Anything else, and fewer than two states, is a ValueError raised before any device work.
        Stores overlap_values (nbins,), overlap_distribution (nbins,) (returned; bin d belongs to overlap_values[d]), overlap_moments
        {'q', 'abs_q', 'q2', 'q4', 'binder' = (3 - <q^4> / <q^2>^2) / 2, and for 'spin' 'chi_sg' = N <q^2>}, overlap_ess =
        (sum w)^2 / sum w^2, overlap_pairs = M (M - 1) / 2 and overlap_kind.  Under uniform weights the device part is the exact
        pair count; other weights are rounded to 32 bits of the largest.  More than 9183 bits (cells) per state do not fit the
        kernel's histogram: NotImplementedError naming the limit, there is no host fallback.  Changes nothing else."""
        from . import overlap
        return overlap.overlap_distribution(self, kind, weights)

    def calculate_overlap_errors(self, kind=None, weights='uniform'):
        """Error bars of the overlap moments of calculate_overlap_distribution -- <q>, <|q|>, <q^2>, <q^4>, the Binder ratio and, for
        'spin', chi_sg -- by the delete-one jackknife over the M rows of `states`.  kind and weights as
        calculate_overlap_distribution.  Equal rows are condensed; one call of tn_pair_rowsums gives, for every distinct row, the
        exact integer sums over all other rows of w_b d^k (k = 0 .. 4) and w_b |n - 2 d|; from them the host forms the estimate
        without each sample in turn (tnac4o_amd/overlap.py: jackknife).  With theta^(-s) the estimate without
        sample s, tbar their mean and M' the samples with a positive weight: error = sqrt((M' - 1) / M' sum_s (theta^(-s) - tbar)^2).
        Returns and stores overlap_errors, a dict over the keys of overlap_moments; stores overlap_error_estimates (the estimates
        themselves: those of calculate_overlap_distribution up to rounding), overlap_bias_corrected = M' theta - (M' - 1) tbar,
        overlap_state_q and overlap_state_q2 (M,) = the mean of q and of q^2 of state s with all OTHER samples (which states are
        typical, which are outliers; nan for a state whose weight was rounded away), overlap_error_kind and overlap_ess.  Writes
        none of the attributes of calculate_overlap_distribution.  Under uniform weights everything up to the final divisions
        is exact; other weights are rounded to 32 bits of the largest.
        INDEPENDENT samples only: the jackknife assumes that the rows of `states` are independent draws -- sample_boltzmann, or
        gibbs_sampling draws.  States moved by the Monte Carlo calls (relax_samples, relax_lines, exchange_clusters,
        temper_samples, anneal_population) are correlated, and the errors are then too small.
        Degenerate statistic: where <s_i> = 0 for every spin (high temperature without fields) the pair statistic is degenerate
        and the jackknife overestimates its variance, by about a factor of 2 (iid bits with p = 1/2, M = 128, n = 64: 1.9 to 2.4
        in a host experiment).
        Fewer than three states with a positive weight and bad arguments are a ValueError, more than 65535 bits (cells) per
        state a NotImplementedError naming the limit, all raised before any device work; there is no host fallback."""
        from . import overlap
        return overlap.overlap_errors(self, kind, weights)

    def calculate_overlap_correlations(self, axis='both', kind=None, weights='uniform'):
        """Overlap correlations between the lattice lines, from all pairs of distinct rows of `states` (whatever wrote them), and the
        second-moment correlation length of the overlap.  The line overlap q_g of a replica pair is the overlap restricted to model
        column g (axis 'x') or model row g (axis 'y'): for kind 'spin' (Ising default) the mean of s_a s_b over the active spins of
        the line, for 'cell' (RMF default) the fraction of its cells in the same state; 'link' is a ValueError (a coupling lies in
        two lines).  weights as calculate_overlap_distribution.  Per axis, one call of tn_pair_moments gives the exact integer sums
        of w_a w_b, w_a w_b d_g and w_a w_b d_g d_g' over the pairs (tnac4o_amd/overlap.py).
        Returns and stores overlap_line_correlations {'x': (Nx, Nx), 'y': (Ny, Ny)} = <q_g q_g'> (only the axes asked for; nan for a
        line without spins); stores overlap_line_mean = <q_g>, overlap_line_sizes = n_g, overlap_chi[axis][m] = chi_SG(k_m) =
        (1 / N) sum <Q_g Q_g'> cos(k_m (g - g')) with Q_g = n_g q_g, k_m = 2 pi m / G, m = 0 .. G // 2 (chi(0) of 'spin' is chi_sg
        of calculate_overlap_distribution), overlap_xi = 1 / (2 sin(pi / G)) sqrt(chi(0) / chi(k_1) - 1) (nan when G < 2 or the
        ratio is below 1), overlap_xi_over_L = xi / G, overlap_line_kind and overlap_ess.  More than 64 lines along an axis, or a
        line wider than 32 words (2048 spins, 128 cells), is a NotImplementedError naming the limit, raised before any device
        work; there is no host fallback.  Changes nothing else."""
        from . import overlap
        return overlap.overlap_correlations(self, axis, kind, weights)

    def calculate_sample_correlations(self, weights='uniform'):
        """<s_i s_j> between every pair of active spins, from the rows of `states` (whatever wrote them), with the magnetisations and
        the site-resolved replica-overlap correlations.  Ising only (ValueError for RMF).  weights as calculate_overlap_distribution.
        Equal rows are condensed; one call of tn_spin_moments gives, for every pair of spins, the exact integer weight of the samples
        in which they differ (tnac4o_amd/overlap.py).
        Returns and stores sample_correlations (n, n) = <sigma_i sigma_j> over the n active spins, sigma = +1 where binary_states
        writes 1 (the convention of `magnetization` and `correlations`), diagonal 1; stores sample_spins (n,), the active spins in
        model order (row and column i belong to spin sample_spins[i]), sample_magnetization (n,) = <sigma_i>,
        sample_overlap_correlations (n, n) = <q_i q_j>, the mean of (s_i s_j)_a (s_i s_j)_b over the pairs of DISTINCT samples
        a != b (the unbiased estimator of <s_i s_j>^2; its mean over i, j is <q^2> of calculate_overlap_distribution and its sums over
        lattice lines are those of calculate_overlap_correlations), sample_chi_sg (Nx, Ny) = chi_SG(k_x, k_y) = (1 / N) sum_ij
        <q_i q_j> cos(k . (r_i - r_j)) at k = 2 pi (m_x / Nx, m_y / Ny), r the model column and row of the spin's cell, and
        overlap_ess.  Under uniform weights everything is exact up to the final divisions; other weights are rounded to 32 bits of
        the largest.  Fewer than two states, or fewer than two with weight, and bad weights are a ValueError, more than 65534 active
        spins a NotImplementedError, all raised before any device work; there is no host fallback.  Changes nothing else."""
        from . import overlap
        return overlap.sample_correlations(self, weights)

    # ------------------------------------------------------------------------------------ output
    def binary_states(self, number=-1):
        """Bit strings: 1 spin up, 0 spin down, 2 inactive (tnac4o.py:261-288)."""
        ns = self.states.shape[0]
        ns = ns + number + 1 if number < 0 else min(number, ns)
        if self.mode != 'Ising':
            return self.states[:ns]
        out = np.zeros((ns, self.L), dtype=np.int8) + 2
        k = -1
        for ny in range(self.Ny_model):
            for nx in range(self.Nx_model):
                k += 1
                act = self.ind0[ny][nx]
                out[:, act] = (1 - _bits(len(act)))[self.states[:ns, k]]
        return out

    def states_from_binary(self, bits):
        """Cell states, in the encoding of `states`, of spin read-outs (Ising): the inverse of binary_states() on the active spins.
        bits: (M, L) integers, 1 spin up, 0 spin down; the entries of inactive spins are ignored.  Returns (M, Nx*Ny) int64 in
        model cell order (host numpy); a value other than 0 / 1 at an active spin is a ValueError."""
        if self.mode != 'Ising':
            raise ValueError('states_from_binary is for Ising models (an RMF state is its own read-out)')
        bits = np.asarray(bits)
        if bits.ndim != 2 or bits.shape[1] != self.L or bits.dtype.kind not in 'iub':
            raise ValueError('bits must be an integer array of shape (M, L) = (M, %d)' % self.L)
        out = np.zeros((bits.shape[0], self.Nx_model * self.Ny_model), dtype=np.int64)
        k = -1
        for ny in range(self.Ny_model):
            for nx in range(self.Nx_model):
                k += 1
                act = np.asarray(self.ind0[ny][nx], dtype=np.int64)
                b = bits[:, act].astype(np.int64)
                if np.any((b != 0) & (b != 1)):
                    raise ValueError('bits of active spins must be 0 or 1')
                out[:, k] = (1 - b) @ (2 ** np.arange(len(act), dtype=np.int64))
        return out

    def save(self, file_name):
        """Save the solution to a .npy file readable by `load` here and by the reference's `tnac4o.load`
        (tnac4o.py:200-231: a pickled dict with these keys)."""
        d = {'mode': self.mode, 'rotation': self.rotation, 'energy': self.energy, 'probability': self.probability,
             'degeneracy': self.degeneracy, 'states': self.states, 'discarded_probability': self.discarded_probability,
             'negative_probability': self.negative_probability, 'Nx': self.Nx_model, 'Ny': self.Ny_model, 'Nc': self.Nc,
             'beta': self.beta}
        if self.mode == 'Ising':
            d['ind'] = self.ind0
        if hasattr(self, 'excitations_encoding'):
            for k in ('excitations_encoding', 'd', 'invd', 'el', 'free_d'):
                d[k] = getattr(self, k)
            if self.excitations_encoding > 1 and self.mode == 'Ising':
                import scipy.sparse
                d['adj'] = scipy.sparse.csr_matrix(self.adj)
        np.save(file_name, d)

    def show_properties(self):
        """Print the lattice size and inverse temperature (what tnac4o.py:233-241 reports)."""
        for label, value in (('L', self.L), ('Ny', self.Ny), ('Nx', self.Nx), ('Beta', self.beta)):
            print('%-7s %s' % (label + ':', value))

    def show_solution(self, state=False):
        """Print a summary of the stored result; with state=True also the best configuration (tnac4o.py:244-259)."""
        if len(self.energy) == 0:
            print('No solution to show.')
            return
        rows = [('Energy', '%4.6f' % self.energy[0]), ('Degeneracy', '%2d' % self.degeneracy),
                ('log2(Probability)', '%0.2e' % self.probability[0]), ('Discarded log2(P)', '%0.2e' % self.discarded_probability),
                ('Min P (err)', '%0.2e' % self.negative_probability), ('# of states', '%1d' % len(self.energy)),
                ('Rotation/direction', '%1d' % self.rotation)]
        width = max(len(k) for k, _ in rows)
        for k, v in rows:
            print('%s : %s' % (k.ljust(width), v))
        if state:
            print(self.states[0])
