"""Host references for tnac4o.calculate_correlation_function (numpy only, no GPU).

- ops_site_np: the operator-weighted row-MPO planes of tn_mpo_from_factor_ops.
- line_pass_np: a numpy restatement of tnac4o._line_pass on host copies of a solver's boundaries and factor tables, in the rotated
  frame: the environments of row_marginals_np with an operator of one cell inserted, carried one start cell at a time (no stack).
- enum_line_tables: the tables model_line_correlations consumes, for every pair of cells of one line of the solver's (rotated)
  lattice, by enumeration of every configuration (small lattices only).
- exact model-frame references: all line pairs by enumeration (Ising, RMF) and from the ring of four 256 x 256 transfer matrices
  (2 x 2 chimera, where every pair of cells of one line is a pair of ring neighbours).
"""
import itertools

import numpy as np

import correlations_ref as cr
import marginals_ref as mr
from tnac4o_amd import auxx


# ---------------------------------------------------------------------------------------------- restatement of the kernels
def ops_site_np(F, dmap, rmap, pd, br, O):
    """Wops (1 + nop, l, d, r, u): plane 0 = sum_s T[s], plane 1 + a = sum_s O[a, s] T[s]."""
    q, nl, nu = F.shape
    Oall = np.vstack([np.ones((1, q)), np.asarray(O, dtype=np.float64).reshape(-1, q)])
    W = np.zeros((pd, br, Oall.shape[0], nl, nu))
    np.add.at(W, (dmap, rmap), (Oall[:, :, None, None] * F[None]).transpose(1, 0, 2, 3))
    return np.ascontiguousarray(W.transpose(2, 3, 0, 1, 4))


def _step(E, At, W, Ab):
    """The left step of the environments E (n, l, t, b) through one site -> (n, r, t', b').  (tensordot: the stacked index keeps
    einsum off BLAS, and the 8 x 8 lattice takes minutes then.)"""
    H = np.tensordot(E, At, ([2], [0]))                          # n l b d x
    Y = np.tensordot(H, W, ([1, 3], [0, 1]))                     # n b x r u
    return np.tensordot(Y, Ab, ([1, 4], [0, 1])).transpose(0, 2, 1, 3)


def _insert(EL, At, Wk, Ab):
    """The plain environment EL (l, t, b) stepped through the operator planes Wk (a, l, d, r, u) -> (a, r, t', b')."""
    H = np.tensordot(EL, At, ([1], [0]))                         # l b d x
    Y = np.tensordot(H, Wk, ([0, 2], [1, 2]))                    # b x a r u
    return np.tensordot(Y, Ab, ([0, 4], [0, 1])).transpose(1, 2, 0, 3)


def _close(E, At, ER, Ab, F, dmap, rmap):
    """D (n, q) raw: the environments E (n, l, t, b) closed at a cell."""
    H = np.tensordot(E, At, ([2], [0]))                          # n l b d x
    HR = np.tensordot(ER, Ab, ([2], [2]))                        # r x b u
    X = np.tensordot(H, HR, ([2, 4], [2, 1]))                    # n l d r u
    return np.einsum('slu,nlsu->ns', F, X[:, :, dmap, rmap, :])


def line_pass_np(ins, max_distance=None):
    """(laws, joints, log2z) as tnac4o._line_pass returns them, from ins.rhoT / ins.rhoB as they stand."""
    Nx, Ny = ins.Nx, ins.Ny
    reach = max(Nx - 1, 1) if max_distance is None else max(1, min(int(max_distance), Nx - 1))
    laws, joints, log2z = [None] * (Nx * Ny), {}, np.zeros((Ny, Nx))
    for ny in range(Ny):
        At = [mr._host(a) for a in ins.rhoT[ny + 1].A]
        Ab = [mr._host(a) for a in ins.rhoB[ny].A]
        cells = [ins._peps_factor(ny, nx) for nx in range(Nx)]
        W = [ins._mpo_site(ny, nx) for nx in range(Nx)]
        ER, lgR = [None] * (Nx + 1), np.zeros(Nx + 1)
        ER[Nx] = np.ones((1, 1, 1))
        for nx in range(Nx - 1, -1, -1):
            E = np.einsum('tdx,ldru,buy,rxy->ltb', At[nx], W[nx], Ab[nx], ER[nx + 1], optimize=True)
            e = np.floor(np.log2(np.abs(E).max()))
            ER[nx], lgR[nx] = E / 2.0 ** e, lgR[nx + 1] + e
        EL, lgL, scale = [np.ones((1, 1, 1))], [0.0], []          # plain environments, their running log2, the factor of every step
        for nx in range(Nx):
            E = np.einsum('ltb,tdx,ldru,buy->rxy', EL[nx], At[nx], W[nx], Ab[nx], optimize=True)
            e = np.floor(np.log2(np.abs(E).max()))
            EL.append(E / 2.0 ** e)
            lgL.append(lgL[nx] + e)
            scale.append(2.0 ** e)
        T = np.zeros(Nx)
        for nx in range(Nx):
            F, dmap, rmap, _, _ = cells[nx]
            D0 = _close(EL[nx][None], At[nx], ER[nx + 1], Ab[nx], F, dmap, rmap)[0]
            T[nx] = D0.sum()
            laws[ny * Nx + nx] = D0 / T[nx]
            log2z[ny, nx] = np.log2(T[nx]) + lgL[nx] + lgR[nx + 1]
        for k in range(Nx - 1):
            F, dmap, rmap, pd, br = cells[k]
            Wk = ops_site_np(F, dmap, rmap, pd, br, ins._line_operators(ny, k))[1:]
            E = _insert(EL[k], At[k], Wk, Ab[k]) / scale[k]
            for m in range(k + 1, min(Nx - 1, k + reach) + 1):
                F, dmap, rmap, _, _ = cells[m]
                joints[(ny * Nx + k, ny * Nx + m)] = _close(E, At[m], ER[m + 1], Ab[m], F, dmap, rmap) / T[m]
                E = _step(E, At[m], W[m], Ab[m]) / scale[m]
    return laws, joints, log2z


# ---------------------------------------------------------------------------------------------- rotated-frame enumeration
def _enumerate(ins):
    """(weights, cell states (n, Nx*Ny), spins (n, L) or None) of every configuration of the solver's (rotated) lattice."""
    if ins.mode == 'Ising':
        rows, cols = np.nonzero(ins.J)
        J = [[int(i), int(j), float(ins.J[i, j])] for i, j in zip(rows, cols)]
        binary = ((np.arange(2 ** ins.L)[:, None] >> np.arange(ins.L)[None, :]) & 1).astype(np.int8)
        E = auxx.energy_Jij(J, binary)
        st, sig = None, 2.0 * binary - 1.0
    else:
        Jr = {'fun': ins.J['fun'], 'fac': ins.J['fac'], 'N': ins.N, 'Nx': ins.Nx, 'Ny': ins.Ny}
        st = np.array(list(itertools.product(*[range(int(n)) for n in np.asarray(ins.N).reshape(-1)])), dtype=np.int64)
        E, sig = auxx.energy_RMF(Jr, st), None
    w = np.exp(-ins.beta * (E - E.min()))
    return w / w.sum(), st, sig


def enum_line_tables(ins, lines='rows', max_distance=None):
    """{(c1, c2): M} of the solver's (rotated) lattice, c1 < c2 two cells of one row ('rows') or one column ('columns') at most
    max_distance cells apart: Ising M[a, b] = <sigma_i sigma_j> over the active spins of the two cells, RMF M = P[s1, s2]."""
    Nx, Ny = ins.Nx, ins.Ny
    w, st, sig = _enumerate(ins)
    out = {}
    for c1 in range(Nx * Ny):
        for c2 in range(c1 + 1, Nx * Ny):
            (y1, x1), (y2, x2) = divmod(c1, Nx), divmod(c2, Nx)
            if not ((lines == 'rows' and y1 == y2) or (lines == 'columns' and x1 == x2)):
                continue
            if max_distance is not None and abs(y1 - y2) + abs(x1 - x2) > max_distance:
                continue
            if ins.mode == 'Ising':
                i, j = np.asarray(ins.ind[y1][x1], dtype=np.int64), np.asarray(ins.ind[y2][x2], dtype=np.int64)
                out[(c1, c2)] = (sig[:, i] * w[:, None]).T @ sig[:, j]
            else:
                n1, n2 = int(ins.N[y1][x1]), int(ins.N[y2][x2])
                out[(c1, c2)] = np.bincount(st[:, c1] * n2 + st[:, c2], weights=w, minlength=n1 * n2).reshape(n1, n2)
    return out


# ---------------------------------------------------------------------------------------------- exact model-frame references
def _line_cells(Nx, Ny, max_distance=None):
    """[(k1, k2, distance)] of the model cells k1 < k2 (row-major) of one row or one column."""
    out = []
    for k1 in range(Nx * Ny):
        for k2 in range(k1 + 1, Nx * Ny):
            (y1, x1), (y2, x2) = divmod(k1, Nx), divmod(k2, Nx)
            d = abs(y1 - y2) + abs(x1 - x2)
            if (y1 == y2 or x1 == x2) and (max_distance is None or d <= max_distance):
                out.append((k1, k2, d))
    return out


def _active(Jd, Nc, k):
    ind = Nc * k + np.arange(Nc)
    return ind[np.abs(Jd[ind, :]).sum(1) + np.abs(Jd[:, ind]).sum(0) > 1e-12]


def exact_line_ising(J, Nx, Ny, Nc, beta, max_distance=None):
    """(line_pairs, line_distance, C, m) of an Ising model by enumeration of all 2^L configurations."""
    L = Nx * Ny * Nc
    Jd = cr._dense(J, L)
    binary = ((np.arange(2 ** L)[:, None] >> np.arange(L)[None, :]) & 1).astype(np.int8)
    E = auxx.energy_Jij(J, binary)
    w = np.exp(-beta * (E - E.min()))
    w /= w.sum()
    sig = 2.0 * binary - 1.0
    rows = []
    for k1, k2, d in _line_cells(Nx, Ny, max_distance):
        for i in _active(Jd, Nc, k1):
            for j in _active(Jd, Nc, k2):
                rows.append((int(i), int(j), d, float(w @ (sig[:, i] * sig[:, j]))))
    rows.sort(key=lambda t: t[:2])
    m = np.zeros(L)
    for k in range(Nx * Ny):
        act = _active(Jd, Nc, k)
        m[act] = w @ sig[:, act]
    return (np.array([t[:2] for t in rows], dtype=np.int64), np.array([t[2] for t in rows], dtype=np.int64),
            np.array([t[3] for t in rows]), m)


def exact_line_rmf(J, beta, max_distance=None):
    """{(y1, x1, y2, x2): P[s1, s2]} for every pair of cells of one line, first cell first in row-major order; and the marginals."""
    N = np.asarray(J['N']).reshape(-1)
    Nx, Ny = J['Nx'], J['Ny']
    st = np.array(list(itertools.product(*[range(int(n)) for n in N])), dtype=np.int64)
    E = auxx.energy_RMF(J, st)
    w = np.exp(-beta * (E - E.min()))
    w /= w.sum()
    out = {}
    for k1, k2, _ in _line_cells(Nx, Ny, max_distance):
        n1, n2 = int(N[k1]), int(N[k2])
        out[divmod(k1, Nx) + divmod(k2, Nx)] = np.bincount(st[:, k1] * n2 + st[:, k2], weights=w, minlength=n1 * n2).reshape(n1, n2)
    return out


def exact_line_chimera_2x2(J, beta):
    """(line_pairs, line_distance, C, m) of synthetic_chimera(2, 2, seed): the pairs of cells of one line, (0,1), (2,3), (0,2), (1,3),
    are the neighbours of the ring (0,0) - (0,1) - (1,1) - (1,0) of 256 x 256 transfer matrices of correlations_ref."""
    Jd = cr._dense(J, 32)
    sig = 1.0 - 2.0 * ((np.arange(256)[:, None] >> np.arange(8)[None, :]) & 1)

    def cell_E(c):
        ind = c * 8 + np.arange(8)
        Jc = Jd[np.ix_(ind, ind)]
        return np.sum((sig @ np.triu(Jc, 1)) * sig, 1) + sig @ Jc.diagonal()

    def bond_E(c1, c2):
        i1, i2 = c1 * 8 + np.arange(8), c2 * 8 + np.arange(8)
        return sig @ (Jd[np.ix_(i1, i2)] + Jd[np.ix_(i2, i1)].T) @ sig.T

    ring = [0, 1, 3, 2]
    mats = []
    for k in range(4):
        a, b = ring[k], ring[(k + 1) % 4]
        Eab = cell_E(a)[:, None] + bond_E(a, b)
        mats.append(np.exp(-beta * (Eab - Eab.min())))
    rows, m = [], np.zeros(32)
    for k in range(4):
        a, b = ring[k], ring[(k + 1) % 4]
        P = mats[k] * (mats[(k + 1) % 4] @ mats[(k + 2) % 4] @ mats[(k + 3) % 4]).T
        P /= P.sum()
        m[a * 8 + np.arange(8)] = P.sum(1) @ sig
        C = sig.T @ P @ sig                      # [spin of a, spin of b]
        for x in range(8):
            for y in range(8):
                i, j = a * 8 + x, b * 8 + y
                rows.append((min(i, j), max(i, j), 1, float(C[x, y])))
    rows.sort(key=lambda t: t[:2])
    return (np.array([t[:2] for t in rows], dtype=np.int64), np.array([t[2] for t in rows], dtype=np.int64),
            np.array([t[3] for t in rows]), m)
