"""Host references for tnac4o.calculate_marginals (numpy only, no GPU).

- row_marginals_np: a numpy restatement of the three-layer row contraction of csrc/marginal.hip, evaluated on host copies of a
  solver's boundaries (rhoT, rhoB) and its host factor tables (_peps_factor, _mpo_site).  Results in the rotated frame.
- exact references by enumeration: a 3 x 3 Ising lattice of 2-spin cells with one inactive spin, a 3 x 3 RMF with 3 states per
  cell, and a 2 x 2 chimera lattice contracted exactly as a ring of four 256 x 256 transfer matrices.
"""
import itertools

import numpy as np

from tnac4o_amd import auxx


# ---------------------------------------------------------------------------------------------- restatement of the kernel
def _negative_rule(p):
    """The rule of tn_calc_pn / tn_cluster_marginal: lift entries below |min| to |min| when min < 0, normalise; (P, minP)."""
    p = np.array(p, dtype=np.float64)
    mn = float(p.min())
    if mn < 0:
        a = abs(mn)
        low = p < a
        p[low] = a
        mn *= int(low.sum())
    no = p.sum()
    if no > 0:
        return p / no, mn / no
    return p + 1.0 / p.size, -1.0


def _host(t):
    return t.detach().cpu().numpy()


def row_marginals_np(ins):
    """(P_rot list row-major, minP (Ny*Nx,), log2 row contractions (Ny, Nx)) from ins.rhoT / ins.rhoB as they stand."""
    Nx, Ny = ins.Nx, ins.Ny
    P_rot, minP, log2z = [], [], np.zeros((Ny, Nx))
    for ny in range(Ny):
        At = [_host(a) for a in ins.rhoT[ny + 1].A]
        Ab = [_host(a) for a in ins.rhoB[ny].A]
        W = [ins._mpo_site(ny, nx) for nx in range(Nx)]                  # (l, d, r, u)
        ER = [None] * (Nx + 1)
        lgR = np.zeros(Nx + 1)
        ER[Nx] = np.ones((1, 1, 1))                                      # (r, t', b')
        for nx in range(Nx - 1, -1, -1):
            E = np.einsum('tdx,ldru,buy,rxy->ltb', At[nx], W[nx], Ab[nx], ER[nx + 1], optimize=True)
            e = np.floor(np.log2(np.abs(E).max()))
            ER[nx], lgR[nx] = E / 2.0 ** e, lgR[nx + 1] + e
        EL, lgL = np.ones((1, 1, 1)), 0.0                                # (l, t, b)
        for nx in range(Nx):
            F, dmap, rmap, _, _ = ins._peps_factor(ny, nx)
            X = np.einsum('ltb,tdx,rxy,buy->ldru', EL, At[nx], ER[nx + 1], Ab[nx], optimize=True)
            raw = np.einsum('slu,slu->s', F, X[:, dmap, rmap, :].transpose(1, 0, 2))
            p, mn = _negative_rule(raw)
            P_rot.append(p)
            minP.append(mn)
            log2z[ny, nx] = np.log2(raw.sum()) + lgL + lgR[nx + 1]
            E = np.einsum('ltb,tdx,ldru,buy->rxy', EL, At[nx], W[nx], Ab[nx], optimize=True)
            e = np.floor(np.log2(np.abs(E).max()))
            EL, lgL = E / 2.0 ** e, lgL + e
    return P_rot, np.array(minP), log2z


# ---------------------------------------------------------------------------------------------- exact references
def ising_3x3_nc2(seed=11):
    """18 spins on 3 x 3 cells of 2 (spin i = cell*2 + m): fields, the intra-cell pair, right couplings between the m = 1 spins,
    down couplings between the m = 0 spins; spin 9 (cell 4, m = 1) has no term at all, so it is inactive."""
    rng = np.random.default_rng(seed)
    Nx = Ny = 3
    dead = 9

    def v():
        return float(rng.integers(-8, 9) or 3) / 8.0
    J = []
    for i in range(18):
        if i != dead:
            J.append([i, i, v()])
    for c in range(9):
        if c * 2 + 1 != dead and c * 2 != dead:
            J.append([c * 2, c * 2 + 1, v()])
    for ny in range(Ny):
        for nx in range(Nx - 1):
            a, b = (ny * Nx + nx) * 2 + 1, (ny * Nx + nx + 1) * 2 + 1
            if dead not in (a, b):
                J.append([a, b, v()])
    for ny in range(Ny - 1):
        for nx in range(Nx):
            a, b = (ny * Nx + nx) * 2, ((ny + 1) * Nx + nx) * 2
            J.append([a, b, v()])
    return J


def _active_sets(J, L, Nc, ncell):
    Jd = np.zeros((L, L))
    for i, j, x in J:
        a, b = (i, j) if i <= j else (j, i)
        Jd[a, b] += x
    out = []
    for c in range(ncell):
        ind = Nc * c + np.arange(Nc)
        w = np.abs(Jd[ind, :]).sum(1) + np.abs(Jd[:, ind]).sum(0)
        out.append(ind[w > 1e-12])
    return out


def _cell_states(binary, act):
    """Cell state of each configuration: bit i of the state is 1 where spin act[i] is down (binary 0)."""
    s = np.zeros(binary.shape[0], dtype=np.int64)
    for i, a in enumerate(act):
        s |= (1 - binary[:, a].astype(np.int64)) << i
    return s


def exact_ising(J, Nx, Ny, Nc, beta):
    """(marginals in model order, magnetisation (L,)) by enumeration of all 2^L configurations."""
    L = Nx * Ny * Nc
    binary = ((np.arange(2 ** L)[:, None] >> np.arange(L)[None, :]) & 1).astype(np.int8)
    E = auxx.energy_Jij(J, binary)
    w = np.exp(-beta * (E - E.min()))
    w /= w.sum()
    acts = _active_sets(J, L, Nc, Nx * Ny)
    marg = [np.bincount(_cell_states(binary, act), weights=w, minlength=2 ** len(act)) for act in acts]
    m = np.zeros(L)
    for act in acts:
        m[act] = w @ (2.0 * binary[:, act] - 1.0)
    return marg, m


def exact_rmf(J, beta):
    """Model-order marginals of an RMF by enumeration of all configurations."""
    N = np.asarray(J['N']).reshape(-1)
    states = np.array(list(itertools.product(*[range(int(n)) for n in N])), dtype=np.int64)
    E = auxx.energy_RMF(J, states)
    w = np.exp(-beta * (E - E.min()))
    w /= w.sum()
    return [np.bincount(states[:, k], weights=w, minlength=int(N[k])) for k in range(N.size)]


def exact_chimera_2x2(J, beta):
    """Model-order marginals and magnetisation of synthetic_chimera(2, 2, seed): the four cells form the ring
    (0,0) - (0,1) - (1,1) - (1,0) - (0,0), so P_a = diag(A B C D) / tr(A B C D) with one 256 x 256 matrix per ring bond."""
    L, Nc = 32, 8
    Jd = np.zeros((L, L))
    for i, j, x in J:
        a, b = (i, j) if i <= j else (j, i)
        Jd[a, b] += x
    sig = 1.0 - 2.0 * ((np.arange(256)[:, None] >> np.arange(8)[None, :]) & 1)       # (256, 8) spins of a cell state
    acts = _active_sets(J, L, Nc, 4)
    assert all(len(a) == 8 for a in acts)

    def cell_E(c):
        ind = c * 8 + np.arange(8)
        Jc = Jd[np.ix_(ind, ind)]
        return np.sum((sig @ np.triu(Jc, 1)) * sig, 1) + sig @ Jc.diagonal()

    def bond_E(c1, c2):
        i1, i2 = c1 * 8 + np.arange(8), c2 * 8 + np.arange(8)
        Jb = Jd[np.ix_(i1, i2)] + Jd[np.ix_(i2, i1)].T
        return sig @ Jb @ sig.T

    ring = [0, 1, 3, 2]
    mats = []
    for k in range(4):
        a, b = ring[k], ring[(k + 1) % 4]
        Eab = cell_E(a)[:, None] + bond_E(a, b)
        mats.append(np.exp(-beta * (Eab - Eab.min())))
    marg = [None] * 4
    for k in range(4):
        M = np.eye(256)
        for j in range(4):
            M = M @ mats[(k + j) % 4]
        d = np.diag(M).copy()
        marg[ring[k]] = d / d.sum()
    m = np.zeros(L)
    for c in range(4):
        m[c * 8 + np.arange(8)] = marg[c] @ sig
    return marg, m
