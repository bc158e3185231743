"""Host references for tnac4o.calculate_correlations (numpy only, no GPU).

- row_bond_tables_np: a numpy restatement of the bond-marginal pass (csrc/marginal.hip, tn_cluster_bond_marginal) on host copies
  of a solver's boundaries and factor tables, in the rotated frame: row_marginals_np without summing out l and u.
- enum_bond_tables: the same tables of the rotated frame by enumeration of every configuration (small lattices only).
- exact model-frame references: nearest-neighbour correlations / pair marginals and the mean energy by enumeration (3 x 3 Ising
  cells of 2 spins, 3 x 3 RMF) and by the ring of four 256 x 256 transfer matrices (2 x 2 chimera).
"""
import itertools

import numpy as np

import marginals_ref as mr
from tnac4o_amd import auxx


# ---------------------------------------------------------------------------------------------- restatement of the kernel
def row_bond_tables_np(ins):
    """(Pl list, Pu list, minB (Ny*Nx,), log2 row contractions (Ny, Nx)) from ins.rhoT / ins.rhoB as they stand."""
    Nx, Ny = ins.Nx, ins.Ny
    Pl, Pu, minB, log2z = [], [], [], np.zeros((Ny, Nx))
    for ny in range(Ny):
        At = [mr._host(a) for a in ins.rhoT[ny + 1].A]
        Ab = [mr._host(a) for a in ins.rhoB[ny].A]
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
            prod = F * X[:, dmap, rmap, :].transpose(1, 0, 2)            # (s, l, u)
            T = prod.sum()
            pl, pu = prod.sum(2) / T, prod.sum(1) / T
            Pl.append(pl)
            Pu.append(pu)
            minB.append(min(0.0, float(pl.min()), float(pu.min())))
            log2z[ny, nx] = np.log2(T) + lgL + lgR[nx + 1]
            E = np.einsum('ltb,tdx,ldru,buy->rxy', EL, At[nx], W[nx], Ab[nx], optimize=True)
            e = np.floor(np.log2(np.abs(E).max()))
            EL, lgL = E / 2.0 ** e, lgL + e
    return Pl, Pu, np.array(minB), log2z


# ---------------------------------------------------------------------------------------------- rotated-frame enumeration
def enum_bond_tables(ins):
    """(Pl, Pu) of every cell of the solver's (rotated) lattice by enumeration, with the bond indices the solver uses."""
    Nx, Ny = ins.Nx, ins.Ny
    beta = ins.beta
    if ins.mode == 'Ising':
        rows, cols = np.nonzero(ins.J)
        J = [[int(i), int(j), float(ins.J[i, j])] for i, j in zip(rows, cols)]
        binary = ((np.arange(2 ** ins.L)[:, None] >> np.arange(ins.L)[None, :]) & 1).astype(np.int8)
        E = auxx.energy_Jij(J, binary)
        st = np.stack([mr._cell_states(binary, ins.ind[ny][nx]) for ny in range(Ny) for nx in range(Nx)], 1)
    else:
        Jr = {'fun': ins.J['fun'], 'fac': ins.J['fac'], 'N': ins.N, 'Nx': Nx, 'Ny': Ny}
        st = np.array(list(itertools.product(*[range(int(n)) for n in np.asarray(ins.N).reshape(-1)])), dtype=np.int64)
        E = auxx.energy_RMF(Jr, st)
    w = np.exp(-beta * (E - E.min()))
    w /= w.sum()
    Pl, Pu = [], []
    for ny in range(Ny):
        for nx in range(Nx):
            c = ny * Nx + nx
            q = int(ins.N[ny][nx])
            if ins.mode == 'Ising':
                bl = int(ins.lr[ny, nx - 1]) if nx > 0 else 1
                pu = int(ins.ld[ny - 1, nx]) if ny > 0 else 1
                l = ins._ind_bond_right(st[:, c - 1], ny, nx - 1) if nx > 0 else np.zeros_like(st[:, c])
                u = ins._ind_bond_down(st[:, c - Nx], ny - 1, nx) if ny > 0 else np.zeros_like(st[:, c])
            else:
                bl, pu = int(ins.ll[ny, nx]), int(ins.lu[ny, nx])
                l = st[:, c - 1] % bl if nx > 0 else np.zeros_like(st[:, c])
                u = st[:, c - Nx] % pu if ny > 0 else np.zeros_like(st[:, c])
            Pl.append(np.bincount(st[:, c] * bl + l, weights=w, minlength=q * bl).reshape(q, bl))
            Pu.append(np.bincount(st[:, c] * pu + u, weights=w, minlength=q * pu).reshape(q, pu))
    return Pl, Pu


# ---------------------------------------------------------------------------------------------- exact model-frame references
def _dense(J, L):
    Jd = np.zeros((L, L))
    for i, j, x in J:
        a, b = (i, j) if i <= j else (j, i)
        Jd[a, b] += x
    return Jd


def _pairs(Jd):
    return np.argwhere(np.triu(Jd, 1) != 0).astype(np.int64)


def exact_ising(J, L, beta):
    """(bond_pairs, <s_i s_j>, <E>, m) by enumeration of all 2^L configurations."""
    Jd = _dense(J, L)
    binary = ((np.arange(2 ** L)[:, None] >> np.arange(L)[None, :]) & 1).astype(np.int8)
    E = auxx.energy_Jij(J, binary)
    w = np.exp(-beta * (E - E.min()))
    w /= w.sum()
    sig = 2.0 * binary - 1.0
    pairs = _pairs(Jd)
    C = np.array([w @ (sig[:, i] * sig[:, j]) for i, j in pairs])
    return pairs, C, float(w @ E), w @ sig


def exact_rmf(J, beta):
    """({two-cell key: P[s1, s2]}, <E>) by enumeration of all configurations."""
    N = np.asarray(J['N']).reshape(-1)
    st = np.array(list(itertools.product(*[range(int(n)) for n in N])), dtype=np.int64)
    E = auxx.energy_RMF(J, st)
    w = np.exp(-beta * (E - E.min()))
    w /= w.sum()
    out = {}
    for key in J['fac']:
        if len(key) == 4:
            c1, c2 = key[0] * J['Nx'] + key[1], key[2] * J['Nx'] + key[3]
            n1, n2 = int(N[c1]), int(N[c2])
            out[key] = np.bincount(st[:, c1] * n2 + st[:, c2], weights=w, minlength=n1 * n2).reshape(n1, n2)
    return out, float(w @ E)


def exact_chimera_2x2(J, beta):
    """(bond_pairs, <s_i s_j>, <E>) of synthetic_chimera(2, 2, seed) from the ring (0,0) - (0,1) - (1,1) - (1,0) of 256 x 256
    transfer matrices: the joint of ring neighbours a -> b is mats[a->b] * (rest of the ring)^T / tr."""
    L = 32
    Jd = _dense(J, L)
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
    joint, marg = {}, [None] * 4
    for k in range(4):
        a, b = ring[k], ring[(k + 1) % 4]
        R = mats[(k + 1) % 4] @ mats[(k + 2) % 4] @ mats[(k + 3) % 4]
        P = mats[k] * R.T
        P /= P.sum()
        joint[(a, b)] = P
        marg[a] = P.sum(1)
    Em = sum(marg[c] @ cell_E(c) for c in range(4)) + sum(float(np.sum(P * bond_E(a, b))) for (a, b), P in joint.items())
    pairs = _pairs(Jd)
    C = []
    for i, j in pairs:
        a, b = i // 8, j // 8
        if a == b:
            C.append(marg[a] @ (sig[:, i % 8] * sig[:, j % 8]))
        elif (a, b) in joint:
            C.append(sig[:, i % 8] @ joint[(a, b)] @ sig[:, j % 8])
        else:
            C.append(sig[:, j % 8] @ joint[(b, a)] @ sig[:, i % 8])
    return pairs, np.array(C), float(Em)
