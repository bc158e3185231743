"""Host references for tnac4o.calculate_free_energy (numpy only, no GPU).

- terms_np: every row contraction r_ny = <rhoB[ny]| row ny |rhoT[ny+1]> and every overlap o_ny = <rhoB[ny]|rhoT[ny]> by einsum on
  host copies of a solver's boundaries and its host factor tables, as marginals_ref.row_marginals_np walks them; log2 of magnitudes.
- log2Z_np: the formula of calculate_free_energy on those terms, written out once more.
- exact entropies of the enumerable instances of tests/sampling_ref.py, over the ACTIVE spins, computed once per (case, beta).
"""
import functools
import itertools

import numpy as np

import marginals_ref as mr
import sampling_ref as sref
from tnac4o_amd import auxx

LN2 = float(np.log(2.0))


def _host(t):
    return t.detach().cpu().numpy()


def _pow2(E):
    e = np.floor(np.log2(np.abs(E).max()))
    return E / 2.0 ** e, e


def terms_np(ins):
    """(log2 |r_ny| (Ny,), log2 |o_ny| (Ny-1,)) from ins.rhoT / ins.rhoB as they stand."""
    Nx, Ny = ins.Nx, ins.Ny
    rows, cuts = np.zeros(Ny), np.zeros(Ny - 1)
    for ny in range(Ny):
        At = [_host(a) for a in ins.rhoT[ny + 1].A]
        Ab = [_host(a) for a in ins.rhoB[ny].A]
        E, lg = np.ones((1, 1, 1)), 0.0                                  # (l, t, b)
        for nx in range(Nx):
            E, e = _pow2(np.einsum('ltb,tdx,ldru,buy->rxy', E, At[nx], ins._mpo_site(ny, nx), Ab[nx], optimize=True))
            lg += e
        assert E.shape == (1, 1, 1)
        rows[ny] = np.log2(abs(E[0, 0, 0])) + lg
    for ny in range(1, Ny):
        At = [_host(a) for a in ins.rhoT[ny].A]
        Ab = [_host(a) for a in ins.rhoB[ny].A]
        E, lg = np.ones((1, 1)), 0.0                                     # (t, b)
        for nx in range(Nx):
            E, e = _pow2(np.einsum('tb,tsx,bsy->xy', E, At[nx], Ab[nx], optimize=True))
            lg += e
        assert E.shape == (1, 1)
        cuts[ny - 1] = np.log2(abs(E[0, 0])) + lg
    return rows, cuts


def energy_shift(ins):
    """sum over the cells of min Es + min E1 + min E4: what the PEPS factors take out of the exponents."""
    return float(sum(np.min(t) for ny in range(ins.Ny) for nx in range(ins.Nx) for t in ins._cell_energies(ny, nx)))


def log2Z_np(ins):
    rows, cuts = terms_np(ins)
    for psi in (ins.rhoB[0], ins.rhoT[ins.Ny]):                          # the trivial ends contract to magnitude 1
        assert abs(abs(float(np.prod([_host(a).reshape(-1)[0] for a in psi.A]))) - 1.0) <= 1e-15
        assert all(tuple(a.shape) == (1, 1, 1) for a in psi.A)
    return float(rows.sum() - cuts.sum() - ins.beta / LN2 * energy_shift(ins)), rows, cuts


@functools.lru_cache(maxsize=None)
def exact_log2Z(case, beta):
    return sref.exact_log2Z(case, beta)


@functools.lru_cache(maxsize=None)
def exact_entropy(case, beta):
    """-sum p ln p (nats) over the configurations of the ACTIVE spins, by enumeration: 'ising3x3' (2^18 configurations, one inactive spin:
    ln 2 taken out) or 'rmf3x3' (3^9)."""
    if case == 'ising3x3':
        binary = ((np.arange(2 ** 18)[:, None] >> np.arange(18)[None, :]) & 1).astype(np.int8)
        E, extra = auxx.energy_Jij(mr.ising_3x3_nc2(), binary), LN2
    elif case == 'rmf3x3':
        states = np.array(list(itertools.product(range(3), repeat=9)), dtype=np.int64)
        E, extra = auxx.energy_RMF(auxx.synthetic_rmf(3, 3, 3, 17), states), 0.0
    else:
        raise ValueError(case)
    w = np.exp(-beta * (E - E.min()))
    p = w / w.sum()
    return float(-np.sum(p * np.log(p))) - extra
