"""Host reference of tn_anneal / tnac4o.anneal_population (numpy and Python integers, no GPU): a whole call composed of
relax_ref.total_energy, relax_ref.sweep and the resampling rule of include/tnpeps.h (K13).

- weights: Emin and the fp64 weights of a step.
- offsets: systematic resampling from EXACT prefix sums of those weights (Python integers over a common power-of-two denominator), with
  the smallest distance of any C_m / W * M + u (m < M - 1) from an integer: how far the offsets are from a value that another order of
  the additions, or another last bit of exp, could move.
- run: one call; besides the outputs it returns that margin and the draw margin of the sweeps (relax_ref).
- delta: the bound of DESIGN section 21 below which the device's offsets may differ from the reference's.
- CASES / TILE_CASES: the seeded inputs shared by the host and the GPU tests.
"""
import functools
from fractions import Fraction
from itertools import accumulate

import numpy as np

import relax_ref as rr

TILE = 256                                   # rows of a tile of the device's running sums (csrc/anneal.hip)


def delta(M):
    """4 M (M + 8) 2^-52: device and reference offsets agree whenever every C_m / W * M + u is at least this far from an integer."""
    return 4.0 * M * (M + 8) * 2.0 ** -52


def weights(E, db):
    """(Emin, w): Emin = the smallest energy that is no NaN (NaN when all are), w = exp(-(db (E - Emin))) with NaN read as 0."""
    E = np.asarray(E, dtype=np.float64)
    emin = np.fmin.reduce(E)
    with np.errstate(invalid='ignore', over='ignore'):
        w = np.exp(-(db * (E - emin)))
    return emin, np.where(np.isnan(w), 0.0, w)


def _integers(w):
    """The doubles w as integers over one common denominator 2^k: (list of int, k)."""
    ratios = [float(x).as_integer_ratio() for x in w]
    k = max(d.bit_length() - 1 for _, d in ratios)
    return [n << (k - (d.bit_length() - 1)) for n, d in ratios], k


def offsets(w, u):
    """Systematic resampling of M rows with the weights w and the uniform number u.  Returns dict(O (M,), parent (M,), counts (M,),
    wsum, w2sum = the exactly summed W and sum w^2 rounded once, margin).  W zero or not finite: the identity, margin inf."""
    w = np.asarray(w, dtype=np.float64)
    M = w.size
    ident = dict(O=np.arange(1, M + 1), parent=np.arange(M), counts=np.ones(M, dtype=np.int64), margin=np.inf)
    if not np.all(np.isfinite(w)):
        return dict(ident, wsum=float(np.sum(w)), w2sum=float(np.sum(w * w)))
    wi, k = _integers(w)
    C = list(accumulate(wi))
    W = C[-1]
    wsum = float(Fraction(W, 1 << k))
    w2sum = float(Fraction(sum(x * x for x in wi), 1 << (2 * k)))
    if W == 0:
        return dict(ident, wsum=0.0, w2sum=0.0)
    un, ud = float(u).as_integer_ratio()
    den = W * ud
    O = np.empty(M, dtype=np.int64)
    prev, margin = 0, np.inf
    for m in range(M - 1):
        num = C[m] * M * ud + un * W                      # C_m / W * M + u = num / den
        f, r = divmod(num, den)
        margin = min(margin, float(Fraction(min(r, den - r), den)))
        prev = min(M, max(prev, f))
        O[m] = prev
    O[M - 1] = M
    parent = np.searchsorted(O, np.arange(M), side='right')
    return dict(O=O, parent=parent, counts=np.diff(np.concatenate([[0], O])), wsum=wsum, w2sum=w2sum, margin=margin)


def run(cells, Nx, Ny, states, family, betas, sweeps, usweep=None, ures=None):
    """tn_anneal.  states (M, ncell); family (M,); betas (K,); usweep (K - 1, sweeps, ncell, M); ures (K - 1,).  Returns a dict: states,
    family, energy, emin, wsum, w2sum (K - 1,), survivors (K - 1,), energy_trace, parent_trace (K - 1, M), margin = the smallest draw
    margin of the sweeps, resample_margin = the smallest distance of a C_m / W * M + u from an integer."""
    betas = np.asarray(betas, dtype=np.float64)
    st = np.array(states, dtype=np.int64)
    fam = np.array(family, dtype=np.int64)
    M, K = st.shape[0], betas.size
    emin, wsum, w2sum = np.zeros(K - 1), np.zeros(K - 1), np.zeros(K - 1)
    survivors = np.zeros(K - 1, dtype=np.int64)
    etrace, ptrace = np.zeros((K - 1, M)), np.zeros((K - 1, M), dtype=np.int64)
    margin, rmargin = np.inf, np.inf
    E = rr.total_energy(cells, Nx, Ny, st)
    for s in range(1, K):
        db = betas[s] - betas[s - 1]
        emin[s - 1], w = weights(E, db)
        r = offsets(w, ures[s - 1])
        wsum[s - 1], w2sum[s - 1] = r['wsum'], r['w2sum']
        survivors[s - 1] = np.count_nonzero(r['counts'] >= 1)
        rmargin = min(rmargin, r['margin'])
        st, fam = st[r['parent']], fam[r['parent']]
        ptrace[s - 1] = r['parent']
        for j in range(sweeps):
            st, _, mg = rr.sweep(cells, Nx, Ny, st, 0, betas[s], usweep[s - 1, j])
            if mg.size:
                margin = min(margin, float(mg.min()))
        E = rr.total_energy(cells, Nx, Ny, st)
        etrace[s - 1] = E
    return dict(states=st, family=fam, energy=E, emin=emin, wsum=wsum, w2sum=w2sum, survivors=survivors, energy_trace=etrace,
                parent_trace=ptrace, margin=margin, resample_margin=rmargin)


# ---------------------------------------------------------------------------------------------- seeded inputs
BETAS = (0.0, 0.3, 0.7, 1.2)
SWEEPS = 2
# relax_ref's inputs on the lattices '2x2' and '3x3' (with and without maps, M = 1, 65, 300) and its integer tables with tied energies;
# a seed whose margins fall below the bounds (tests/test_anneal_host.py) is replaced, never excused
CASES = [c for c in rr.CASES if c[0] in ('2x2', '3x3')]
CASE_IDS = ['%s-%s-M%d%s' % (c[0], 'maps' if c[1] else 'plain', c[2], '-int' if c[4] else '') for c in CASES]
SEED_SHIFT = {}                              # case -> what is added to its seed of the uniform numbers (a replaced seed)


@functools.lru_cache(maxsize=None)
def case_inputs(case, K=len(BETAS)):
    """dict(cells, Nx, Ny, states (M, ncell), family, betas (K,), usweep (K - 1, SWEEPS, ncell, M), ures (K - 1,)) of a case; computed once,
    never modified.  K > 4 continues the schedule in steps of 0.4."""
    Ny, Nx, cells, states, _ = rr.case_inputs(case)
    M, ncell = states.shape
    rng = np.random.default_rng(case[3] + 2 + SEED_SHIFT.get(case, 0))
    betas = np.array(list(BETAS) + [BETAS[-1] + 0.4 * (i + 1) for i in range(K - len(BETAS))])[:K]
    usweep, ures = rng.random((K - 1, SWEEPS, ncell, M)), rng.random(K - 1)
    for a in (usweep, ures, betas):
        a.setflags(write=False)
    return dict(cells=cells, Nx=Nx, Ny=Ny, states=states, family=np.arange(M), betas=betas, usweep=usweep, ures=ures)


def run_case(c, lo=0, hi=None, state=None):
    """run() on the steps lo .. hi - 1 of a case's inputs (step s goes from betas[s] to betas[s + 1]), from `state` = a previous result."""
    hi = c['betas'].size - 1 if hi is None else hi
    s = state or c
    return run(c['cells'], c['Nx'], c['Ny'], s['states'], s['family'], c['betas'][lo:hi + 1], SWEEPS, c['usweep'][lo:hi], c['ures'][lo:hi])


@functools.lru_cache(maxsize=None)
def case_reference(case):
    return run_case(case_inputs(case))


# resampling alone on the one-cell lattice (q = 100): M around the tile of the running sums and above its square, so that the sums of
# the tiles span more than one group of the wave that adds them up; (M, seed)
TILE_CASES = [(TILE - 1, 11), (TILE, 12), (TILE + 1, 13), (TILE * TILE + 3, 16)]
TILE_BETAS = (0.5, 0.9, 1.6)


@functools.lru_cache(maxsize=None)
def tile_inputs(M, seed):
    Ny, Nx, qs = rr.LATTICES['1x1']
    cells = rr.make_cells(Ny, Nx, qs, False, seed)
    rng = np.random.default_rng(seed + 1)
    states = rng.integers(0, qs[0], size=(M, 1))
    ures = rng.random(len(TILE_BETAS) - 1)
    return dict(cells=cells, Nx=Nx, Ny=Ny, states=states, family=np.arange(M), betas=np.array(TILE_BETAS), ures=ures)


@functools.lru_cache(maxsize=None)
def tile_reference(M, seed):
    c = tile_inputs(M, seed)
    return run(c['cells'], c['Nx'], c['Ny'], c['states'], c['family'], c['betas'], 0, None, c['ures'])


# ---------------------------------------------------------------------------------------------- the law problem
LAW_BETAS = np.linspace(0.0, 0.7, 8)
LAW_SWEEPS = 2
Z_M, Z_SEEDS = 2 ** 12, tuple(range(500, 516))
LAW_M, LAW_SEED = 2 ** 14, 77


def exact_log2Z(cells, Nx, Ny, beta):
    """log2 sum_x exp(-beta E(x)) over all configurations, by enumeration."""
    E = rr.total_energy(cells, Nx, Ny, rr.all_configurations(cells))
    e0 = E.min()
    return float(np.log2(np.sum(np.exp(-beta * (E - e0)))) - beta * e0 / np.log(2.0))


def law_inputs(M, seed):
    """A fresh population on relax_ref.law_problem(): uniformly random states and the uniform numbers of LAW_BETAS with LAW_SWEEPS sweeps."""
    cells, _ = rr.law_problem()
    rng = np.random.default_rng(seed)
    K = LAW_BETAS.size
    return dict(cells=cells, Nx=2, Ny=2, states=rng.integers(0, 4, size=(M, 4)), family=np.arange(M), betas=LAW_BETAS,
                usweep=rng.random((K - 1, LAW_SWEEPS, 4, M)), ures=rng.random(K - 1))


@functools.lru_cache(maxsize=None)
def law_reference(M, seed):
    c = law_inputs(M, seed)
    return run(c['cells'], 2, 2, c['states'], c['family'], c['betas'], LAW_SWEEPS, c['usweep'], c['ures'])


# rows of 4, 16 and 32 bytes (the lattices above have rows of 2, 8 and 18): every width of the pieces a row is copied in; (Ny, Nx, q, M, seed)
WIDTH_CASES = [(1, 2, 5, 70, 21), (2, 4, 3, 70, 22), (4, 4, 2, 70, 23)]
WIDTH_BETAS = (0.1, 0.6, 1.3)


@functools.lru_cache(maxsize=None)
def width_inputs(case):
    Ny, Nx, q, M, seed = case
    cells = rr.make_cells(Ny, Nx, [q] * (Ny * Nx), False, seed)
    rng = np.random.default_rng(seed + 1)
    K = len(WIDTH_BETAS)
    return dict(cells=cells, Nx=Nx, Ny=Ny, states=rng.integers(0, q, size=(M, Ny * Nx)), family=np.arange(M), betas=np.array(WIDTH_BETAS),
                usweep=rng.random((K - 1, 1, Ny * Nx, M)), ures=rng.random(K - 1))


@functools.lru_cache(maxsize=None)
def width_reference(case):
    c = width_inputs(case)
    return run(c['cells'], c['Nx'], c['Ny'], c['states'], c['family'], c['betas'], 1, c['usweep'], c['ures'])
