"""Driver of tnac4o.temper_samples: parallel tempering with isoenergetic cluster moves (PT+ICM: Zhu, Ochoa, Katzgraber) over the stored
configurations with the library's tn_temper (csrc/temper.hip).

The M = R T stored states are R chains of T temperatures: row m belongs to chain m // T and starts at temperature index m % T.  A round
is (1) heat-bath sweeps of relax_samples' move with every row at the beta it currently holds, (2) exchange_clusters' move between
the rows of two chains that sit at the SAME temperature, for every temperature at or above cluster_beta_min, (3) swaps of the
temperature labels of the rows at neighbouring temperatures inside a chain, accepted with min(1, exp((beta' - beta)(E' - E))),
alternating between the even and the odd pairs of temperatures.  Each of the three leaves the joint law prod_c prod_t pi_beta_t
invariant, so the composition does.  States, assignment and counters stay on the device for all rounds of a call.

The host part (the bit tables, every argument check, the layout of the uniform numbers) is plain numpy and runs without a GPU."""
import ctypes as C

import numpy as np

from .exchange import check_pairs, coupling_csr
from .overlap import MAX_SPIN_BITS, active_spins
from .sampler import check_states

UNIFORM_KEYS = ('sweep', 'cluster', 'swap')


def check_betas(betas):
    """The ladder: a sequence of T >= 1 positive finite numbers, strictly increasing.  Returns it as float64 (T,); ValueError otherwise."""
    try:
        b = np.array(betas, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('betas must be a sequence of numbers')
    if b.ndim != 1 or b.size < 1:
        raise ValueError('betas must be a non-empty one-dimensional sequence')
    if not np.all(np.isfinite(b)) or not np.all(b > 0.0):
        raise ValueError('betas must be positive and finite')
    if np.any(np.diff(b) <= 0.0):
        raise ValueError('betas must be strictly increasing')
    return b


def bit_tables(solver):
    """The tables that turn cell states into packed spin bits and back on the device (Ising): (nbits, cellbits (Nx*Ny, nbmax) int32,
    bitcell (nbits, 2) int32).  Row position p = active spin p in model order (the bits of overlap.spin_bits); cells are numbered in
    the walk order of the CURRENT rotation, as the device holds them: model cell k sits at solver.order[k], and bit j of its state is
    spin ind0[k][j] (binary_states).  cellbits[cell, j] = the position of bit j of that cell's state, -1 beyond its spins;
    bitcell[p] = (cell, j)."""
    if solver.mode != 'Ising':
        raise ValueError("bit_tables is defined for mode 'Ising' only")
    act = active_spins(solver)
    n = int(act.size)
    spins = [np.asarray(solver.ind0[ny][nx], dtype=np.int64) for ny in range(solver.Ny_model) for nx in range(solver.Nx_model)]
    nbmax = max([1] + [len(s) for s in spins])
    cellbits = np.full((len(spins), nbmax), -1, dtype=np.int32)
    bitcell = np.full((n, 2), -1, dtype=np.int32)
    order = np.asarray(solver.order)
    for k, s in enumerate(spins):
        pos = np.searchsorted(act, s)
        cellbits[order[k], :len(s)] = pos
        bitcell[pos, 0] = order[k]
        bitcell[pos, 1] = np.arange(len(s))
    return n, cellbits, bitcell


def _check_one(u, name, shape):
    """sampler.check_uniforms' rules on one array of a given shape."""
    is_np = isinstance(u, np.ndarray)
    if not is_np:
        import torch
        if not isinstance(u, torch.Tensor):
            raise ValueError("uniforms[%r] must be a numpy array or a torch tensor (got %s)" % (name, type(u).__name__))
    if tuple(u.shape) != tuple(shape):
        raise ValueError('uniforms[%r] must have shape %s, got %s' % (name, tuple(shape), tuple(u.shape)))
    if is_np:
        if u.dtype != np.float64:
            raise ValueError('uniforms[%r] must be float64, got %s' % (name, u.dtype))
        ok = bool(np.all((u >= 0.0) & (u < 1.0)))
    else:
        import torch
        if u.dtype != torch.float64:
            raise ValueError('uniforms[%r] must be float64, got %s' % (name, u.dtype))
        ok = bool(((u >= 0.0) & (u < 1.0)).all().item())
    if not ok:                                            # (a NaN fails both comparisons)
        raise ValueError('uniforms[%r] must lie in [0, 1) (no NaN)' % name)
    return u


def uniform_shapes(rounds, sweeps, ncell, M, T, Tc, Pc):
    """The shapes of the three arrays of uniform numbers: sweep (rounds, sweeps, Ny*Nx, M) -- round, sweep, cell in walk order of the
    current rotation, row --, cluster (rounds, Tc, Pc), swap (rounds, R, T - 1)."""
    return {'sweep': (rounds, sweeps, ncell, M), 'cluster': (rounds, Tc, Pc), 'swap': (rounds, M // T, T - 1)}


def check_temper_uniforms(uniforms, shapes):
    """None, or a dict with exactly the keys 'sweep', 'cluster', 'swap', each under sampler.check_uniforms' rules in its shape of
    uniform_shapes.  Returns it as it is; ValueError otherwise."""
    if uniforms is None:
        return None
    if not isinstance(uniforms, dict) or set(uniforms) != set(UNIFORM_KEYS):
        raise ValueError("uniforms must be None or a dict with the keys 'sweep', 'cluster' and 'swap'")
    return {k: _check_one(uniforms[k], k, shapes[k]) for k in UNIFORM_KEYS}


def draw_block(shapes, lo, hi):
    """The uniform numbers of the rounds lo .. hi - 1 from numpy's global generator, in the order sweep, cluster, swap."""
    return {k: np.random.rand(*((hi - lo,) + tuple(shapes[k][1:]))) for k in UNIFORM_KEYS}


def check_arguments(solver, betas, rounds, sweeps, cluster_moves, cluster_beta_min, pairs, uniforms, keep, rounds_per_call, seed=None):
    """Everything temper_samples can refuse before any device work.  Returns a dict: betas, T, R, M, states (M, Nx*Ny) int64 in model
    order, rounds, sweeps, cluster (bool), cluster_from, pairs (rounds, Pc, 2) int32, shapes, uniforms (None or the dict), keep,
    rounds_per_call, seed (None or an int: rng.check_seed, not together with uniforms).  The pairings are drawn here (before any
    uniform) when pairs is None: from numpy's global generator, or with a seed from its pairing keys."""
    from . import rng
    b = check_betas(betas)
    T = int(b.size)
    seed = rng.check_seed_alone(seed, uniforms)
    for name, v in (('rounds', rounds), ('sweeps', sweeps)):
        if isinstance(v, bool) or int(v) != v or v < 0:
            raise ValueError('%s must be a non-negative integer' % name)
    rounds, sweeps = int(rounds), int(sweeps)
    if rounds_per_call is not None and (isinstance(rounds_per_call, bool) or int(rounds_per_call) != rounds_per_call or rounds_per_call < 1):
        raise ValueError('rounds_per_call must be None or a positive integer')
    if getattr(solver, 'states', None) is None or np.asarray(solver.states).ndim != 2 or np.asarray(solver.states).shape[0] < 1:
        raise ValueError('temper_samples works on the stored states (run sample_boltzmann, gibbs_sampling, a search or relax_samples first)')
    st = check_states(np.asarray(solver.states), solver._cell_sizes()[solver.order])
    M = int(st.shape[0])
    if M % T:
        raise ValueError('the %d stored states are no multiple of the %d temperatures (betas)' % (M, T))
    R = M // T
    if keep is not None and (isinstance(keep, bool) or int(keep) != keep or not 0 <= keep < T):
        raise ValueError('keep must be None or a temperature index in [0, %d)' % T)
    cluster = bool(cluster_moves)
    cluster_from = 0
    if cluster:
        if solver.mode != 'Ising':
            raise ValueError("cluster_moves=True is defined for mode 'Ising' only (RMF: cluster_moves=False)")
        if R < 2:
            raise ValueError('cluster_moves=True needs at least two chains (M >= 2 len(betas))')
        n = int(active_spins(solver).size)
        if n < 1:
            raise ValueError('the model has no active spin')
        if n > MAX_SPIN_BITS:
            raise NotImplementedError('the model has %d active spins; the cluster move takes at most %d; there is no host fallback' % (n, MAX_SPIN_BITS))
        if cluster_beta_min is not None:
            cmin = float(cluster_beta_min)
            if not np.isfinite(cmin):
                raise ValueError('cluster_beta_min must be None or a finite number')
            cluster_from = int(np.searchsorted(b, cmin, side='left'))
        pairs = rng.draw_pairs(seed, rng.TEMPER_PAIRING, rounds, R) if (seed is not None and pairs is None) else check_pairs(pairs, rounds, R)
    else:
        if pairs is not None:
            raise ValueError('pairs must be None with cluster_moves=False')
        if cluster_beta_min is not None:
            raise ValueError('cluster_beta_min must be None with cluster_moves=False')
        pairs = np.zeros((rounds, 0, 2), dtype=np.int32)
        cluster_from = T
    shapes = uniform_shapes(rounds, sweeps, solver.Nx * solver.Ny, M, T, T - cluster_from, int(pairs.shape[1]))
    return dict(betas=b, T=T, R=R, M=M, states=st, rounds=rounds, sweeps=sweeps, cluster=cluster, cluster_from=cluster_from, pairs=pairs,
                shapes=shapes, uniforms=check_temper_uniforms(uniforms, shapes), keep=None if keep is None else int(keep),
                rounds_per_call=None if rounds_per_call is None else int(rounds_per_call), seed=seed)


def seeded_block(seed, shapes, lo, hi, dev):
    """The uniform numbers of the rounds lo .. hi - 1 filled on the device (one tn_uniforms per array): every number a function of the
    seed and its logical position with the GLOBAL round, so the blocks of any cut join to the same arrays."""
    from . import rng
    kinds = {'sweep': rng.TEMPER_SWEEP, 'cluster': rng.TEMPER_CLUSTER, 'swap': rng.TEMPER_SWAP}
    out = {}
    for k in UNIFORM_KEYS:
        tail = tuple(shapes[k][1:])
        out[k] = rng.fill(seed, kinds[k], lo * int(np.prod(tail[:-1], dtype=np.int64)), (hi - lo,) + tail, dev=dev)
    return out


def round_bytes(shapes, M, record):
    """Device bytes one round of a call takes: its uniform numbers (the sweep's are the large item) and, with record, its traces."""
    n = sum(int(np.prod(shapes[k][1:])) for k in UNIFORM_KEYS) * 8
    if record:
        n += M * 12 + int(np.prod(shapes['cluster'][1:])) * 8
    return n


def plan_rounds(rounds, per_round, budget):
    """Rounds per call: as many as fit `budget` bytes, at least one, at most `rounds`."""
    return int(max(1, min(max(rounds, 1), budget // max(per_round, 1))))


def reorder_trace(energy_trace, tidx_trace, T):
    """(rounds, M) energies and temperature indices by row -> (rounds, T, R) energies by temperature and chain."""
    rounds, M = energy_trace.shape
    out = np.empty((rounds, T, M // T))
    chain = np.arange(M) // T
    for r in range(rounds):
        out[r, tidx_trace[r], chain] = energy_trace[r]
    return out


def temper_native(solver, states_rot, a, record, tables=None, meas=None):
    """The device loop: states, tables and graph go up once, the rounds run in blocks of rounds_per_call calls of tn_temper with round0
    advanced, everything comes back once.  states_rot: (M, Ny*Nx) in the lattice order of the current rotation; a: what
    check_arguments returned; tables: (nbits, cellbits, bitcell, rowptr, cols) numpy, or None without cluster moves.  meas: None, or
    what ladder.check_arguments returned with nbits, bitcell and links (numpy, or None) added: the blocks are cut so that one ends behind
    every measurement round, and tn_ladder_measure follows it on the stream with that block's energies, adding to the accumulators of
    the measurement's time bin.  Returns a dict of numpy arrays: states, energy, tidx, accepted, attempted, with record energy_trace,
    tidx_trace, sizes, differing, and with meas spin_hist (B, T, nbits + 1), link_hist (B, T, nlinks + 1) or None, esums (B, T, 3)."""
    import torch
    from . import ops
    from .relax import EnergyCells
    dev = torch.device('cuda', torch.cuda.current_device())
    Nx, Ny = solver.Nx, solver.Ny
    M, T, R, rounds, sweeps = a['M'], a['T'], a['R'], a['rounds'], a['sweeps']
    table = EnergyCells(solver, dev)
    d_st = torch.as_tensor(np.ascontiguousarray(states_rot, dtype=np.int16)).to(dev)
    d_tidx = torch.as_tensor((np.arange(M) % T).astype(np.int32)).to(dev)
    d_slot = torch.as_tensor(np.arange(M, dtype=np.int32).reshape(R, T)).to(dev)
    d_acc = torch.zeros(max(T - 1, 0), dtype=torch.int32, device=dev)
    d_att = torch.zeros(max(T - 1, 0), dtype=torch.int32, device=dev)
    bits = None
    if tables is not None:
        bits = (tables[0],) + tuple(torch.as_tensor(np.ascontiguousarray(t, dtype=np.int32)).to(dev) for t in tables[1:])
    d_pairs = torch.as_tensor(a['pairs']).to(dev) if tables is not None else None
    per = a['rounds_per_call']
    if per is None:
        fixed = M * Nx * Ny * 2 + int(ops.lib().tn_temper_ws_bytes(Nx, Ny, M, T, 0 if tables is None else tables[0], a['pairs'].shape[1]))
        per = plan_rounds(rounds, round_bytes(a['shapes'], M, record), max(torch.cuda.mem_get_info(dev)[0] // 2 - fixed, 0))
    given = a['uniforms']
    due = {}
    if meas is not None:
        B = meas['B']
        due = {int(r) + 1: int(b) for r, b in zip(meas['after'], meas['bins'])}               # block end -> time bin
        m_bitcell = torch.as_tensor(np.ascontiguousarray(meas['bitcell'], dtype=np.int32)).to(dev)
        m_links = None if meas['links'] is None else torch.as_tensor(np.ascontiguousarray(meas['links'], dtype=np.int32)).to(dev)
        d_sh = torch.zeros((B, T, meas['nbits'] + 1), dtype=torch.int64, device=dev)
        d_lh = None if m_links is None else torch.zeros((B, T, m_links.shape[0] + 1), dtype=torch.int64, device=dev)
        d_es = torch.zeros((B, T, 3), dtype=torch.float64, device=dev)

    def block(u, lo, hi):
        u = u[lo:hi]
        return (torch.as_tensor(np.ascontiguousarray(u)) if isinstance(u, np.ndarray) else u).to(dev).contiguous()

    outs = []
    energy = None
    from .ladder import block_ends
    lo = 0
    for hi in block_ends(rounds, per, None if meas is None else meas['after']):
        if a.get('seed') is not None:
            d_u = seeded_block(a['seed'], a['shapes'], lo, hi, dev)
        else:
            u = given if given is not None else draw_block(a['shapes'], 0, hi - lo)
            off = lo if given is not None else 0
            d_u = {k: block(u[k], off, off + hi - lo) for k in UNIFORM_KEYS}
        out = ops.temper(table.cells, Nx, Ny, a['betas'], d_st, d_tidx, d_slot, lo, hi - lo, sweeps, usweep=d_u['sweep'], bits=bits,
                         cluster_from=a['cluster_from'], cpairs=None if d_pairs is None else d_pairs[lo:hi].contiguous(), ucl=d_u['cluster'],
                         uswap=d_u['swap'], accepted=d_acc if T > 1 else None, attempted=d_att if T > 1 else None, record=record)
        energy = out['energy']
        if record:
            outs.append(out)
        del d_u                                            # (released in stream order: the next block's numbers may take their place)
        if hi in due:
            b = due[hi]
            ops.ladder_measure(table.cells, Nx, Ny, d_st, d_slot, meas['nbits'], m_bitcell, d_sh[b], m_links, None if d_lh is None else d_lh[b],
                               meas['split'], energy, d_es[b])
        lo = hi
    res = dict(states=d_st.cpu().numpy().astype(np.int64), energy=energy.cpu().numpy(), tidx=d_tidx.cpu().numpy().astype(np.int64),
               accepted=d_acc.cpu().numpy().astype(np.int64), attempted=d_att.cpu().numpy().astype(np.int64))
    if record:
        for k in ('energy_trace', 'tidx_trace', 'sizes', 'differing'):
            res[k] = None if outs[0][k] is None else np.concatenate([o[k].cpu().numpy() for o in outs], axis=0)
    if meas is not None:
        res.update(spin_hist=d_sh.cpu().numpy(), link_hist=None if d_lh is None else d_lh.cpu().numpy(), esums=d_es.cpu().numpy())
    del table
    return res


def temper_samples(solver, betas, rounds=10, sweeps=1, cluster_moves=True, cluster_beta_min=None, pairs=None, uniforms=None, record=False,
                   keep=None, rounds_per_call=None, seed=None, measure=None, measure_from=0, measure_bins=16, measure_pairs='all',
                   measure_links=True):
    """temper_samples of tnac4o (documented there)."""
    a = check_arguments(solver, betas, rounds, sweeps, cluster_moves, cluster_beta_min, pairs, uniforms, keep, rounds_per_call, seed)
    meas = None
    if measure is not None:
        from . import ladder
        meas = ladder.check_arguments(solver, a, measure, measure_from, measure_bins, measure_pairs, measure_links)
    tables = None
    if a['cluster']:
        tables = bit_tables(solver) + coupling_csr(solver)
    if meas is not None:
        nbits, _, bitcell = tables[:3] if tables is not None else bit_tables(solver)
        meas.update(nbits=nbits, bitcell=bitcell, links=ladder.link_table(solver) if meas['links'] else None)
    st = a['states']
    rot = np.empty_like(st)
    rot[:, solver.order] = st                                # the inverse of _store_result's states[:, order]
    res = temper_native(solver, rot, a, bool(record), tables, meas)
    T, R = a['T'], a['R']
    states, energy, tidx = res['states'][:, solver.order], res['energy'], res['tidx']
    solver.temper_betas = a['betas']
    solver.temper_index, solver.temper_beta = tidx, a['betas'][tidx]
    solver.temper_swap_accepted, solver.temper_swap_attempted = res['accepted'], res['attempted']
    if meas is not None:
        ladder.store(solver, res['spin_hist'], res['link_hist'], res['esums'], meas['n_meas'], R, a['betas'])
    if record:
        solver.temper_energy_trace = reorder_trace(res['energy_trace'], res['tidx_trace'], T)
        Tc, Pc = a['shapes']['cluster'][1:]
        empty = np.zeros((a['rounds'], Tc, Pc), dtype=np.int64)
        solver.temper_cluster_sizes = empty if res['sizes'] is None else res['sizes'].astype(np.int64)
        solver.temper_cluster_differing = empty.copy() if res['differing'] is None else res['differing'].astype(np.int64)
    if a['keep'] is not None:
        rows = np.flatnonzero(tidx == a['keep'])             # one row per chain, chains ascending
        states, energy = states[rows], energy[rows]
    solver.states, solver.energy = states, energy
    solver.probability = solver.sample_log2Z = solver.log2Z_lower = solver.log2Z_estimate = None
    return energy
