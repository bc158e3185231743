"""Driver of tnac4o.anneal_population: population annealing (Hukushima, Iba; Machta; Wang, Machta, Katzgraber) with the library's
tn_anneal (csrc/anneal.hip).

A population of M configurations that samples the Boltzmann law at betas[0] is taken along the schedule betas[1], betas[2], ...  A step
from beta' to beta (1) gives row m the weight w_m = exp(-(beta - beta') (E_m - Emin)), (2) resamples the population to M rows with
n_m copies of row m, E[n_m] = M w_m / W, by systematic resampling with ONE uniform number, (3) makes `sweeps` heat-bath sweeps of
relax_samples' move at beta.  (2) turns samples of pi_beta' weighted by w into unweighted samples of pi_beta, (3) leaves pi_beta
invariant and takes the copies apart.  The mean weight W / M estimates Z(beta) / Z(beta') exp((beta - beta') Emin) without bias, so the
running product is an estimate of the partition function at every beta of the schedule.  The population never leaves the device.

The host part (every argument check, the layout of the uniform numbers, the estimators) is plain numpy and runs without a GPU."""
import numpy as np

from .sampler import check_states
from .temper import _check_one, plan_rounds

STEP_KEYS = ('resample', 'sweep')


def check_schedule(betas):
    """The schedule: a sequence of K >= 1 finite numbers, betas[0] >= 0, strictly increasing.  Returns it as float64 (K,); ValueError
    otherwise."""
    try:
        b = np.array(betas, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('betas must be a sequence of numbers')
    if b.ndim != 1 or b.size < 1:
        raise ValueError('betas must be a non-empty one-dimensional sequence')
    if not np.all(np.isfinite(b)):
        raise ValueError('betas must be finite')
    if b[0] < 0.0:
        raise ValueError('betas[0] must not be negative')
    if np.any(np.diff(b) <= 0.0):
        raise ValueError('betas must be strictly increasing')
    return b


def uniform_shapes(K, sweeps, ncell, M):
    """The shapes of the arrays of uniform numbers: resample (K - 1,) -- one number per step --, sweep (K - 1, sweeps, Ny*Nx, M) -- step,
    sweep, cell in walk order of the current rotation, row --, init (M, Ny*Nx), the draw of a fresh population."""
    return {'resample': (K - 1,), 'sweep': (K - 1, sweeps, ncell, M), 'init': (M, ncell)}


def check_anneal_uniforms(uniforms, shapes, fresh):
    """None, or a dict with exactly the keys 'resample' and 'sweep' -- and 'init' when the population is drawn (fresh) --, each under
    sampler.check_uniforms' rules in its shape of uniform_shapes.  Returns it as it is; ValueError otherwise."""
    if uniforms is None:
        return None
    keys = STEP_KEYS + (('init',) if fresh else ())
    if not isinstance(uniforms, dict) or set(uniforms) != set(keys):
        raise ValueError('uniforms must be None or a dict with the keys %s' % ', '.join(repr(k) for k in keys))
    return {k: _check_one(uniforms[k], k, shapes[k]) for k in keys}


def draw_block(shapes, lo, hi):
    """The uniform numbers of the steps lo .. hi - 1 (step s goes from betas[s] to betas[s + 1]) from numpy's global generator, in the
    order resample, sweep."""
    return {k: np.random.rand(*((hi - lo,) + tuple(shapes[k][1:]))) for k in STEP_KEYS}


def draw_population(u, qs):
    """A population drawn uniformly: state = min(floor(u q_k), q_k - 1), u (M, ncell) in [0, 1), qs (ncell,) the states of every cell."""
    qs = np.asarray(qs, dtype=np.int64)
    return np.minimum(np.floor(np.asarray(u, dtype=np.float64) * qs[None, :]).astype(np.int64), qs[None, :] - 1)


def check_arguments(solver, betas, sweeps, M, uniforms, log2Z0, steps_per_call, seed=None):
    """Everything anneal_population can refuse before any device work.  Returns a dict: betas, K, M, fresh (the population is drawn),
    states ((M, Nx*Ny) int64 in model order, None when fresh), sweeps, shapes, uniforms (None or the dict), log2Z0, steps_per_call,
    seed (None or an int: rng.check_seed, not together with uniforms)."""
    from .rng import check_seed_alone
    b = check_schedule(betas)
    K = int(b.size)
    seed = check_seed_alone(seed, uniforms)
    if isinstance(sweeps, bool) or int(sweeps) != sweeps or sweeps < 0:
        raise ValueError('sweeps must be a non-negative integer')
    if steps_per_call is not None and (isinstance(steps_per_call, bool) or int(steps_per_call) != steps_per_call or steps_per_call < 1):
        raise ValueError('steps_per_call must be None or a positive integer')
    qs = solver._cell_sizes()
    fresh = M is not None
    st = None
    if fresh:
        if isinstance(M, bool) or int(M) != M or M < 1:
            raise ValueError('M must be None or a positive integer')
        M = int(M)
        if b[0] != 0.0:
            raise ValueError('M is given: the population is drawn uniformly, which is the law at betas[0] = 0 only (got betas[0] = %g)' % b[0])
    else:
        if getattr(solver, 'states', None) is None or np.asarray(solver.states).ndim != 2 or np.asarray(solver.states).shape[0] < 1:
            raise ValueError('anneal_population with M=None works on the stored states (run sample_boltzmann, relax_samples or temper_samples first, '
                             'or give M and betas[0] = 0)')
        st = check_states(np.asarray(solver.states), qs[solver.order])
        M = int(st.shape[0])
    if log2Z0 is None:
        log2Z0 = float(np.sum(np.log2(qs.astype(np.float64)))) if b[0] == 0.0 else 0.0
    else:
        try:
            log2Z0 = float(log2Z0)
        except (TypeError, ValueError):
            raise ValueError('log2Z0 must be None or a finite number')
        if not np.isfinite(log2Z0):
            raise ValueError('log2Z0 must be None or a finite number')
    shapes = uniform_shapes(K, int(sweeps), solver.Nx * solver.Ny, M)
    return dict(betas=b, K=K, M=M, fresh=fresh, states=st, sweeps=int(sweeps), shapes=shapes, uniforms=check_anneal_uniforms(uniforms, shapes, fresh),
                log2Z0=log2Z0, steps_per_call=None if steps_per_call is None else int(steps_per_call), seed=seed)


def seeded_block(seed, shapes, lo, hi, dev):
    """The uniform numbers of the steps lo .. hi - 1 filled on the device (one tn_uniforms per array): every number a function of the
    seed and its logical position with the GLOBAL step, so the blocks of any cut join to the same arrays."""
    from . import rng
    tail = tuple(shapes['sweep'][1:])
    return {'resample': rng.fill(seed, rng.ANNEAL_RESAMPLE, 0, (hi - lo,), first=lo, dev=dev),
            'sweep': rng.fill(seed, rng.ANNEAL_SWEEP, lo * tail[0] * tail[1], (hi - lo,) + tail, dev=dev)}


def seeded_population(seed, M, qs, dev):
    """draw_population on the device from the seed's init numbers (rng.ANNEAL_INIT: row = member, index = cell): (M, ncell) int16."""
    import torch
    from . import rng
    q = torch.as_tensor(np.asarray(qs, dtype=np.float64)).to(dev)
    u = rng.fill(seed, rng.ANNEAL_INIT, 0, (M, int(q.numel())), dev=dev)
    return torch.minimum(torch.floor(u * q[None, :]), q[None, :] - 1.0).to(torch.int16)


def step_bytes(shapes, M, record):
    """Device bytes one step of a call takes: its uniform numbers (the sweep's are the large item), its row of the energy trace and, with
    record, of the parent trace."""
    return (1 + int(np.prod(shapes['sweep'][1:]))) * 8 + M * 8 + (M * 4 if record else 0)


# ---------------------------------------------------------------------------------------------- estimators (host)
def log2Z_path(betas, emin, wsum, M, log2Z0):
    """(K,) log2 Z along the schedule: log2Z0, then the running sum of log2(W_s / M) - (betas[s] - betas[s-1]) Emin_s / ln 2."""
    betas = np.asarray(betas, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        inc = np.log2(np.asarray(wsum, dtype=np.float64) / M) - np.diff(betas) * np.asarray(emin, dtype=np.float64) / np.log(2.0)
    return np.concatenate([[float(log2Z0)], float(log2Z0) + np.cumsum(inc)])


def free_energy_path(betas, log2Z):
    """-ln Z / beta where beta > 0, NaN where beta = 0."""
    betas = np.asarray(betas, dtype=np.float64)
    out = np.full(betas.shape, np.nan)
    pos = betas > 0.0
    out[pos] = -np.asarray(log2Z)[pos] * np.log(2.0) / betas[pos]
    return out


def family_statistics(family):
    """(rho_t, entropy) of the family labels of a population of M rows: with n_f rows of family f and p_f = n_f / M,
    rho_t = M sum_f p_f^2 (1 for M distinct families, M for one) and entropy = -sum_f p_f ln p_f."""
    family = np.asarray(family)
    M = family.size
    p = np.unique(family, return_counts=True)[1].astype(np.float64) / M
    return float(M * np.sum(p * p)), float(-np.sum(p * np.log(p)))


# ---------------------------------------------------------------------------------------------- the device loop
def anneal_native(solver, states_rot, a, record):
    """The device loop: states and families go up once, the schedule runs in blocks of steps_per_call steps of tn_anneal, each on
    betas[lo .. hi] with states and family carried over on the device, everything comes back once.  states_rot: (M, Ny*Nx) in the
    lattice order of the current rotation, or None with a['seed'] and a['fresh']: the population is then made on the device;
    a: what check_arguments returned.  Returns a dict of numpy arrays: states, energy, family,
    energy0 (M,) = the energies on entry, emin, wsum, w2sum, survivors (K - 1,), energy_trace (K - 1, M) and with record parent_trace."""
    import torch
    from . import ops
    from .relax import EnergyCells
    dev = torch.device('cuda', torch.cuda.current_device())
    Nx, Ny = solver.Nx, solver.Ny
    M, K, sweeps, betas = a['M'], a['K'], a['sweeps'], a['betas']
    steps = K - 1
    table = EnergyCells(solver, dev)
    seed = a.get('seed')
    if states_rot is None:
        d_st = seeded_population(seed, M, solver._cell_sizes(), dev)
    else:
        d_st = torch.as_tensor(np.ascontiguousarray(states_rot, dtype=np.int16)).to(dev)
    d_fam = torch.arange(M, dtype=torch.int32, device=dev)
    per = a['steps_per_call']
    if per is None:
        fixed = M * Nx * Ny * 2 + M * 12 + int(ops.lib().tn_anneal_ws_bytes(Nx, Ny, M))
        per = plan_rounds(steps, step_bytes(a['shapes'], M, record), max(torch.cuda.mem_get_info(dev)[0] // 2 - fixed, 0))
    given = a['uniforms']

    def block(u, lo, hi):
        u = u[lo:hi]
        return (torch.as_tensor(np.ascontiguousarray(u)) if isinstance(u, np.ndarray) else u).to(dev).contiguous()

    first = ops.anneal(table.cells, Nx, Ny, betas[:1], d_st, d_fam, 0)
    energy0 = energy = first['energy']
    outs = []
    for lo in range(0, steps, per):
        hi = min(lo + per, steps)
        if seed is not None:
            d_u = seeded_block(seed, a['shapes'], lo, hi, dev)
        else:
            u = given if given is not None else draw_block(a['shapes'], 0, hi - lo)
            off = lo if given is not None else 0
            d_u = {k: block(u[k], off, off + hi - lo) for k in STEP_KEYS}
        out = ops.anneal(table.cells, Nx, Ny, betas[lo:hi + 1], d_st, d_fam, sweeps, usweep=d_u['sweep'] if sweeps else None, ures=d_u['resample'],
                         record=record)
        energy = out['energy']
        outs.append(out)
        del d_u                                             # (released in stream order: the next block's numbers may take their place)
    res = dict(states=d_st.cpu().numpy().astype(np.int64), energy=energy.cpu().numpy(), family=d_fam.cpu().numpy().astype(np.int64),
               energy0=energy0.cpu().numpy())

    def joined(k, dtype, tail=()):
        return np.concatenate([o[k].cpu().numpy() for o in outs], axis=0).astype(dtype) if outs else np.zeros((0,) + tail, dtype=dtype)

    for k in ('emin', 'wsum', 'w2sum'):
        res[k] = joined(k, np.float64)
    res['survivors'] = joined('survivors', np.int64)
    res['energy_trace'] = joined('energy_trace', np.float64, (M,))
    if record:
        res['parent_trace'] = joined('parent_trace', np.int64, (M,))
    del table
    return res


def anneal_population(solver, betas, sweeps=1, M=None, uniforms=None, record=False, log2Z0=None, steps_per_call=None, seed=None):
    """anneal_population of tnac4o (documented there)."""
    a = check_arguments(solver, betas, sweeps, M, uniforms, log2Z0, steps_per_call, seed)
    if a['fresh'] and a['seed'] is not None:
        rot = None
    elif a['fresh']:
        u = a['uniforms']['init'] if a['uniforms'] is not None else np.random.rand(a['M'], solver.Nx * solver.Ny)
        rot = draw_population(u if isinstance(u, np.ndarray) else u.cpu().numpy(), solver._cell_sizes())
    else:
        st = a['states']
        rot = np.empty_like(st)
        rot[:, solver.order] = st                            # the inverse of _store_result's states[:, order]
    res = anneal_native(solver, rot, a, bool(record))
    b, Mp = a['betas'], a['M']
    solver.anneal_betas = b
    solver.anneal_log2Z = log2Z_path(b, res['emin'], res['wsum'], Mp, a['log2Z0'])
    solver.anneal_free_energy = free_energy_path(b, solver.anneal_log2Z)
    E = np.concatenate([res['energy0'][None, :], res['energy_trace']], axis=0)
    solver.anneal_energy_mean = E.mean(axis=1)
    solver.anneal_heat_capacity = b * b * E.var(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        solver.anneal_ess = res['wsum'] * res['wsum'] / res['w2sum']
    solver.anneal_survivors = res['survivors']
    solver.anneal_family = res['family']
    solver.anneal_rho_t, solver.anneal_family_entropy = family_statistics(res['family'])
    if record:
        solver.anneal_energy_trace, solver.anneal_parent_trace = res['energy_trace'], res['parent_trace']
    solver.states, solver.energy = res['states'][:, solver.order], res['energy']
    solver.probability = solver.sample_log2Z = solver.log2Z_lower = solver.log2Z_estimate = None
    return solver.energy
