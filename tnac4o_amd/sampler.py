"""Driver of tnac4o.sample_boltzmann: configurations drawn from the Boltzmann distribution by the library's sampling walk
(tn_gibbs_sample, csrc/sampler.hip), each with log2 of the probability q(x) it was drawn with, and what follows from those numbers.
Driver of tnac4o.calculate_log_probability as well: the same walk forced along given configurations (tn_gibbs_score), and the host
arithmetic of tnac4o.calculate_free_energy (log2 Z from row contractions over boundary overlaps).

For a sample x drawn with probability q(x) the number  s(x) = -beta E(x) / ln 2 - log2 q(x)  is an estimate of log2 Z:
  * exact contraction: q is the Boltzmann distribution and s(x) = log2 Z for every sample;
  * truncated boundaries: mean s = log2 Z - KL(q || p) / ln 2 <= log2 Z (a variational bound), and mean 2^s is an unbiased estimate
    of Z (importance weights 2^(s - log2 Z)).  The spread of s over the samples measures what the truncation costs.
Z runs over the ACTIVE spins of the model: a spin without any term does not appear in the network (it would add exactly 1 to log2 Z).

The host part (estimators, the layout and validation of the uniform numbers, the chunk planner) is plain numpy and runs without a GPU.
"""
import ctypes as C

import numpy as np

LN2 = float(np.log(2.0))
LDS_BYTES = 150 * 1024                                    # the bound tn_sample_pn holds a cell's table and environments to


def log2z_estimators(energy, log2q, beta):
    """(sample_log2Z (M,), log2Z_lower, log2Z_estimate) of sampled energies and log2 q.  lower = mean of the per-sample values;
    estimate = log2 mean 2^s, evaluated with the maximum taken out (the values are far beyond the range of 2.0**x).  lower <= estimate
    (Jensen); they coincide when all samples agree."""
    s = -float(beta) * np.asarray(energy, dtype=np.float64) / LN2 - np.asarray(log2q, dtype=np.float64)
    if s.ndim != 1 or s.size == 0:
        raise ValueError('energy and log2q must be vectors of the same, non-zero length')
    m = float(np.max(s))
    lower = float(np.mean(s))
    est = m + float(np.log2(np.mean(np.exp2(s - m))))
    return s, lower, max(est, lower)                      # (rounding alone can put the estimate an ulp below the mean of equal values)


def check_uniforms(uniforms, ncell, M):
    """The uniform numbers of a walk: None -> np.random.rand(ncell, M) from numpy's global generator (the stream one rand(M) per cell
    consumes); else a (ncell, M) float64 numpy array or torch tensor of numbers in [0, 1), row = cell in walk order, which is
    returned as it is.  Anything else: ValueError."""
    if uniforms is None:
        return np.random.rand(ncell, M)
    is_np = isinstance(uniforms, np.ndarray)
    if not is_np:
        import torch
        if not isinstance(uniforms, torch.Tensor):
            raise ValueError('uniforms must be None, a numpy array or a torch tensor (got %s)' % type(uniforms).__name__)
    if tuple(uniforms.shape) != (ncell, M):
        raise ValueError('uniforms must have shape (Ny*Nx, M) = (%d, %d), got %s' % (ncell, M, tuple(uniforms.shape)))
    if is_np:
        if uniforms.dtype != np.float64:
            raise ValueError('uniforms must be float64, got %s' % uniforms.dtype)
        ok = bool(np.all((uniforms >= 0.0) & (uniforms < 1.0)))
    else:
        import torch
        if uniforms.dtype != torch.float64:
            raise ValueError('uniforms must be float64, got %s' % uniforms.dtype)
        ok = bool(((uniforms >= 0.0) & (uniforms < 1.0)).all().item())
    if not ok:                                            # (a NaN fails both comparisons)
        raise ValueError('uniforms must lie in [0, 1) (no NaN)')
    return uniforms


def plan_chunk(M, ws_bytes, budget, B=1):
    """Samples per call of the walk: the largest power of two <= M whose workspace ws_bytes(chunk) fits `budget` bytes and whose row
    keys fit int64 (chunk^2 B^2 < 2^63).  MemoryError when not even one sample fits."""
    if M < 1:
        raise ValueError('M must be positive')
    c = 1 << (int(M).bit_length() - 1)
    while c >= 1:
        if c * c * int(B) * int(B) < 2 ** 63 and ws_bytes(c) <= budget:
            return c
        c >>= 1
    raise MemoryError('the sampling walk needs %d bytes of workspace for a single sample, %d are available' % (ws_bytes(1), budget))


def chunk_slices(M, chunk):
    """[(lo, hi)] covering 0 .. M in steps of at most chunk."""
    if chunk is None or int(chunk) != chunk or chunk < 1:
        raise ValueError('chunk must be a positive integer')
    return [(lo, min(lo + int(chunk), M)) for lo in range(0, M, int(chunk))]


def cell_misfit(q, p, Dr, br, running_sum=True):
    """None, or why tn_sample_pn cannot take a cell (its table, the running sum and the environments share the LDS).  running_sum =
    False: the same for tn_score_pn, which keeps the table and the environments only (tn_calc_pn's bound)."""
    front = p * Dr + Dr * br + p * br
    if not running_sum:
        need = (front + q) * 8
        if need > LDS_BYTES:
            return 'the table of %d states and the environments need %d bytes of LDS, tn_score_pn holds %d' % (q, need, LDS_BYTES)
        return None
    need = (max(front, q) + q) * 8
    if need > LDS_BYTES:
        return 'the table of %d states, its running sum and the environments need %d bytes of LDS, tn_sample_pn holds %d' % (q, need, LDS_BYTES)
    return None


def check_states(states, qs):
    """Configurations to score: an integer array (M, len(qs)), M >= 1, entry k of a row in [0, qs[k]).  A signed dtype narrower than 64
    bits is read as unsigned, as the solver stores the 256 states of a cell in int8.  Returns them as int64; anything else: ValueError."""
    qs = np.asarray(qs, dtype=np.int64).reshape(-1)
    if not isinstance(states, np.ndarray):
        raise ValueError('states must be a numpy array of integers (got %s)' % type(states).__name__)
    if states.dtype.kind not in 'iu':
        raise ValueError('states must have an integer dtype, got %s' % states.dtype)
    if states.ndim != 2 or states.shape[1] != qs.size or states.shape[0] < 1:
        raise ValueError('states must have shape (M, Nx*Ny) = (M, %d) with M >= 1, got %s' % (qs.size, tuple(states.shape)))
    if states.dtype.kind == 'i' and states.dtype.itemsize < 8:
        states = np.ascontiguousarray(states).view('u%d' % states.dtype.itemsize)
    if states.dtype == np.uint64 and states.max() > np.uint64(2 ** 62):
        raise ValueError('states: an entry lies outside the states of its cell')
    st = states.astype(np.int64)
    bad = (st < 0) | (st >= qs[None, :])
    if bad.any():
        m, k = np.argwhere(bad)[0]
        raise ValueError('states[%d, %d] = %d lies outside [0, %d), the states of that cell' % (m, k, st[m, k], qs[k]))
    return st


def log2z_from_rows(rows, overlaps, shifts, beta, rows_log2=None, overlaps_log2=None, ends=(1.0, 1.0)):
    """log2 Z from the contractions of tnac4o.calculate_free_energy (host arithmetic only):
        log2 Z = sum_ny log2 |r_ny| - sum_ny log2 |o_ny| - log2 |e_B e_T| - (beta / ln 2) sum shifts
    rows (Ny,): the row contractions r_ny = <rhoB[ny]| row ny |rhoT[ny+1]>, overlaps (Ny-1,): o_ny = <rhoB[ny]|rhoT[ny]>, each as a
    signed number times 2^(its entry of rows_log2 / overlaps_log2; None = 0) -- only magnitudes enter, the norm and sign of every
    interior boundary occur once above and once below the line.  ends: what the two trivial boundaries rhoB[0], rhoT[Ny] contract
    to (1 in magnitude for the solver's).  shifts: the minima the PEPS factors took out of the energy tables (any shape; summed).
    Returns (log2Z, log2 |r| (Ny,), log2 |o| (Ny-1,))."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1)
    o = np.asarray(overlaps, dtype=np.float64).reshape(-1)
    if r.size < 1 or o.size != r.size - 1:
        raise ValueError('need Ny >= 1 row contractions and Ny - 1 overlaps (got %d and %d)' % (r.size, o.size))
    lr = np.zeros(r.size) if rows_log2 is None else np.asarray(rows_log2, dtype=np.float64).reshape(-1)
    lo = np.zeros(o.size) if overlaps_log2 is None else np.asarray(overlaps_log2, dtype=np.float64).reshape(-1)
    if lr.size != r.size or lo.size != o.size:
        raise ValueError('one power-of-two exponent per contraction')
    with np.errstate(divide='ignore'):
        lr = np.log2(np.abs(r)) + lr
        lo = np.log2(np.abs(o)) + lo
        le = float(np.log2(abs(float(ends[0]) * float(ends[1]))))
    net = float(np.sum(lr)) - float(np.sum(lo)) - le
    return net - float(beta) / LN2 * float(np.sum(np.asarray(shifts, dtype=np.float64))), lr, lo


def _walk_table(solver, who, running_sum):
    """(CellTable, B) of a solver whose rhoT is set up, for tn_gibbs_sample (running_sum) or tn_gibbs_score; NotImplementedError
    naming the limit when a cell does not fit."""
    from .beam import CellTable
    Nx = solver.Nx
    B = int(max(np.max(solver.ld), np.max(solver.lr), 2))
    table = CellTable(solver)
    walk = 'the sampling walk, tn_gibbs_sample' if running_sum else 'the scoring walk, tn_gibbs_score'
    if table.misfit is not None:
        raise NotImplementedError('%s: %s (limit of %s)' % (who, table.misfit, walk))
    for k in range(Nx * solver.Ny):
        c = table.cells[k]
        why = cell_misfit(c.q, c.p, c.Dr, c.br, running_sum)
        if why is not None:
            raise NotImplementedError('%s: cell (%d, %d): %s' % (who, k // Nx, k % Nx, why))
    return table, B


def sample_native(solver, M, uniforms=None, chunk=None, seed=None):
    """The walk of tnac4o.sample_boltzmann over solver.rhoT (which must be set up), in column slices of `uniforms` of at most `chunk`
    samples: one upload of the uniform numbers and one read-back of states / energies / log2 q per slice.  seed (an integer, uniforms
    None): the numbers of every slice are filled on the device instead (rng.WALK: row = cell, index = sample), nothing is drawn or
    uploaded.  Stores the results on the solver and returns the energies."""
    import torch
    from . import ops, rng
    from ._lib import lib
    Nx, Ny = solver.Nx, solver.Ny
    ncell = Nx * Ny
    M = int(M)
    if M < 1:
        raise ValueError('M must be positive')
    if seed is None:
        uniforms = check_uniforms(uniforms, ncell, M)
    if chunk is not None:
        chunk_slices(M, chunk)                            # (validates chunk before any device work)
    dev = solver.rhoT[0].A[0].device
    table, B = _walk_table(solver, 'sample_boltzmann', True)
    L = lib()

    def ws_bytes(m):
        return int(L.tn_gibbs_sample_ws_bytes(Nx, Ny, m, table.qmax, table.max_env, table.max_t1, table.max_w))

    if chunk is None:
        chunk = plan_chunk(M, ws_bytes, torch.cuda.mem_get_info(dev)[0] // 2, B)
    elif int(chunk) ** 2 * B * B >= 2 ** 63:
        raise NotImplementedError('sample_boltzmann: chunk^2 x (boundary index range)^2 exceeds int64 (row keys): use a smaller chunk')
    slices = chunk_slices(M, chunk)
    cmax = max(hi - lo for lo, hi in slices)
    wsb = ws_bytes(cmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    d_states = torch.empty((cmax, ncell), dtype=torch.int16, device=dev)
    d_E = torch.empty(cmax, dtype=torch.float64, device=dev)
    d_lq = torch.empty(cmax, dtype=torch.float64, device=dev)
    states = np.empty((M, ncell), dtype=np.int64)
    energy = np.empty(M)
    log2q = np.empty(M)
    globalmin, max_groups = 1.0, 0
    on_device = seed is None and not isinstance(uniforms, np.ndarray)
    if on_device:
        uniforms = uniforms.to(dev).contiguous()
    for lo, hi in slices:
        m = hi - lo
        if seed is not None:
            u = rng.fill(seed, rng.WALK, 0, (ncell, m), first=lo, dev=dev)
            u_ptr, ldu = u.data_ptr(), m
        elif on_device:
            u_ptr, ldu, u = uniforms.data_ptr() + lo * 8, M, uniforms
        else:
            u = torch.as_tensor(np.ascontiguousarray(uniforms[:, lo:hi])).to(dev)
            u_ptr, ldu = u.data_ptr(), m
        gmin, mg = C.c_double(0.0), C.c_int64(0)
        ops.check(L.tn_gibbs_sample(Nx, Ny, C.cast(table.cells, C.c_void_p), m, B, u_ptr, ldu, d_states.data_ptr(), d_E.data_ptr(),
                                    d_lq.data_ptr(), C.byref(gmin), C.byref(mg), ws.data_ptr(), wsb, ops._stream()))
        states[lo:hi] = d_states[:m].cpu().numpy()
        energy[lo:hi] = d_E[:m].cpu().numpy()
        log2q[lo:hi] = d_lq[:m].cpu().numpy()
        globalmin, max_groups = min(globalmin, float(gmin.value)), max(max_groups, int(mg.value))
        del u
    del ws, table
    solver._store_result(energy, states, log2q, 0, 0, globalmin)
    solver.sample_log2Z, solver.log2Z_lower, solver.log2Z_estimate = log2z_estimators(energy, log2q, solver.beta)
    solver.sample_max_groups = max_groups
    return energy


def score_native(solver, states_rot, chunk=None, cells=False):
    """The walk of tnac4o.calculate_log_probability over solver.rhoT (which must be set up): tn_gibbs_score along the configurations
    states_rot (M, Ny*Nx) integers in the lattice order of the current rotation, every entry inside the states of its cell, in row
    slices of at most `chunk` configurations: one upload of the states and one read-back of energies / log2 q (/ the per-cell
    increments) per slice.  The chunk planner, the slices and the CellTable are sample_native's.  Returns (log2 q (M,), energy (M,),
    cell log2 q (M, Ny*Nx) in walk order or None, smallest table flag, largest number of distinct boundary rows); stores nothing."""
    import torch
    from . import ops
    from ._lib import lib
    Nx, Ny = solver.Nx, solver.Ny
    ncell = Nx * Ny
    states_rot = np.asarray(states_rot)
    M = int(states_rot.shape[0])
    if states_rot.ndim != 2 or states_rot.shape[1] != ncell or M < 1:
        raise ValueError('states must have shape (M, Nx*Ny) with M >= 1')
    if chunk is not None:
        chunk_slices(M, chunk)                            # (validates chunk before any device work)
    dev = solver.rhoT[0].A[0].device
    table, B = _walk_table(solver, 'calculate_log_probability', False)
    L = lib()

    def ws_bytes(m):
        return int(L.tn_gibbs_score_ws_bytes(Nx, Ny, m, table.qmax, table.max_env, table.max_t1, table.max_w))

    if chunk is None:
        chunk = plan_chunk(M, ws_bytes, torch.cuda.mem_get_info(dev)[0] // 2, B)
    elif int(chunk) ** 2 * B * B >= 2 ** 63:
        raise NotImplementedError('calculate_log_probability: chunk^2 x (boundary index range)^2 exceeds int64 (row keys): use a smaller chunk')
    slices = chunk_slices(M, chunk)
    cmax = max(hi - lo for lo, hi in slices)
    wsb = ws_bytes(cmax)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    # one result buffer per slice: energies, log2 q and (cells) the increments travel back in one copy
    d_out = torch.empty(cmax * (2 + (ncell if cells else 0)), dtype=torch.float64, device=dev)
    st16 = np.ascontiguousarray(states_rot, dtype=np.int16)
    energy = np.empty(M)
    log2q = np.empty(M)
    cell_lq = np.empty((M, ncell)) if cells else None
    globalmin, max_groups = 1.0, 0
    for lo, hi in slices:
        m = hi - lo
        d_st = torch.as_tensor(st16[lo:hi]).to(dev)
        base = d_out.data_ptr()
        gmin, mg = C.c_double(0.0), C.c_int64(0)
        ops.check(L.tn_gibbs_score(Nx, Ny, C.cast(table.cells, C.c_void_p), m, B, d_st.data_ptr(), base, base + m * 8,
                                   base + 2 * m * 8 if cells else None, C.byref(gmin), C.byref(mg), ws.data_ptr(), wsb, ops._stream()))
        host = d_out[:m * (2 + (ncell if cells else 0))].cpu().numpy()
        energy[lo:hi] = host[:m]
        log2q[lo:hi] = host[m:2 * m]
        if cells:
            cell_lq[lo:hi] = host[2 * m:].reshape(m, ncell)
        globalmin, max_groups = min(globalmin, float(gmin.value)), max(max_groups, int(mg.value))
        del d_st
    del ws, table
    return log2q, energy, cell_lq, globalmin, max_groups
