"""Driver of tnac4o.relax_samples: sweeps of block updates of whole cells over given configurations with the library's tn_cell_sweep
(csrc/relax.hip) -- a heat bath that leaves the Boltzmann law invariant, or a quench to the conditional minimum of every cell.

The energy of a configuration is a sum over the cells of Es[s] + E1[s, left] + E4[s, up] (tnac4o._cell_energies), so the conditional law
of one whole cell given its four neighbours is a table of q numbers, and the cells of one checkerboard colour are conditionally
independent of each other: one sweep updates colour 0 (ny + nx even), then colour 1.  No boundary MPS and no contraction is involved;
the call reads the energy tables alone.

The host part (validation and layout of the uniform numbers, the argument checks) is plain numpy and runs without a GPU.
"""
import ctypes as C

import numpy as np

from .sampler import chunk_slices, plan_chunk

MODES = {'heat_bath': 0, 'quench': 1}
QUENCH_BLOCK = 4                                          # sweeps per call while a quench runs until nothing moves


def check_sweep_uniforms(uniforms, sweeps, ncell, M):
    """The uniform numbers of `sweeps` heat-bath sweeps: None -> np.random.rand(sweeps, ncell, M) from numpy's global generator; else a
    (sweeps, ncell, M) float64 numpy array or torch tensor of numbers in [0, 1) -- entry (j, k, m) serves sweep j, cell k in walk order
    of the current rotation, sample m -- which is returned as it is.  Anything else: ValueError (the rules of sampler.check_uniforms)."""
    shape = (int(sweeps), int(ncell), int(M))
    if uniforms is None:
        return np.random.rand(*shape)
    is_np = isinstance(uniforms, np.ndarray)
    if not is_np:
        import torch
        if not isinstance(uniforms, torch.Tensor):
            raise ValueError('uniforms must be None, a numpy array or a torch tensor (got %s)' % type(uniforms).__name__)
    if tuple(uniforms.shape) != shape:
        raise ValueError('uniforms must have shape (sweeps, Ny*Nx, M) = %s, got %s' % (shape, tuple(uniforms.shape)))
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


def check_relax_arguments(mode, sweeps, beta, uniforms, max_sweeps, seed=None):
    """The argument rules of tnac4o.relax_samples that need neither the states nor a device: (library mode, sweeps or None, beta).
    seed: under rng.check_seed, not together with uniforms and not with mode='quench'.  ValueError otherwise."""
    from .rng import check_seed_alone
    if mode not in MODES:
        raise ValueError("mode must be 'heat_bath' or 'quench' (got %r)" % (mode,))
    if check_seed_alone(seed, uniforms) is not None and mode == 'quench':
        raise ValueError("seed must be None with mode='quench' (a quench draws nothing)")
    if sweeps is None:
        if mode != 'quench':
            raise ValueError("sweeps=None (until nothing moves) needs mode='quench'")
        if int(max_sweeps) != max_sweeps or max_sweeps < 1:
            raise ValueError('max_sweeps must be a positive integer')
    elif int(sweeps) != sweeps or sweeps < 0:
        raise ValueError('sweeps must be a non-negative integer (or None in quench mode)')
    if mode == 'quench' and uniforms is not None:
        raise ValueError("uniforms must be None with mode='quench' (a quench draws nothing)")
    beta = float(beta)
    if mode == 'heat_bath' and not (beta > 0.0 and np.isfinite(beta)):
        raise ValueError('beta must be positive and finite')
    return MODES[mode], (None if sweeps is None else int(sweeps)), beta


class EnergyCells:
    """The tn_beam_cell array of a solver with the ENERGY part alone (include/tnpeps.h: what tn_cell_sweep reads), row-major in the
    lattice of the current rotation: index and energy tables of beam.SiteTables, no PEPS factor and no boundary MPS -- rhoT is not
    needed.  cells: the ctypes array; keep: the tables the pointers were taken from (they must outlive the call)."""

    def __init__(self, solver, dev):
        from .beam import SiteTables, _Cell
        Nx, Ny = solver.Nx, solver.Ny
        ising = solver.mode == 'Ising'
        tabs = {(ny, nx): SiteTables(solver, ny, nx, dev) for ny in range(Ny) for nx in range(Nx)}
        self.cells = (_Cell * (Nx * Ny))()
        self.keep = tabs
        for (ny, nx), tb in tabs.items():
            c = self.cells[ny * Nx + nx]
            c.down, c.right, c.Es = tb.down.data_ptr(), tb.right.data_ptr(), tb.Es.data_ptr()
            c.E1 = tb.E1.data_ptr() if nx > 0 else None
            c.E4 = tb.E4.data_ptr() if ny > 0 else None
            c.left_map = tabs[(ny, nx - 1)].right.data_ptr() if (ising and nx > 0) else None
            c.up_map = tabs[(ny - 1, nx)].down.data_ptr() if (ising and ny > 0) else None
            c.q = tb.q
            c.e1cols = tb.E1.shape[1] if tb.E1.dim() == 2 else 1
            c.e4cols = tb.E4.shape[1] if tb.E4.dim() == 2 else 1


def relax_native(solver, states_rot, mode, beta, sweeps, uniforms=None, chunk=None, max_sweeps=64, seed=None):
    """tn_cell_sweep over the configurations states_rot (M, Ny*Nx) integers in the lattice order of the current rotation, every entry
    inside the states of its cell, in row slices of at most `chunk` configurations.  mode: 0 heat bath / 1 quench; sweeps: their
    number, or None (quench): blocks of QUENCH_BLOCK sweeps until no cell of the slice moves in the last one, at most max_sweeps.
    uniforms: what check_sweep_uniforms returned (heat bath), None (quench, or a heat bath with seed: an integer, the numbers of every
    slice are then filled on the device -- rng.RELAX_SWEEP: row = sweep * Ny*Nx + cell, index = configuration).  Per slice: one upload of
    its states and of its uniform numbers, one read-back of everything it returns (the quench until nothing moves also reads one flag
    per block).
    Returns (states (M, Ny*Nx) int64 in the same order, energy, energy before, moves, last moves, sweeps run); stores nothing."""
    import torch
    from . import ops, rng
    from ._lib import lib
    Nx, Ny = solver.Nx, solver.Ny
    ncell = Nx * Ny
    states_rot = np.asarray(states_rot)
    M = int(states_rot.shape[0])
    if states_rot.ndim != 2 or states_rot.shape[1] != ncell or M < 1:
        raise ValueError('states must have shape (M, Nx*Ny) with M >= 1')
    if chunk is not None:
        chunk_slices(M, chunk)                            # (validates chunk before any device work)
    dev = torch.device('cuda', torch.cuda.current_device())
    table = EnergyCells(solver, dev)
    L = lib()
    on_device = uniforms is not None and not isinstance(uniforms, np.ndarray)
    nsw = 0 if sweeps is None else int(sweeps)

    def out_bytes(m):                                     # energies before / after, moves, last moves, states
        return m * 24 + m * ncell * 2

    def all_bytes(m):
        u = 0 if (mode == 1 or on_device) else nsw * ncell * m * 8
        return int(L.tn_cell_sweep_ws_bytes(Nx, Ny, m)) + out_bytes(m) + m * 4 + u

    if chunk is None:
        chunk = plan_chunk(M, all_bytes, torch.cuda.mem_get_info(dev)[0] // 2)
    slices = chunk_slices(M, chunk)
    cmax = max(hi - lo for lo, hi in slices)
    wsb = int(L.tn_cell_sweep_ws_bytes(Nx, Ny, cmax))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    d_out = torch.empty(out_bytes(cmax), dtype=torch.uint8, device=dev)
    d_mv = torch.empty(cmax, dtype=torch.int32, device=dev)
    st16 = np.ascontiguousarray(states_rot, dtype=np.int16)
    states = np.empty((M, ncell), dtype=np.int64)
    energy, before = np.empty(M), np.empty(M)
    moves, last = np.empty(M, dtype=np.int64), np.empty(M, dtype=np.int64)
    if on_device:
        uniforms = uniforms.to(dev).contiguous()
    cells = C.cast(table.cells, C.c_void_p)
    swept = 0
    for lo, hi in slices:
        m = hi - lo
        base = d_out.data_ptr()
        p_before, p_E, p_moves, p_last, p_st = base, base + 8 * m, base + 16 * m, base + 20 * m, base + 24 * m
        d_st = d_out[24 * m:24 * m + 2 * m * ncell].view(torch.int16)
        d_st.copy_(torch.as_tensor(st16[lo:hi]).reshape(-1))
        d_moves = d_out[16 * m:20 * m].view(torch.int32)
        d_last = d_out[20 * m:24 * m].view(torch.int32)
        d_moves.zero_()
        d_last.zero_()

        def call(n, u_ptr, ldu, E_ptr, mv_ptr, last_ptr, mode=mode):
            ops.check(L.tn_cell_sweep(Nx, Ny, cells, m, p_st, mode, beta, n, u_ptr, ldu, E_ptr, mv_ptr, last_ptr, ws.data_ptr(), wsb, ops._stream()))

        call(0, None, 0, p_before, None, None, mode=1)      # no sweep: the energies of the states as they arrive
        u = None
        if mode == 0:
            if seed is not None:
                u = rng.fill(seed, rng.RELAX_SWEEP, 0, (nsw * ncell, m), first=lo, dev=dev)
                u_ptr, ldu = u.data_ptr(), m
            elif on_device:
                u_ptr, ldu = uniforms.data_ptr() + lo * 8, M
            else:
                u = torch.as_tensor(np.ascontiguousarray(uniforms[:, :, lo:hi])).to(dev)
                u_ptr, ldu = u.data_ptr(), m
            call(nsw, u_ptr, ldu, p_E, p_moves, p_last)
            done = nsw
        elif sweeps is not None:
            call(nsw, None, 0, p_E, p_moves, p_last)
            done = nsw
        else:
            done = 0
            while True:
                n = min(QUENCH_BLOCK, int(max_sweeps) - done)
                call(n, None, 0, p_E, d_mv.data_ptr(), p_last)
                d_moves += d_mv[:m]
                done += n
                if done >= int(max_sweeps) or not bool(d_last.any().item()):
                    break
        host = d_out[:out_bytes(m)].cpu().numpy()
        before[lo:hi] = host[:8 * m].view(np.float64)
        energy[lo:hi] = host[8 * m:16 * m].view(np.float64)
        moves[lo:hi] = host[16 * m:20 * m].view(np.int32)
        last[lo:hi] = host[20 * m:24 * m].view(np.int32)
        states[lo:hi] = host[24 * m:].view(np.int16).reshape(m, ncell)
        swept = max(swept, done)
        del u
    del ws, table
    return states, energy, before, moves, last, swept
