"""Driver of tnac4o.relax_lines: sweeps that resample (heat bath) or minimise (quench) WHOLE lattice rows and columns exactly with the
library's tn_line_sweep (csrc/lines.hip).

Under E = sum over the cells of Es[s] + E1[s, left] + E4[s, up] one lattice row is a chain of cells once the rows above and below are
given, and so is a column: its conditional law is sampled exactly by one forward pass of messages and one backward pass of draws, its
conditional minimum found by the same recursion in (min, +).  Rows (columns) of one parity do not interact: a pass updates the even
lines, then the odd ones.  No boundary MPS and no contraction is involved; the call reads the energy tables relax_samples reads.

The host part (argument rules, layout of the uniform numbers, the range guard of the linear-domain heat bath) is plain numpy and runs
without a GPU.
"""
import ctypes as C

import numpy as np

from .relax import QUENCH_BLOCK, EnergyCells, check_relax_arguments
from .sampler import chunk_slices, plan_chunk

LINES = {'rows': 0, 'columns': 1, 'both': 2}
BETA_RANGE = 300.0                                        # the range guard of tn_line_sweep: beta (max - min) of every chain table


def passes(lines):
    """Passes per sweep: 2 for 'both', else 1."""
    return 2 if lines == 'both' else 1


def check_line_arguments(mode, lines, sweeps, beta, uniforms, max_sweeps, seed=None):
    """The argument rules of tnac4o.relax_lines that need neither the states nor a device: relax.check_relax_arguments and `lines`.
    Returns (library mode, library lines, sweeps or None, beta); ValueError otherwise."""
    if not isinstance(lines, str) or lines not in LINES:
        raise ValueError("lines must be 'rows', 'columns' or 'both' (got %r)" % (lines,))
    lib_mode, nsw, b = check_relax_arguments(mode, sweeps, beta, uniforms, max_sweeps, seed)
    return lib_mode, LINES[lines], nsw, b


def check_line_uniforms(uniforms, sweeps, P, ncell, M):
    """The uniform numbers of `sweeps` heat-bath line sweeps of P passes: None -> np.random.rand(sweeps, P, ncell, M) from numpy's
    global generator; else a (sweeps, P, ncell, M) float64 numpy array or torch tensor of numbers in [0, 1) -- entry (j, p, k, m) serves
    sweep j, pass p, cell k in walk order of the current rotation, sample m -- returned as it is.  Anything else: ValueError."""
    shape = (int(sweeps), int(P), int(ncell), int(M))
    if uniforms is None:
        return np.random.rand(*shape)
    is_np = isinstance(uniforms, np.ndarray)
    if not is_np:
        import torch
        if not isinstance(uniforms, torch.Tensor):
            raise ValueError('uniforms must be None, a numpy array or a torch tensor (got %s)' % type(uniforms).__name__)
    if tuple(uniforms.shape) != shape:
        raise ValueError('uniforms must have shape (sweeps, passes, Ny*Nx, M) = %s, got %s' % (shape, tuple(uniforms.shape)))
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


def chain_range(solver, lines):
    """The largest max - min over the chain tables the passes of `lines` read in the current rotation (E1 right of column 0 for rows,
    E4 below row 0 for columns), from the solver's host tables; 0.0 without one."""
    r = 0.0
    for ny in range(solver.Ny):
        for nx in range(solver.Nx):
            _, E1, E4 = solver._cell_energies(ny, nx)
            if lines in ('rows', 'both') and nx > 0:
                r = max(r, float(np.max(E1) - np.min(E1)))
            if lines in ('columns', 'both') and ny > 0:
                r = max(r, float(np.max(E4) - np.min(E4)))
    return r


def check_range_guard(solver, lines, beta):
    """The range guard of the linear-domain heat bath (tn_line_sweep): beta (max - min) <= 300 for every chain table; ValueError beyond."""
    r = chain_range(solver, lines)
    if not beta * r <= BETA_RANGE:
        raise ValueError('range guard: beta x (max - min) of a chain table is %g, above %g: the linear-domain heat bath of whole lines '
                         'is not safe at this beta (use relax_samples, or a smaller beta)' % (beta * r, BETA_RANGE))


def lines_native(solver, states_rot, mode, lines, beta, sweeps, uniforms=None, chunk=None, max_sweeps=64, seed=None):
    """tn_line_sweep over the configurations states_rot (M, Ny*Nx) integers in the lattice order of the current rotation, every entry
    inside the states of its cell, in row slices of at most `chunk` configurations.  mode: 0 heat bath / 1 quench; lines: 0 rows /
    1 columns / 2 both; sweeps: their number, or None (quench): blocks of QUENCH_BLOCK sweeps until no line of the slice moves in the
    last one, at most max_sweeps.  uniforms: what check_line_uniforms returned (heat bath), None (quench, or a heat bath with seed: an
    integer, the numbers of every slice are then filled on the device -- rng.RELAX_LINE: row = (sweep * P + pass) * Ny*Nx + cell, index =
    configuration).  Per slice: one upload of its states and of its uniform numbers, one read-back of everything it returns.
    Returns (states (M, Ny*Nx) int64 in the same order, energy, energy before, moves, last moves, sweeps run); stores nothing."""
    import torch
    from . import ops, rng
    from ._lib import lib
    Nx, Ny = solver.Nx, solver.Ny
    ncell = Nx * Ny
    P = 2 if lines == 2 else 1
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
        u = 0 if (mode == 1 or on_device) else nsw * P * ncell * m * 8
        return int(L.tn_line_sweep_ws_bytes(Nx, Ny, m)) + out_bytes(m) + m * 4 + u

    if chunk is None:
        chunk = plan_chunk(M, all_bytes, torch.cuda.mem_get_info(dev)[0] // 2)
    slices = chunk_slices(M, chunk)
    cmax = max(hi - lo for lo, hi in slices)
    wsb = int(L.tn_line_sweep_ws_bytes(Nx, Ny, cmax))
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
            ops.check(L.tn_line_sweep(Nx, Ny, cells, m, p_st, mode, lines, beta, n, u_ptr, ldu, E_ptr, mv_ptr, last_ptr, ws.data_ptr(), wsb,
                                      ops._stream()))

        call(0, None, 0, p_before, None, None, mode=1)      # no sweep: the energies of the states as they arrive
        u = None
        if mode == 0:
            if seed is not None:
                u = rng.fill(seed, rng.RELAX_LINE, 0, (nsw * P * ncell, m), first=lo, dev=dev)
                u_ptr, ldu = u.data_ptr(), m
            elif on_device:
                u_ptr, ldu = uniforms.data_ptr() + lo * 8, M
            else:
                u = torch.as_tensor(np.ascontiguousarray(uniforms[..., lo:hi])).to(dev)
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
