#!/usr/bin/env python3
"""Headline benchmark: boundary-MPS PEPS contraction, ms per sweep, chimera L=2048, chi=64 (BASELINE.json).

One sweep = one `_setup_rhoT` (reference tnac4o.py:1674-1695): for each of the 16 rows, build the row MPO, absorb it
into the boundary MPS and compress back to chi=64 with the defaults of search_ground_state (graduate_truncation,
tolS=1e-16, tolV=1e-10, max_sweeps=20).  Synthetic chimera couplings (seed 20260004).

One step = the sweeps of the 4 lattice rotations of ONE instance (the reference's 4-rotation loop, examples/e06:97-109),
`value` = wall ms of a step / 4.  N = 1: the 4 chains are interleaved on 4 HIP streams of the one GPU.  N > 1 (`--mode
sweep`, the default) is the north-star decomposition of the same job: the rotations are dealt to min(N, 4) teams of
N / teams ranks; a team's first rank sweeps its rotation(s), and when a team has partners (N = 8: 4 rotations x 2 beam
shards) it broadcasts the boundary MPS of every row to them over RCCL inside the timed step (what the beam shards need
before the search can start).  Same total work for every N => "scaling": "strong".  `--mode replicas` keeps the round-1
form (every rank its own instance, no collective, "weak").  With `--full`, after the timed steps one full 4-rotation
ground-state search (solve_rotations: sweeps + M=1024 beam + RCCL gather at merge time) is timed once as `full_solve`.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the --steps steps and prints the line (`metric`,
`value`, `unit`, `ms_per_step`, ...).  `--full` adds everything else, outside the timed steps unless stated: the
single-chain sweeps with events on every launch (kernel and phase tables, launch census), `roofline` (the kernel family
with the largest summed duration, timed with HIP events on its launch stream inside the timed region), `full_solve`, and
`cpu_baseline` (the CPU oracle on a bounded sample of the same sweep, whole bulk rows, on the host cores).

`--dump-outputs DIR` writes what the last timed step computed (the boundary MPS of every row of rank 0's rotations) as
float64 .npy files; the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')   # one hardware queue per chain (see tnac4o_amd/__init__.py); before torch touches HIP

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch         # noqa: E402

FAMILIES = ['gemm_kernel<128,128>', 'gemm_kernel<128,32>', 'gemm_kernel<32,128>', 'gemm_kernel<64,64>',
            'splitk_reduce_kernel', 'absorb_kernel', 'gram_partial_kernel', 'Jacobi rounds (svdl_kernel; eig_small3_kernel on separate launches)',
            'rows_times_small_kernel', 'small_t_times_vecs_kernel', 'panel step (cq_fused_kernel, sq_kernel; cq_gram / cq_pass / cq_post on the six-launch chain)',
            'lu_reconstruct_kernel', 'qr_aux (diag_qr, assemble_R, init_Q, norms, copies)',
            'svd_aux (norms, init, gather)', 'misc (nfactor, scaling, builders)']
COUNTERS = {'qr_nominal': 15, 'svd_nominal': 16, 'svd_stream': 17, 'svdvals_nominal': 18, 'svd_rounds': 19}   # counter-only families
PHASES = ['gemm_var (attach / projector / environment GEMMs, scaling)', 'absorb', 'qr', 'svd_trunc', 'svdvals', 'mpo_build']
MFMA_FAM = {0, 1, 2, 3}
PMC_ALIASES = {7: ('Jacobi rounds (svdl_kernel)', 'eig_small_kernel'),
               10: ('panel step (cq_fused_kernel, sq_kernel)', 'panel step (cq_fused / cq_gram / cq_pass / cq_post)')}   # keys of profiles/rNN_pmc_traffic.json
SERIAL_FAM = {7: ('svdl_kernel', 'round of the block-Jacobi SVD (pair Gram matrices from LDS, up to 2 x 63 Jacobi steps of 32 plane rotations on the 64 x 64 '
                   'Gram matrix or its Newton-like fast path, rotation of the vectors in LDS; all rounds of a call in ONE launch, svdl_kernel)', None),
              10: ('cq_fused_kernel',
                   'launch of the panel step (ONE per panel of up to 4096 rows: Gram, 32-step one-wave Cholesky, substitution passes, '
                   'Householder reconstruction and reflector products behind in-kernel barriers; six per taller panel, of which the '
                   'passes after convergence return at once); each is a chain of dependent memory round trips and one-wave factorisations', 1)}
PEAK_F64_MFMA_TFLOPS = 78.6      # MI355X fp64 matrix peak (vendor figure quoted in SURVEY.md §7; not in the microarch guide)
PEAK_HBM_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
WORKLOADS = {'chimera2048': ('Ising', 16, 20260004, 3.0), 'chimera512': ('Ising', 8, 20260003, 3.0),
             'chimera128': ('Ising', 4, 20260002, 3.0), 'rmf64': ('RMF', 64, 20260005, 1.0)}


def _get(lib, phase, f):
    calls, ms, fl, by = C.c_uint64(0), C.c_double(0), C.c_double(0), C.c_double(0)
    lib.tn_profile_get_phase(phase, f, C.byref(calls), C.byref(ms), C.byref(fl), C.byref(by))
    return dict(calls=int(calls.value), ms=ms.value, flops=fl.value, bytes=by.value)


def profile_totals(lib, phase=-1):
    return [dict(kernel=FAMILIES[f], **_get(lib, phase, f)) for f in range(len(FAMILIES))]


def phase_report(lib, pmc):
    """Sub-timers of SURVEY.md §8(d): summed kernel durations of one single-chain sweep split by the entry point that
    issued the launch, plus the three SVD-step roofline figures and the nominal QR rate."""
    rep = {}
    for ph, name in enumerate(PHASES):
        t = profile_totals(lib, ph)
        rep[name] = {'kernel_ms': round(sum(x['ms'] for x in t), 3), 'launches': sum(x['calls'] for x in t)}
    qr, svd, stream, sv = (_get(lib, -1, COUNTERS[k]) for k in ('qr_nominal', 'svd_nominal', 'svd_stream', 'svdvals_nominal'))
    t_qr = rep['qr']['kernel_ms'] * 1e-3
    t_svd = rep['svd_trunc']['kernel_ms'] * 1e-3
    if t_qr > 0:
        rep['qr'].update({'calls': qr['calls'], 'nominal_tflops': qr['flops'] / t_qr / 1e12,
                          'frac_of_f64_mfma_peak': qr['flops'] / t_qr / 1e12 / PEAK_F64_MFMA_TFLOPS,
                          'compulsory_GBps': qr['bytes'] / t_qr / 1e9,
                          'note': 'nominal counts use the full (m, n) of every call; the truncating passes stop early (rank_tol)'})
    if t_svd > 0:
        tert = None
        if pmc and pmc.get('svd_step'):
            tert = pmc['svd_step']
        rep['svd_trunc'].update({
            'calls': svd['calls'], 'executed_sweeps': stream['calls'],
            'nominal_tflops': svd['flops'] / t_svd / 1e12,
            'hbm_primary_compulsory_GBps': svd['bytes'] / t_svd / 1e9,
            'hbm_primary_frac': svd['bytes'] / t_svd / 1e9 / PEAK_HBM_GBS,
            'hbm_secondary_jacobi_streaming_model_GBps': stream['bytes'] / t_svd / 1e9,
            'hbm_secondary_frac': stream['bytes'] / t_svd / 1e9 / PEAK_HBM_GBS,
            'hbm_tertiary_pmc': tert,
            'hbm_tertiary_pmc_one_launch_form': (pmc or {}).get('whole_call', {}).get('tn_svd_trunc_192x900_one_launch'),
            'note': 'block Jacobi (32-wide blocks): the pair Gram/apply are MFMA GEMMs on L2/Infinity-Cache-resident data, '
                    'so the streaming model of a column-pair Jacobi overstates the bytes actually moved; the step is '
                    'latency-bound (eig_small: one workgroup per block pair), not HBM-bound'})
    if sv['calls']:
        rep['svdvals'].update({'calls': sv['calls']})
    return rep


def cpu_model():
    try:
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.startswith('model name'):
                    return line.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


def load_pmc():
    for name in ('r05_pmc_traffic.json', 'r04_pmc_traffic.json', 'r03_pmc_traffic.json', 'r02_pmc_traffic.json', 'r01_pmc_traffic.json'):
        try:
            d = json.load(open(os.path.join(ROOT, 'profiles', name)))
            d['file'] = 'profiles/' + name
            return d
        except (OSError, ValueError):
            continue
    return None


DUMP_SAMPLE_BYTES = 48 << 20       # the sampled site-tensor elements; with the small arrays the dump stays under 64 MB


def dump_outputs(out_dir, solvers, rots):
    """What the timed path hands its caller, for each lattice rotation r swept on this rank: the boundary MPS rhoT[ny] of
    every row ny (site tensors A[nx] of shape (D[nx], d, D[nx + 1]), the accumulated power-of-two norm factor normC, the bond
    dimensions D) and the sweep's rhoT_overlap / rhoT_discarded.  The site tensors (up to 8 MB each at L = 2048) enter as a
    fixed sample: K elements of each at indices drawn by a generator seeded with (r, ny, nx), K set by the arguments alone.
    Files, float64, Ny rows each:
        rot<r>_sites.npy      (Ny, Nx, K)     sampled elements of A[nx] of rhoT[ny]
        rot<r>_bond_dims.npy  (Ny, Nx + 1)    D of rhoT[ny]
        rot<r>_log2_normC.npy (Ny,)           log2 normC of rhoT[ny]
        rot<r>_overlap.npy, rot<r>_discarded.npy (Ny,)"""
    os.makedirs(out_dir, exist_ok=True)
    if not solvers:
        return
    K = max(1, min(2048, DUMP_SAMPLE_BYTES // (8 * sum(s.Ny * s.Nx for s in solvers))))
    for r, s in zip(rots, solvers):
        Ny, Nx = s.Ny, s.Nx
        dev = s.rhoT[0].A[0].device
        sites = torch.empty((Ny, Nx, K), dtype=torch.float64, device=dev)
        log2_normC = np.zeros(Ny)
        for ny in range(Ny):
            psi = s.rhoT[ny]
            for nx, A in enumerate(psi.A):
                idx = np.random.default_rng([r, ny, nx]).integers(0, A.numel(), K)
                sites[ny, nx] = A.reshape(-1)[torch.from_numpy(idx).to(dev)]
            if psi._nfs:
                log2_normC[ny] = float(torch.stack([f[0] for f in psi._nfs]).log2().sum())
        out = {'sites': sites.cpu().numpy(),
               'bond_dims': np.array([s.rhoT[ny].D for ny in range(Ny)], dtype=np.float64),
               'log2_normC': log2_normC,
               'overlap': np.array([float(s.rhoT_overlap[ny]) for ny in range(Ny)]),
               'discarded': np.array([float(s.rhoT_discarded[ny]) for ny in range(Ny)])}
        for name, a in out.items():
            np.save(os.path.join(out_dir, 'rot%d_%s.npy' % (r, name)), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--workload', default='chimera2048', choices=sorted(WORKLOADS))
    ap.add_argument('--L', type=int, default=None, choices=[128, 512, 2048], help='shorthand for --workload chimera<L>')
    ap.add_argument('--chi', type=int, default=None, help='bond dimension (default 64; 128 for rmf64)')
    ap.add_argument('--mode', default='sweep', choices=['sweep', 'replicas'],
                    help='sweep: one instance, rotations (and beam partners) sharded over the ranks, strong scaling; '
                         'replicas: every rank its own instance, no collective, weak scaling')
    ap.add_argument('--cpu-rows', type=int, default=2, help='whole bulk rows (apply_mpo + compress_mps) timed on the CPU oracle (0 disables)')
    ap.add_argument('--concurrent', type=int, default=4,
                    help='N = 1: lattice rotations of the instance interleaved on the GPU, one stream each (4 = the full step)')
    ap.add_argument('--no-profile', action='store_true')
    ap.add_argument('--sample', type=int, default=8,
                    help='in the timed region bracket every n-th launch of the dominant kernel family with events')
    ap.add_argument('--no-search', action='store_true', help='skip the (untimed) full ground-state search figure')
    ap.add_argument('--beam-shards', default='auto',
                    help="ranks per rotation team when --gpus exceeds the number of rotations: 'auto' (default) = 1, i.e. one working rank per "
                         "rotation and the other ranks idle in the timed sweep step (a sweep is one sequential chain: a partner has nothing "
                         "to do there but receive the boundary MPS); an integer forces teams of that size, whose owners broadcast the boundary "
                         "MPS to their beam partners over RCCL inside the timed step and whose search is walked by the whole team in the "
                         "library (tn_beam_search_team: the conditional tables of a site-step split over the ranks; DESIGN.md section 6)")
    ap.add_argument('--nrot', type=int, default=4, help='lattice rotations of the instance (4 = the reference driver; fewer only for rehearsals)')
    ap.add_argument('--rehearse-one-gpu', action='store_true',
                    help='multi-rank rehearsal on a single GPU: every rank uses cuda:0 and the exchange runs over gloo')
    ap.add_argument('--force-dist', action='store_true',
                    help='initialise the RCCL process group even with one rank (rehearses the multi-GPU code path on one GPU)')
    ap.add_argument('--full', action='store_true',
                    help='also measure what the headline does not need: kernel / phase tables and roofline (--no-profile drops them), '
                         'the full ground-state search (--no-search) and the CPU baseline (--cpu-rows)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps write what the last one computed to DIR/<name>.npy (see dump_outputs)')
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit('--steps must be at least 1')
    if not args.full:
        args.no_profile, args.no_search, args.cpu_rows = True, True, 0
    if args.L:
        args.workload = 'chimera%d' % args.L
    kind, n, seed, beta = WORKLOADS[args.workload]
    chi = args.chi or (128 if kind == 'RMF' else 64)

    # stdout carries exactly one JSON line (rank 0): everything the libraries print while we work (RCCL's version banner
    # goes to stdout) is routed to stderr, and the real stdout is restored just before the line is written
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if args.rehearse_one_gpu:
        local = 0
    torch.cuda.set_device(local)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        for k, v in (('RANK', '0'), ('WORLD_SIZE', '1'), ('MASTER_PORT', '29533')):
            os.environ.setdefault(k, v)
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if args.rehearse_one_gpu:
            dist.init_process_group('gloo')
        else:
            dist.init_process_group('nccl', device_id=torch.device('cuda', local))

    import tnac4o_amd
    from tnac4o_amd import _lib, parallel
    from tnac4o_amd.auxx import synthetic_chimera, synthetic_rmf
    lib = _lib.lib()
    pmc = load_pmc() if args.full else None
    replicas = args.mode == 'replicas'
    inst_seed = seed + (rank if replicas else 0)
    J = synthetic_chimera(n, n, inst_seed) if kind == 'Ising' else synthetic_rmf(n, n, 8, inst_seed)
    kw = dict(graduate_truncation=True, Dmax=chi, tolS=1e-16, tolV=1e-10, max_sweeps=20)
    NROT = max(1, min(4, args.nrot))

    def make(rot=0):
        if kind == 'Ising':
            s = tnac4o_amd.tnac4o(mode='Ising', Nx=n, Ny=n, Nc=8, J=J, beta=beta)
        else:
            s = tnac4o_amd.tnac4o(mode='RMF', Nx=n, Ny=n, J=J, beta=beta)
        if rot % 4:
            s.rotate_graph(rot % 4)
        return s

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- who does what (sweep mode): teams of B = world / nteams consecutive ranks, rotations dealt round-robin to teams
    if replicas or world == 1:
        nteams, B, team, owner = 1, 1, 0, True
        my_rots = list(range(max(1, min(args.concurrent, NROT)))) if world == 1 else list(range(NROT))
        beam_group = None
    else:
        nteams = min(world, NROT)
        if world % nteams:
            raise SystemExit('--gpus must be 1, 2, 4 or a multiple of the number of rotations')
        B = 1 if args.beam_shards == 'auto' else int(args.beam_shards)
        if B < 1 or world % B or world // B < nteams:
            raise SystemExit('--beam-shards must divide --gpus and leave at least one team per rotation')
        if B == 1:
            # one working rank per rotation; with more ranks than rotations the others idle (they take part in the barriers and in the
            # final gather only): sharding the beam inside a rotation loses against the library's beam walk of one rank
            team, owner = rank, rank < nteams
            my_rots = [r for r in range(NROT) if r % nteams == rank] if owner else []
            beam_group = None
        else:
            nteams = world // B
            team, owner = rank // B, rank % B == 0
            my_rots = [r for r in range(NROT) if r % nteams == team]
            beam_group = parallel._beam_groups(world, B)[team]
    sweeps_per_step = len(my_rots) * (world if replicas else 1) if (replicas or world == 1) else NROT
    solvers = [make(r) for r in my_rots] if owner else []
    solver = solvers[0] if solvers else None

    def step():
        if owner:
            parallel.run_concurrent([(lambda s=s: s._setup_rhoT(**kw)) for s in solvers])
        if beam_group is not None or (args.force_dist and world == 1):
            # the boundary MPS of every row to the beam partners (RCCL broadcast; rehearsed on a group of one with --force-dist)
            for s in (solvers if owner else [None] * len(my_rots)):
                parallel.broadcast_site_tensors([m.A for m in s.rhoT] if owner else None, beam_group, rehearse=world == 1)

    # Untimed phase.  (1) one single-chain sweep without any instrumentation (latency of one chain), (2) the same with
    # events on every kernel family (per-family / per-phase tables), (3) the W warm-up steps.  The timed steps then
    # bracket only the dominant family's launches with events, so the roofline duration is measured inside the timed
    # region at small overhead.
    warm_prof, single_ms, single_prof_ms, phases, panel_stats, chain_info, census = None, None, None, None, None, None, None
    mask_all = (1 << len(FAMILIES)) - 1
    if owner and rank == 0 and not args.no_profile and args.warmup > 0:
        torch.cuda.synchronize()
        from tnac4o_amd import ops as _ops
        _ops.panel_stats(reset=True)
        t0 = time.perf_counter()
        solver._setup_rhoT(**kw)
        torch.cuda.synchronize()
        single_ms = 1e3 * (time.perf_counter() - t0)
        panel_stats = _ops.panel_stats()
        panel_stats['what'] = 'iterated Cholesky-QR panel step (csrc/cholqr.hip) over the un-instrumented single-chain sweep'
        lib.tn_profile_reset()
        lib.tn_profile_enable(mask_all)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver._setup_rhoT(**kw)
        torch.cuda.synchronize()
        single_prof_ms = 1e3 * (time.perf_counter() - t0)
        warm_prof = profile_totals(lib)
        phases = phase_report(lib, pmc)
        lib.tn_profile_enable(0)
        # what the chain driver did on rotation 0 (tn_compress_mps info, summed over the rows of that sweep)
        infos = [m.native_info for m in solver.rhoT if m is not None and getattr(m, 'native_info', None)]
        chain_info = {'rows': len(infos),
                      'plain_pass_fallbacks_per_sweep': sum(i['reveal_fallbacks'] for i in infos),
                      'reveal_error_bound_max': max([i['reveal_error_bound'] for i in infos] or [0.0]),
                      'reveal_error_bound_limit': 2.0 ** -56,
                      'redone_rows_after_barrier_timeouts': sum(i.get('redone', 0) for i in infos),
                      'bonds_without_decomposition_in_intermediate_passes': sum(i.get('gauge_skipped', 0) for i in infos),
                      'rows_with_the_4chi_pass_as_variational_target': sum(i.get('target_swapped', 0) for i in infos),
                      'rows_without_the_4chi_stage_sweep': sum(i.get('var1_skipped', 0) for i in infos),
                      'sites_absorbed_inside_the_attach': sum(i.get('attach_fused', 0) for i in infos),
                      'what': 'rotation 0, one sweep: fallbacks of the weighted first pass to the plain one (the big plain tn_qr shape), its '
                              'a-posteriori bound, and how often the shortcuts of the intermediate stages applied (csrc/chain.hip)'}
        # launch census of the OTHER rotations (the timed step averages all four; their launch mix differs): one instrumented single-chain
        # sweep each, same events-on-every-launch form as the rotation-0 tables
        census = {'0': {'launches': sum(p['calls'] for p in warm_prof), 'kernel_ms': round(sum(p['ms'] for p in warm_prof), 1),
                        'jacobi_round_launches': warm_prof[7]['calls'], 'panel_step_launches': warm_prof[10]['calls']}}
        if world == 1 and len(solvers) > 1:
            for r_i, s_i in enumerate(solvers[1:], start=1):
                lib.tn_profile_reset()
                lib.tn_profile_enable(mask_all)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s_i._setup_rhoT(**kw)
                torch.cuda.synchronize()
                ms_i = 1e3 * (time.perf_counter() - t0)
                t_i = profile_totals(lib)
                lib.tn_profile_enable(0)
                census[str(my_rots[r_i])] = {'launches': sum(p['calls'] for p in t_i), 'kernel_ms': round(sum(p['ms'] for p in t_i), 1),
                                             'jacobi_round_launches': t_i[7]['calls'], 'panel_step_launches': t_i[10]['calls'],
                                             'single_chain_sweep_with_events_ms': round(ms_i, 1)}
    for _ in range(args.warmup):
        step()
    if not args.no_profile:
        dom_mask = mask_all if warm_prof is None else 1 << max(range(len(warm_prof)), key=lambda i: warm_prof[i]['ms'])
        if dist is not None and world > 1:          # every rank samples the family rank 0 found dominant
            t = torch.tensor([dom_mask], dtype=torch.int64, device=parallel._comm_device(None))
            dist.broadcast(t, src=0)
            dom_mask = int(t.item())
        lib.tn_profile_reset()
        lib.tn_profile_sample(max(1, args.sample))
        lib.tn_profile_enable(dom_mask)
        from tnac4o_amd import ops as _ops
        _ops.panel_stats(reset=True)            # the passes the panel chain really applies during the timed steps (device counters)
    step_ms = []
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ts = time.perf_counter()
        step()
        torch.cuda.synchronize()
        step_ms.append(1e3 * (time.perf_counter() - ts))
    barrier()
    dt = time.perf_counter() - t0
    prof, timed_panel = None, None
    if not args.no_profile:
        prof = profile_totals(lib)
        lib.tn_profile_enable(0)
        lib.tn_profile_sample(1)
        timed_panel = _ops.panel_stats()
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=parallel._comm_device(None))
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = 1e3 * dt / args.steps
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, solvers, my_rots)

    # second headline, outside the timed region: one full ground-state search of the 4 rotations
    # (sweeps + beam M=1024, merge of the rotations; with N > 1 sharded exactly like the timed step, one RCCL all-gather)
    full = None
    if not args.no_search:
        M = 1024 if kind == 'Ising' else 64
        skw = dict(M=M, relative_P_cutoff=1e-8, Dmax=chi)
        barrier()
        t0s = time.perf_counter()
        if world == 1 or replicas:
            res = parallel.solve_rotations(make, rotations=tuple(my_rots), concurrent=True, **skw) if rank == 0 else None
        else:
            res = parallel.solve_rotations(make, rotations=tuple(range(NROT)), concurrent=(B == 1), beam_shards=B, **skw)
        barrier()
        if res is not None:
            full = {'ms': 1e3 * (time.perf_counter() - t0s), 'rotations': len(res['records']), 'M': M,
                    'energy': res['energy'], 'degeneracy': res['degeneracy'], 'log2_probability': res['probability'],
                    'best_rotation': res['rotation'],
                    'what': 'solve_rotations: %d rotation(s), sweeps + beam search + merge%s' %
                            (len(res['records']), '' if world == 1 else ', one RCCL all-gather of the records')}

    if rank == 0:
        par = ('1 GPU: %d lattice rotations of one instance interleaved on %d HIP streams' % (len(my_rots), len(my_rots))) \
            if world == 1 else \
            ('%d ranks, every rank its own instance with 4 interleaved rotations, no collective' % world) if replicas else \
            ('%d ranks = %d rotation teams x %d rank(s): each team owner sweeps %d rotation(s)%s' %
             (world, nteams, B, len(my_rots), ', boundary MPS broadcast to its beam partner(s) over RCCL in the timed step'
              if B > 1 else (', %d rank(s) idle (more GPUs than rotations; --beam-shards 2 shards the beam instead)' % (world - nteams)
                             if world > nteams else '')))
        out = {
            'metric': 'PEPS-contraction ms/sweep, %s chi=%d (boundary-MPS sweep _setup_rhoT)' % (
                'chimera L=%d' % (n * n * 8) if kind == 'Ising' else 'RMF %dx%d d=8' % (n, n), chi),
            'value': ms_per_step / sweeps_per_step, 'unit': 'ms/sweep', 'n_gpus': world, 'steps': args.steps,
            'warmup': args.warmup, 'ms_per_step': ms_per_step, 'higher_is_better': False,
            'scaling': 'weak' if replicas else 'strong', 'vs_baseline': None, 'dtype': 'f64', 'data': 'synthetic',
            'config': {'workload': '%s, synthetic couplings seed %d, beta=%g, chi=%d; one sweep = %d rows of MPO absorb + '
                                   'compress_mps; one step = the sweeps of the %d lattice rotations of one instance' % (
                                       ('chimera L=%d (Nx=Ny=%d, Nc=8)' % (n * n * 8, n)) if kind == 'Ising' else
                                       ('Random Markov Field %d x %d, d=8' % (n, n)), seed, beta, chi, n, sweeps_per_step),
                       'sweeps_per_step': sweeps_per_step, 'parallelism': par, 'mode': args.mode,
                       'median_ms_per_sweep': statistics.median(step_ms) / sweeps_per_step,
                       'step_ms_rank0': [round(x, 1) for x in step_ms],
                       'single_chain_sweep_latency_ms': single_ms,
                       'single_chain_sweep_latency_with_events_on_every_launch_ms': single_prof_ms},
        }
        if single_ms:
            # a sweep is one sequential chain; a GPU interleaves c chains at (1 + f (c - 1)) x the latency of one, f
            # measured here when 4 chains ran (else the round-3 figure 0.11); more GPUs than rotations add nothing to the sweep step
            t1 = single_ms
            f = ((ms_per_step / t1 - 1.0) / 3.0) if (world == 1 and len(my_rots) == 4) else 0.11
            model = {}
            for N in (1, 2, 4, 8):
                c = max(1, 4 // min(N, 4))
                model[str(N)] = {'chains_per_gpu': c, 'expected_step_ms': t1 * (1.0 + f * (c - 1)), 'expected_value_ms_per_sweep': t1 * (1.0 + f * (c - 1)) / 4.0}
            for N in model:
                model[N]['expected_speedup_vs_1'] = model['1']['expected_step_ms'] / model[N]['expected_step_ms']
            out['scaling_model'] = {'single_chain_latency_ms': t1, 'cost_of_an_added_chain_frac': f, 'by_gpus': model,
                                    'note': 'strong scaling of ONE instance over its 4 lattice rotations (north-star decomposition): bounded by the latency '
                                            'of one chain; N = 8 keeps 4 working ranks (beam sharding inside a rotation does not pay at M = 1024)'}
        if solver is not None and getattr(solver, 'rhoT', None):
            out['config'].update({'rhoT_discarded_max': float(max(solver.rhoT_discarded)),
                                  'rhoT_overlap_min': float(min(solver.rhoT_overlap)),
                                  'bond_dims_mid_row': [int(d) for d in solver.rhoT[n // 2].D]})
        if prof is not None:
            dom = max(range(len(prof)), key=lambda i: prof[i]['ms'])
            d = dict(prof[dom])
            avg_ms = d['ms'] / max(1, d['calls'])
            executed = None
            if dom == 10 and timed_panel is not None:
                # The launches book what is known when they are enqueued (Gram, reflector products, the single-launch form's
                # panel in / reflectors out); the substitution passes are data dependent, so the work they REALLY did comes from the
                # device counters: 3 b flops per panel element and pass; 16 bytes per element and pass for the six-launch chain
                # (read + write of the panel), none for the single-launch form (the tile stays in LDS).  A launch that finds its
                # panel converged books nothing.  Counters cover every launch of the timed steps, the events every n-th: scale.
                frac_sampled = 1.0 / max(1, args.sample)
                pe6, pe1 = timed_panel['pass_elements_six_launch_chain'], timed_panel['pass_elements_single_launch']
                d['flops'] += 3.0 * 32 * (pe6 + pe1) * frac_sampled
                d['bytes'] += 16.0 * pe6 * frac_sampled
                executed = {'panels': timed_panel['panels'], 'single_launch_panels': timed_panel['single_launch_panels'],
                            'substitution_passes_applied': timed_panel['substitution_passes'],
                            'pass_elements_six_launch_chain': pe6, 'pass_elements_single_launch': pe1,
                            'note': 'bytes / flops of the substitution passes are booked from these device counters (executed work), not per launch'}
            if dom in MFMA_FAM:
                ach = d['flops'] / (d['ms'] * 1e-3) / 1e12 if d['ms'] > 0 else 0.0
                roof = {'bound': 'mfma', 'achieved': ach, 'peak': PEAK_F64_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                        'frac': ach / PEAK_F64_MFMA_TFLOPS}
            else:
                ach = d['bytes'] / (d['ms'] * 1e-3) / 1e9 if d['ms'] > 0 else 0.0
                roof = {'bound': 'hbm', 'achieved': ach, 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': ach / PEAK_HBM_GBS}
            if executed is not None:
                roof['executed_work'] = executed
            roof.update({'traffic': None, 'kernel': d['kernel'], 'launches_timed': d['calls'],
                         'launch_sampling': 'every %d-th launch of this family bracketed by HIP events on its stream, inside '
                                            'the timed region' % max(1, args.sample),
                         'avg_launch_ms': avg_ms,
                         'algorithmic_flops_per_launch': d['flops'] / max(1, d['calls']),
                         'algorithmic_bytes_per_launch': d['bytes'] / max(1, d['calls'])})
            if dom in SERIAL_FAM:
                _, what, nser = SERIAL_FAM[dom]
                if nser is None:             # rounds per launch are data dependent: library counter over the SAME timed region
                    rounds = _get(lib, -1, COUNTERS['svd_rounds'])
                    nsw_timed = max(1, args.steps * len(my_rots))
                    rounds_per_sweep = rounds['calls'] / nsw_timed
                    launches_per_sweep = d['calls'] * max(1, args.sample) / nsw_timed        # sampled launches x sampling interval
                    nser = max(1.0, rounds_per_sweep / max(1.0, launches_per_sweep))
                    roof['rounds_per_launch'] = nser
                    roof['rounds_per_sweep'] = rounds_per_sweep
                    roof['launches_per_sweep_timed_region'] = launches_per_sweep
                roof['us_per_serial_step'] = 1e3 * avg_ms / nser
                roof['serial_step'] = '%s, %.1f per launch' % (what, nser)
            fam = None
            if pmc:
                for key in (d['kernel'],) + PMC_ALIASES.get(dom, ()):
                    fam = pmc.get('families', {}).get(key) or fam
            if fam:
                roof['traffic'] = fam['traffic_bytes_per_launch']
                roof['traffic_shape'] = fam.get('probe_shape', 'tn_qr 16384 x 1024 (tools/pmc_probe.py): per-launch mean of the probe, NOT of '
                                                'the workload mix -- compare it with algorithmic_bytes_per_launch_same_probe below, not with '
                                                'algorithmic_bytes_per_launch above')
                roof['traffic_detail'] = {
                    'unit': 'bytes per launch', 'source': '%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, '
                    'FETCH_SIZE x2 per the gfx950 correction) on tools/pmc_probe.py: the same kernels at the bulk shapes of '
                    'this workload (tn_qr 16384 x 1024, tn_svd_trunc 1024 x 1024)' % pmc['file'],
                    'fetch': fam['fetch_bytes_per_launch'], 'write': fam['write_bytes_per_launch'],
                    'algorithmic_bytes_per_launch_same_probe': fam.get('algorithmic_bytes_per_launch'),
                    'traffic_over_algorithmic': fam.get('traffic_over_algorithmic')}
            if dom in SERIAL_FAM:
                ratio = (fam or {}).get('traffic_over_algorithmic')
                roof['limited_by'] = ('latency: serial steps of single workgroups and dependent memory round trips, not bytes (measured HBM traffic of '
                                      'this family on the probe: %s its algorithmic bytes); figure of merit = time per serial step' %
                                      ('%.2fx' % ratio if ratio else 'not collected for'))
            out['roofline'] = roof
            table = warm_prof if warm_prof is not None else prof
            nsw = 1 if warm_prof is not None else args.steps * len(my_rots)
            out['kernel_table_source'] = ('ROTATION 0 alone: one single-chain sweep before the timed region with events on every launch '
                                          '(kernel_time_ms_per_sweep, kernel_launches_per_sweep, launches_per_sweep, the phase table, gemm_mfma); '
                                          'the other rotations: launch_census_by_rotation' if warm_prof is not None else 'timed sweeps')
            out['kernel_time_ms_per_sweep'] = {p['kernel']: round(p['ms'] / nsw, 3) for p in table}
            out['kernel_launches_per_sweep'] = {p['kernel']: p['calls'] // nsw for p in table}
            out['launches_per_sweep'] = sum(p['calls'] for p in table) // nsw
            if phases is not None:
                out['phase_kernel_time_single_chain_sweep'] = phases
            gm = [p for i, p in enumerate(table) if i in MFMA_FAM and p['ms'] > 0]
            if gm:
                fl, ms = sum(p['flops'] for p in gm), sum(p['ms'] for p in gm)
                out['gemm_mfma'] = {'achieved': fl / (ms * 1e-3) / 1e12, 'peak': PEAK_F64_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                                    'frac': fl / (ms * 1e-3) / 1e12 / PEAK_F64_MFMA_TFLOPS, 'ms_per_sweep': ms / nsw}
                if warm_prof is not None:
                    t_sw = ms_per_step / sweeps_per_step * 1e-3
                    out['sweep_mfma'] = {
                        'executed_mfma_gemm_flops_per_sweep': fl, 'unit': 'TFLOP/s', 'peak': PEAK_F64_MFMA_TFLOPS,
                        'achieved_at_step_rate': fl / t_sw / 1e12, 'frac_at_step_rate': fl / t_sw / 1e12 / PEAK_F64_MFMA_TFLOPS,
                        'frac_single_chain': (fl / (single_ms * 1e-3) / 1e12 / PEAK_F64_MFMA_TFLOPS) if single_ms else None,
                        'note': 'all MFMA GEMM flops a sweep executes / wall time of a sweep; SQ MFMA counters: ' +
                                ((pmc or {}).get('mfma_counters', {}).get('file', 'not collected'))}
            ab = table[5]
            if ab['ms'] > 0:
                out['absorb_hbm'] = {'achieved': ab['bytes'] / (ab['ms'] * 1e-3) / 1e9, 'peak': PEAK_HBM_GBS, 'unit': 'GB/s',
                                     'frac': ab['bytes'] / (ab['ms'] * 1e-3) / 1e9 / PEAK_HBM_GBS, 'launches_per_sweep': ab['calls'] // nsw,
                                     'what': 'absorb_mfma_kernel over the sites that are still materialised -- since round 5 the edge sites only (small '
                                             'tensors): the absorption of a bulk site rides on the attach products of the first pass and its 134 MB tensor '
                                             'is never formed (DESIGN.md 4.7); the kernel at the bulk shape moves 4.35 TB/s (PMC probe, 1.04x algorithmic)'}
        if panel_stats is not None:
            out['panel_step'] = panel_stats
        if chain_info is not None:
            out['chain_driver'] = chain_info
        if census is not None:
            out['launch_census_by_rotation'] = census
        if full is not None:
            out['full_solve'] = full
        if args.cpu_rows > 0 and world == 1 and kind == 'Ising' and solver is not None:
            out['cpu_baseline'] = cpu_baseline(n, args, solver, kw, single_ms)
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def physical_cores():
    """Physical cores of the box (sockets x cores per socket from /proc/cpuinfo; logical count as a fallback)."""
    try:
        phys = {}
        pid = cid = None
        with open('/proc/cpuinfo') as f:
            for line in f:
                if line.startswith('physical id'):
                    pid = line.split(':')[1].strip()
                elif line.startswith('core id'):
                    cid = line.split(':')[1].strip()
                elif not line.strip():
                    if pid is not None and cid is not None:
                        phys[(pid, cid)] = 1
                    pid = cid = None
        if phys:
            return len(phys)
    except OSError:
        pass
    return os.cpu_count() or 1


def cpu_baseline(n, args, solver, kw, single_ms):
    """CPU oracle ("port" of the reference algorithm: oracle/ = numpy/scipy on OpenBLAS restating tnac4o.py:1688-1693 / mps.py:175-200)
    on a bounded sample of the SAME sweep: `cpu_rows` WHOLE bulk rows -- MPS.apply_mpo + MPS.compress_mps with the defaults of
    search_ground_state, each from the boundary MPS the GPU sweep fed into that row -- timed with the fastest of the
    BLAS thread counts {1, 8, 16, 32, 64, physical cores} as found on a proxy (the 4096 x 1024 QR + attach GEMM of a bulk site: what
    the reference spends 87 % of a row on).  The product path runs the same rows on the GPU from the same inputs (`gpu_ms_per_row`);
    the fidelity of the two compressed states is asserted (>= 1 - 1e-12) per row.  `value` = CPU time per row; the full-sweep figure
    multiplies by the number of rows (edge rows are cheaper: an upper bound, stated).  The first-pass sample of the earlier rounds
    (plain first canonisation pass over 8 sites of one row) is kept as the sub-field `first_pass_sample`."""
    from oracle import mps_ref as mr
    from tnac4o_amd import mps
    try:
        import threadpoolctl
    except ImportError:
        threadpoolctl = None
    phys, logical = physical_cores(), os.cpu_count() or 1
    # OpenBLAS cannot grow its thread pool beyond the size it started with (OMP_NUM_THREADS / OPENBLAS_NUM_THREADS, else the CPU
    # count): a higher limit crashes it in its worker threads.  That start-up size bounds every thread count tried below.
    usable = logical
    if threadpoolctl is not None:
        usable = min([p['num_threads'] for p in threadpoolctl.threadpool_info() if p.get('user_api') == 'blas'] or [logical])

    def limited(nt, fn):
        if threadpoolctl is None:
            return fn()
        with threadpoolctl.threadpool_limits(limits=nt):
            return fn()

    # ---- thread count: proxy = one bulk-site step of the reference's first pass (attach GEMM 4096 x 1024 x 1024 + QR of 4096 x 1024)
    rng = np.random.default_rng(1)
    Tp = rng.standard_normal((4096, 1024))
    Cp = rng.standard_normal((1024, 1024))

    def proxy():
        t0 = time.perf_counter()
        mr.qr_pos(Tp @ Cp)
        return 1e3 * (time.perf_counter() - t0)
    counts = [1] if threadpoolctl is None else sorted({c for c in (1, 8, 16, 32, 64, phys, usable) if c <= usable})
    proxy_ms = {}
    for nt in counts:
        limited(nt, proxy)                                 # (first touch: thread pool start-up)
        proxy_ms[str(nt)] = min(limited(nt, proxy) for _ in range(2))
    threads = int(min(proxy_ms, key=proxy_ms.get))

    # ---- whole bulk rows.  The thread count that enters `value` is chosen on a REAL row (the first one, timed at 8 / 16 / 32 BLAS threads
    # plus the proxy's winner): the rows are dominated by 16384 x 1024 factorisations, the proxy is a quarter of that
    kwc = dict(Dmax=kw['Dmax'], tolS=1e-16, tolV=1e-10, max_sweeps=20, graduate_truncation=True)
    rows = [n // 2 - i for i in range(max(1, args.cpu_rows))]
    per_row = []
    row_ms_by_threads = {}
    cand = [threads] if threadpoolctl is None else sorted({c for c in (8, 16, 32, threads) if c <= usable})
    for ny in rows:
        psi = solver.rhoT[ny + 1]
        mpo = solver._row_mpo(ny)
        inp = [a.cpu().numpy() for a in psi.A]
        Ws = [w.cpu().numpy() for w in mpo.W]

        def cpu_row():
            o = mr.RefMPS(d=[a.shape[1] for a in inp], L=n, Dmax=1, canonise=None)
            o.A = [np.array(a) for a in inp]
            o.D = [inp[0].shape[0]] + [a.shape[2] for a in inp]
            M = mr.RefMPO(n)
            for i, W in enumerate(Ws):
                M.set_direct(np.array(W), i)
            t0 = time.perf_counter()
            o.apply_mpo(M, Hconj=True)
            ov = o.compress_mps(**kwc)
            return 1e3 * (time.perf_counter() - t0), o, ov
        if not row_ms_by_threads and len(cand) > 1:
            best = None
            for nt in cand:
                r_ = limited(nt, cpu_row)
                row_ms_by_threads[str(nt)] = r_[0]
                if best is None or r_[0] < best[0][0]:
                    best = (r_, nt)
            (cpu_ms, o, ov_ref), threads = best
        else:
            cpu_ms, o, ov_ref = limited(threads, cpu_row)
        out = psi.copy()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ov = out.apply_mpo_compress(mpo, Hconj=True, **kwc)
        torch.cuda.synchronize()
        gpu_ms = 1e3 * (time.perf_counter() - t0)
        got = mr.RefMPS(d=[a.shape[1] for a in out.A], L=n, Dmax=1, canonise=None)
        got.A = [a.cpu().numpy() for a in out.A]
        fid = abs(mr.mps_dot(got, o)) / np.sqrt(mr.mps_dot(got, got) * mr.mps_dot(o, o))
        assert 1.0 - fid < 1e-12, 'cpu_baseline: GPU and CPU oracle disagree on row %d (1 - fidelity = %.2e)' % (ny, 1.0 - fid)
        per_row.append({'row': ny, 'cpu_ms': cpu_ms, 'gpu_ms': gpu_ms, 'one_minus_fidelity': float(1.0 - fid), 'overlap_cpu': float(ov_ref),
                        'overlap_gpu': float(ov), 'discarded_max_cpu': float(max(o.discarded)), 'discarded_max_gpu': float(max(out.discarded)),
                        'absorbed_bond_max': int(max(a.shape[0] for a in inp) * max(w.shape[0] for w in Ws))})
    cpu_row_ms = float(np.mean([r['cpu_ms'] for r in per_row]))
    gpu_row_ms = float(np.mean([r['gpu_ms'] for r in per_row]))

    # ---- the earlier rounds' sample, kept for continuity: plain first canonisation pass over the right edge + 4 bulk sites of the middle row
    first_pass = None
    try:
        ny = n // 2
        psi = solver.rhoT[ny + 1].copy()
        psi.apply_mpo(solver._row_mpo(ny), Hconj=True)
        sites = list(range(n - 1, n - 9, -1))
        host = {s_: psi.A[s_].cpu().numpy() for s_ in sites}

        def fp_run():
            o = mr.RefMPS(d=[int(a.shape[1]) for a in psi.A], L=n, Dmax=1, canonise=None)
            o.A = [host[s_].copy() if s_ in host else None for s_ in range(n)]
            o.D = list(psi.D)
            o.C, o.pC = np.ones((1, 1)), n
            t0 = time.perf_counter()
            for s_ in sites:
                o.attach_AC()
                o.orth_right(s_)
            return 1e3 * (time.perf_counter() - t0)
        first_pass = {'what': 'plain first canonisation pass (attach GEMM + QR + nfactor) over sites %d..%d of row %d' % (sites[0], sites[-1], ny),
                      'cpu_ms': limited(threads, fp_run), 'threads': threads}
    except Exception as e:                                 # noqa: BLE001 -- a sub-field must not take the bench line down
        first_pass = {'error': repr(e)}
    return {'value': cpu_row_ms, 'unit': 'ms per bulk row (apply_mpo + compress_mps)', 'cores': threads, 'kind': 'port', 'cpu_model': cpu_model(),
            'physical_cores': phys, 'logical_cores': logical, 'usable_blas_threads': usable, 'proxy_ms_by_blas_threads': proxy_ms, 'row_ms_by_blas_threads': row_ms_by_threads,
            'sample': 'whole bulk rows %s of the %d-row sweep (chi = %d): MPS.apply_mpo + MPS.compress_mps of the reference algorithm (oracle/, '
                      'numpy + scipy LAPACK) from the boundary MPS the GPU sweep fed into each row; %d BLAS threads = the fastest of %s on the first of '
                      'these rows (row_ms_by_blas_threads)' % (rows, n, kw['Dmax'], threads, sorted(int(k) for k in row_ms_by_threads) or [threads]),
            'rows': per_row, 'gpu_ms_per_row': gpu_row_ms, 'speedup_per_row': cpu_row_ms / gpu_row_ms if gpu_row_ms > 0 else None,
            'full_sweep_cpu_ms_extrapolation': cpu_row_ms * n,
            'extrapolation': 'CPU time per bulk row x %d rows (the two edge rows are cheaper: an upper bound by < 2 rows); no GPU figure enters it' % n,
            'first_pass_sample': first_pass}


if __name__ == '__main__':
    main()
