// Cell sweeps over given configurations (no counterpart in the reference): tn_cell_sweep moves M configurations by block updates of
// whole cells -- a heat bath at inverse temperature beta, or a quench to the conditional minimum -- under the energy the walks add up
// (walk.h: cell_energy).  No boundary MPS and no contraction: only the energy tables of the cells are read.
//
// The conditional energy of cell c in state s, given the states sl, su, sr, sb of its four neighbours (R, Bc: the right / lower cell):
//     e(s) = (((1.0 Es[s] + E1[s, L]) + E4[s, U]) + R.E1[sr, R.left_map(s)]) + Bc.E4[sb, Bc.up_map(s)]
// with these additions in this order (a term is absent at a lattice edge; nothing here can contract into an FMA).  Cells of one
// checkerboard colour (ny + nx even / odd) have no neighbour of their own colour, so one launch updates a whole colour in place from the
// states as they stand before it: a workgroup per (cell, tile of samples), no barrier across workgroups, no atomics.
//
// Inside a workgroup a GROUP of W lanes serves one sample at a time, state s on lane s % W of the group in chunk s / W; W (8, 32 or 64)
// and whether the energies stay in registers (q <= 256) or are evaluated again per pass (any q) depend on q alone:
//   minimum    lane-local over the chunks, then a butterfly over the group on (energy, state): the smallest state attaining it;
//   heat bath  w_s = exp(-beta (e(s) - min e)); running sum c_s = carry + (shuffle scan inside the chunk), carry += the chunk's total,
//              chunks in ascending order, W_tot = c_{q-1}; t = u W_tot; new state = the first s with c_s >= t and w_s > 0, otherwise the
//              last s with w_s > 0 (tn_sample_pn's rule);
//   quench     new state = the smallest s attaining min e if min e < e(current) strictly, otherwise the cell stays.
// A cell's tables (Es, and E1 / E4 transposed so that the lanes of a group read consecutive words) are staged in LDS when they fit
// TN_CELL_SWEEP_LDS bytes (default 32 KiB, at most 150 KiB, 0: never), otherwise they are read from global memory: the same values,
// the same bits.
// A state outside [0, q) of its cell is never used as an index: as a neighbour it is read as 0, as the current state of a quench its
// energy counts as +inf.
#include "walk.h"
#include "sweep.h"

#pragma clang fp contract(off)

namespace tn {

namespace {

constexpr int64_t SWEEP_LDS_BYTES = 150 * 1024;      // the most a cell's staged tables may take (tn_sample_pn's bound)
constexpr int64_t SWEEP_LDS_DEFAULT = 32 * 1024;    // ... and what they may take by default (TN_CELL_SWEEP_LDS)
constexpr int SWEEP_TILE = 256;                      // samples per workgroup = its threads (a result never depends on it)
constexpr int SWEEP_PUT = 40;                        // table entries one launch of put_cells_kernel carries in its arguments

struct SweepCellPack { SweepCell c[SWEEP_PUT]; };

// The table of the call travels in kernel arguments (copied when the launch is enqueued): no staging buffer has to outlive the call.
__global__ __launch_bounds__(64) void put_cells_kernel(SweepCellPack pack, int n, SweepCell* out) {
    const int i = threadIdx.x;
    if (i < n) out[i] = pack.c[i];
}

struct SweepArgs {
    const SweepCell* cells;
    int16_t* states;
    const double* uniforms;             // row 0 = cell 0 of this sweep
    uint8_t* chg;                       // [cell][sample]: 1 = the update changed the state (may be NULL)
    int64_t Nx, Ny, M, ldu, ntiles;
    int colour, mode;
    double beta;
    SweepBetas rb;                      // the per-row-beta instances only (tn_temper): beta of sample m = rb.betas[rb.tidx[m]]
};

__device__ __forceinline__ int in_cell(int s, int q) { return (s >= 0 && s < q) ? s : 0; }

// what a cell update reads of its sample, gathered for the whole tile at once (one thread per sample) so that the waves' loop over
// the samples starts from LDS: own state, columns of E1 / E4, states of the right / lower neighbour, the uniform number
struct SweepPrep {
    int cur[SWEEP_TILE], L[SWEEP_TILE], U[SWEEP_TILE], sr[SWEEP_TILE], sb[SWEEP_TILE];
    double u[SWEEP_TILE];
};

template <int W, int NJ, bool LDS, bool RB>
__device__ __forceinline__ void sweep_tile(const SweepArgs& a, const SweepCell& c, const SweepCell* R, const SweepCell* B, int64_t k, bool has_left,
                                           bool has_up, const double* tEs, const double* tE1, const double* tE4, const SweepPrep& p, const double* pbeta, int64_t m0, int64_t m1) {
    constexpr int G = 64 / W, NR = NJ > 0 ? NJ : 1;
    const int tid = threadIdx.x, lane = tid & 63, l = lane % W, g = (tid >> 6) * G + lane / W;
    const int q = c.q, nchunk = (q + W - 1) / W;
    const int64_t ncell = a.Nx * a.Ny;
    const int64_t e1s = LDS ? 1 : c.e1cols, e1l = LDS ? (q | 1) : 1, e4s = LDS ? 1 : c.e4cols, e4l = LDS ? (q | 1) : 1;
    const double inf = std::numeric_limits<double>::infinity();
    // what a lane reads of its own states is the same for every sample
    auto right_col = [&](int s) { return R ? (R->left_map ? (int)R->left_map[s] : s) : 0; };
    auto down_col = [&](int s) { return B ? (B->up_map ? (int)B->up_map[s] : s) : 0; };
    double esv[NR];
    int rmv[NR], dmv[NR];
    if constexpr (NJ > 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int s = j * W + l;
            esv[j] = 0.0; rmv[j] = 0; dmv[j] = 0;
            if (s < q) { esv[j] = tEs[s]; rmv[j] = right_col(s); dmv[j] = down_col(s); }
        }
    }
    const int per = 4 * G, nloc = (int)(m1 - m0), niter = (nloc + per - 1) / per;
    for (int it = 0; it < niter; ++it) {
        const int ii = it * per + g;
        const bool active = ii < nloc;
        const int i = active ? ii : nloc - 1;                    // an idle group repeats the tile's last sample and writes nothing
        const int64_t m = m0 + i;
        const int cur = p.cur[i];
        const int64_t L = p.L[i], U = p.U[i];
        const double* Rrow = R ? R->E1 + (int64_t)p.sr[i] * R->e1cols : nullptr;
        const double* Brow = B ? B->E4 + (int64_t)p.sb[i] * B->e4cols : nullptr;
        auto energy = [&](int s, double es, int rm, int dm) {
            double e = 1.0 * es;
            if (has_left) e = e + tE1[s * e1s + L * e1l];
            if (has_up) e = e + tE4[s * e4s + U * e4l];
            if (R) e = e + Rrow[rm];
            if (B) e = e + Brow[dm];
            return e;
        };
        auto energy_of = [&](int s) { return energy(s, tEs[s], right_col(s), down_col(s)); };
        // ---- minimum and the smallest state attaining it
        double ev[NR];
        double be = inf;
        int bs = 0x7fffffff;
        if constexpr (NJ > 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int s = j * W + l;
                ev[j] = inf;
                if (s < q) {
                    ev[j] = energy(s, esv[j], rmv[j], dmv[j]);
                    if (ev[j] < be || bs == 0x7fffffff) { be = ev[j]; bs = s; }
                }
            }
        } else {
            for (int j = 0; j < nchunk; ++j) {
                const int s = j * W + l;
                if (s < q) {
                    const double e = energy_of(s);
                    if (e < be || bs == 0x7fffffff) { be = e; bs = s; }
                }
            }
        }
#pragma unroll
        for (int o = W / 2; o >= 1; o >>= 1) {
            const double oe = __shfl_xor(be, o, W);
            const int os = __shfl_xor(bs, o, W);
            if (os != 0x7fffffff && (bs == 0x7fffffff || oe < be || (oe == be && os < bs))) { be = oe; bs = os; }
        }
        int news;
        if (a.mode == 1) {
            double ecur = inf;
            if constexpr (NJ > 0) {                              // the lane that holds the current state has its energy already
                const int cc = in_cell(cur, q);
                double v = ev[0];
#pragma unroll
                for (int j = 1; j < NJ; ++j) if (cc / W == j) v = ev[j];
                v = __shfl(v, cc % W, W);
                if (cur >= 0 && cur < q) ecur = v;
            } else {
                if (cur >= 0 && cur < q) ecur = energy_of(cur);
            }
            news = be < ecur ? bs : cur;
        } else {
            // ---- weights, their running sum in chunk order, the draw
            const double u = p.u[i];
            double wv[NR], cv[NR];
            double carry = 0.0;
            double beta = a.beta;
            if constexpr (RB) beta = pbeta[i];
            auto weight = [&](int s, double e) { return s < q ? exp(-beta * (e - be)) : 0.0; };
            auto scan = [&](double v) {                          // inclusive over the group, lane order
#pragma unroll
                for (int o = 1; o < W; o <<= 1) {
                    const double t = __shfl_up(v, o, W);
                    if (l >= o) v += t;
                }
                return v;
            };
            // first pass: W_tot (and, in registers, every c_s)
            if constexpr (NJ > 0) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    wv[j] = 0.0; cv[j] = 0.0;
                    if (j < nchunk) {
                        wv[j] = weight(j * W + l, ev[j]);
                        const double v = scan(wv[j]);
                        cv[j] = carry + v;
                        carry = carry + __shfl(v, W - 1, W);
                    }
                }
            } else {
                for (int j = 0; j < nchunk; ++j) {
                    const int s = j * W + l;
                    const double v = scan(weight(s, s < q ? energy_of(s) : 0.0));
                    carry = carry + __shfl(v, W - 1, W);
                }
            }
            const double t = u * carry;
            int first = 0x7fffffff, last = -1;
            if constexpr (NJ > 0) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int s = j * W + l;
                    if (s < q && wv[j] > 0.0) {
                        last = s;
                        if (cv[j] >= t && first == 0x7fffffff) first = s;
                    }
                }
            } else {
                double carry2 = 0.0;
                for (int j = 0; j < nchunk; ++j) {
                    const int s = j * W + l;
                    const double w = weight(s, s < q ? energy_of(s) : 0.0);
                    const double v = scan(w);
                    if (s < q && w > 0.0) {
                        last = s;
                        if (carry2 + v >= t && first == 0x7fffffff) first = s;
                    }
                    carry2 = carry2 + __shfl(v, W - 1, W);
                }
            }
#pragma unroll
            for (int o = W / 2; o >= 1; o >>= 1) {
                first = min(first, __shfl_xor(first, o, W));
                last = max(last, __shfl_xor(last, o, W));
            }
            news = first != 0x7fffffff ? first : last;
        }
        if (active && l == 0) {
            if (news != cur) a.states[m * ncell + k] = (int16_t)news;
            if (a.chg) a.chg[k * a.M + m] = news != cur ? 1 : 0;
        }
    }
}

// the class of a cell: how its states are laid over the lanes (a function of q alone).  One kernel per class, so that the small
// cells do not pay for the registers of the large ones; a workgroup whose cell belongs to another class returns at once.
__host__ __device__ inline int sweep_class(int64_t q) { return q <= 8 ? 0 : q <= 32 ? 1 : q <= 256 ? 2 : 3; }

// RB: every sample at its own beta (staged next to what SweepPrep holds); the body of the move is the one above
template <int CLS, bool RB>
__global__ __launch_bounds__(256) void cell_sweep_kernel(SweepArgs a) {
    extern __shared__ double lds[];
    const int64_t slot = blockIdx.x / a.ntiles, tile = blockIdx.x % a.ntiles;
    const int64_t half = (a.Nx + 1) / 2, ny = slot / half, nx = 2 * (slot % half) + ((ny + a.colour) & 1);
    if (nx >= a.Nx) return;
    const int64_t k = ny * a.Nx + nx;
    const SweepCell c = a.cells[k];
    if (sweep_class(c.q) != CLS) return;
    const bool has_left = nx > 0, has_up = ny > 0;
    const SweepCell* R = nx + 1 < a.Nx ? a.cells + k + 1 : nullptr;
    const SweepCell* B = ny + 1 < a.Ny ? a.cells + k + a.Nx : nullptr;
    const int64_t m0 = tile * SWEEP_TILE, m1 = m0 + SWEEP_TILE < a.M ? m0 + SWEEP_TILE : a.M;
    const int q = c.q;
    const double* tEs = c.Es;
    const double* tE1 = c.E1;
    const double* tE4 = c.E4;
    __shared__ SweepPrep prep;
    const double* pbeta = nullptr;
    if constexpr (RB) {
        __shared__ double sbeta[SWEEP_TILE];
        if ((int64_t)threadIdx.x < m1 - m0) {
            const int64_t t = a.rb.tidx[m0 + threadIdx.x];
            sbeta[threadIdx.x] = a.rb.betas[t >= 0 && t < a.rb.T ? t : 0];
        }
        pbeta = sbeta;
    }
    if ((int64_t)threadIdx.x < m1 - m0) {
        const int i = threadIdx.x;
        const int64_t m = m0 + i;
        const int16_t* row = a.states + m * a.Nx * a.Ny;
        int L = 0, U = 0;
        if (has_left) { const int sl = in_cell(row[k - 1], a.cells[k - 1].q); L = c.left_map ? (int)c.left_map[sl] : sl; }
        if (has_up) { const int su = in_cell(row[k - a.Nx], a.cells[k - a.Nx].q); U = c.up_map ? (int)c.up_map[su] : su; }
        prep.cur[i] = row[k]; prep.L[i] = L; prep.U[i] = U;
        prep.sr[i] = R ? in_cell(row[k + 1], R->q) : 0;
        prep.sb[i] = B ? in_cell(row[k + a.Nx], B->q) : 0;
        prep.u[i] = a.mode == 0 ? a.uniforms[k * a.ldu + m] : 0.0;
    }
    if (c.staged) {                                              // (uniform over the workgroup)
        const int64_t ldq = q | 1;
        double* sEs = lds;
        double* sE1 = sEs + q;
        double* sE4 = sE1 + (has_left ? c.e1cols * ldq : 0);
        for (int i = threadIdx.x; i < q; i += 256) sEs[i] = c.Es[i];
        if (has_left)
            for (int64_t i = threadIdx.x; i < (int64_t)q * c.e1cols; i += 256) sE1[(i % c.e1cols) * ldq + i / c.e1cols] = c.E1[i];
        if (has_up)
            for (int64_t i = threadIdx.x; i < (int64_t)q * c.e4cols; i += 256) sE4[(i % c.e4cols) * ldq + i / c.e4cols] = c.E4[i];
        tEs = sEs; tE1 = sE1; tE4 = sE4;
    }
    __syncthreads();
#define SWEEP_RUN(W, NJ)                                                                             \
    do {                                                                                             \
        if (c.staged) sweep_tile<W, NJ, true, RB>(a, c, R, B, k, has_left, has_up, tEs, tE1, tE4, prep, pbeta, m0, m1);  \
        else sweep_tile<W, NJ, false, RB>(a, c, R, B, k, has_left, has_up, tEs, tE1, tE4, prep, pbeta, m0, m1);        \
    } while (0)
    if constexpr (CLS == 0) SWEEP_RUN(8, 1);
    else if constexpr (CLS == 1) SWEEP_RUN(32, 1);
    else if constexpr (CLS == 2) SWEEP_RUN(64, 4);
    else SWEEP_RUN(64, 0);
#undef SWEEP_RUN
}

template <int CLS, bool RB>
int launch_sweep(hipStream_t st, const SweepArgs& a, int64_t nblocks, int64_t lds) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)cell_sweep_kernel<CLS, RB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL((cell_sweep_kernel<CLS, RB>), dim3((unsigned)nblocks), dim3(256), (size_t)lds, st, a));
    TN_CHECK_LAUNCH("cell_sweep_kernel");
    return 0;
}

// moves of one sweep from the flags of its two launches: last[m] = their number, moves[m] = (first sweep ? 0 : moves[m]) + it
__global__ __launch_bounds__(256) void sweep_moves_kernel(const uint8_t* chg, int64_t ncell, int64_t M, int first, int32_t* moves, int32_t* last) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    int32_t n = 0;
    for (int64_t k = 0; k < ncell; ++k) n += chg[k * M + m];
    if (moves) moves[m] = (first ? 0 : moves[m]) + n;
    if (last) last[m] = n;
}

// energy of every configuration: cell by cell in walk order through cell_energy (walk.h), the additions of the walks' energy_out.  The
// states a cell's term reads pass through a three-entry window (up, left, own) so that one outside its cell is read as 0.
__global__ __launch_bounds__(256) void sweep_energy_kernel(const SweepCell* cells, const int16_t* states, int64_t Nx, int64_t Ny, int64_t M, double* energy) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const int16_t* row = states + m * Nx * Ny;
    double E = 0.0;
    for (int64_t ny = 0; ny < Ny; ++ny)
        for (int64_t nx = 0; nx < Nx; ++nx) {
            const int64_t k = ny * Nx + nx;
            const SweepCell& c = cells[k];
            CellDev cd;
            cd.down = nullptr; cd.right = nullptr; cd.Es = c.Es; cd.E1 = c.E1; cd.E4 = c.E4; cd.left_map = c.left_map; cd.up_map = c.up_map;
            cd.q = c.q; cd.e1cols = c.e1cols; cd.e4cols = c.e4cols;
            int16_t win[3];
            win[0] = ny > 0 ? (int16_t)in_cell(row[k - Nx], cells[k - Nx].q) : 0;
            win[1] = nx > 0 ? (int16_t)in_cell(row[k - 1], cells[k - 1].q) : 0;
            win[2] = (int16_t)in_cell(row[k], c.q);
            E = E + cell_energy(cd, win[2], win, 2, 2, nx > 0 ? 1 : 0, ny > 0 ? 1 : 0);
        }
    energy[m] = E;
}

// the workspace of tn_cell_sweep: the table of the cells, the flags of a sweep
struct SweepWs {
    SweepCell* cells;
    uint8_t* chg;
    int64_t bytes;
};
SweepWs sweep_layout(void* ws, int64_t Nx, int64_t Ny, int64_t M) {
    WsCarve w{(char*)ws};
    SweepWs s;
    s.cells = w.take<SweepCell>(Nx * Ny * (int64_t)sizeof(SweepCell));
    s.chg = w.take<uint8_t>(Nx * Ny * M);
    s.bytes = w.total();
    return s;
}

// largest tables (bytes) that are staged; read per call: the tests switch it.  The default keeps four workgroups on a compute unit,
// which measured faster for the heat bath of 256-state cells than staging their 66 KiB at two workgroups per unit
int64_t sweep_lds_limit() { return std::min(std::max<int64_t>(env_i64("TN_CELL_SWEEP_LDS", SWEEP_LDS_DEFAULT), 0), SWEEP_LDS_BYTES); }

}  // namespace

// ---- what tn_temper shares (sweep.h) ---------------------------------------------------------------------------------------------
#define SWEEP_CHECK(cond, msg)                      \
    do {                                            \
        if (!(cond)) {                              \
            set_error("%s: %s", who, msg);          \
            return -1;                              \
        }                                           \
    } while (0)

int64_t sweep_cells_bytes(int64_t Nx, int64_t Ny) { return Nx * Ny * (int64_t)sizeof(SweepCell); }

int sweep_plan(const char* who, int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, SweepPlan& plan) {
    const int64_t ncell = Nx * Ny;
    const int64_t lds_limit = sweep_lds_limit();
    plan.Nx = Nx; plan.Ny = Ny; plan.M = M;
    plan.tab.assign((size_t)ncell, SweepCell{});
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 4; ++k) { plan.lds_bytes[c][k] = 0; plan.present[c][k] = false; }   // per colour and class of cells
    for (int64_t k = 0; k < ncell; ++k) {
        const tn_beam_cell& c = cells[k];
        const int64_t ny = k / Nx, nx = k % Nx;
        SWEEP_CHECK(c.q >= 1 && c.q <= 32767 && c.Es, "cells: q outside 1 .. 32767, or Es null");
        SWEEP_CHECK(nx == 0 || (c.E1 && c.e1cols >= 1 && c.e1cols < ((int64_t)1 << 31)), "cells: E1 null or e1cols out of range right of column 0");
        SWEEP_CHECK(ny == 0 || (c.E4 && c.e4cols >= 1 && c.e4cols < ((int64_t)1 << 31)), "cells: E4 null or e4cols out of range below row 0");
        SweepCell& t = plan.tab[(size_t)k];
        t.Es = c.Es; t.E1 = nx > 0 ? c.E1 : nullptr; t.E4 = ny > 0 ? c.E4 : nullptr;
        t.left_map = nx > 0 ? c.left_map : nullptr; t.up_map = ny > 0 ? c.up_map : nullptr;
        t.q = (int32_t)c.q; t.e1cols = nx > 0 ? (int32_t)c.e1cols : 1; t.e4cols = ny > 0 ? (int32_t)c.e4cols : 1;
        const int64_t ldq = c.q | 1;
        const int64_t bytes = (c.q + (nx > 0 ? c.e1cols * ldq : 0) + (ny > 0 ? c.e4cols * ldq : 0)) * 8;
        t.staged = bytes <= lds_limit ? 1 : 0;
        const int colour = (int)((ny + nx) & 1), cls = sweep_class(c.q);
        plan.present[colour][cls] = true;
        if (t.staged) plan.lds_bytes[colour][cls] = std::max(plan.lds_bytes[colour][cls], bytes);
    }
    plan.ntiles = cdiv(M, SWEEP_TILE);
    const int64_t slots = Ny * ((Nx + 1) / 2);
    plan.nblocks = 0;
    SWEEP_CHECK(!__builtin_mul_overflow(slots, plan.ntiles, &plan.nblocks) && plan.nblocks < ((int64_t)1 << 31),
                "cells x tiles of samples exceed 2^31 workgroups: fewer samples per call");
    return 0;
}
#undef SWEEP_CHECK

int sweep_put_cells(hipStream_t st, const SweepPlan& plan, SweepCell* dev) {
    const int64_t ncell = plan.Nx * plan.Ny;
    for (int64_t k0 = 0; k0 < ncell; k0 += SWEEP_PUT) {
        SweepCellPack pack;
        const int n = (int)std::min<int64_t>(SWEEP_PUT, ncell - k0);
        memset((void*)&pack, 0, sizeof(pack));
        for (int i = 0; i < n; ++i) pack.c[i] = plan.tab[(size_t)(k0 + i)];
        hipLaunchKernelGGL(put_cells_kernel, dim3(1), dim3(64), 0, st, pack, n, dev + k0);
        TN_CHECK_LAUNCH("put_cells_kernel");
    }
    return 0;
}

int sweep_once(hipStream_t st, const SweepPlan& plan, const SweepCell* dev, int16_t* states, int mode, double beta, const SweepBetas& rb,
               const double* uniforms, int64_t ldu, uint8_t* chg) {
    for (int colour = 0; colour < 2; ++colour) {
        SweepArgs a;
        a.cells = dev; a.states = states; a.uniforms = uniforms; a.chg = chg;
        a.Nx = plan.Nx; a.Ny = plan.Ny; a.M = plan.M; a.ldu = ldu; a.ntiles = plan.ntiles; a.colour = colour; a.mode = mode; a.beta = beta;
        a.rb = rb;
        const int64_t* lds = plan.lds_bytes[colour];
        if (rb.betas) {
            if (plan.present[colour][0]) BS((launch_sweep<0, true>(st, a, plan.nblocks, lds[0])));
            if (plan.present[colour][1]) BS((launch_sweep<1, true>(st, a, plan.nblocks, lds[1])));
            if (plan.present[colour][2]) BS((launch_sweep<2, true>(st, a, plan.nblocks, lds[2])));
            if (plan.present[colour][3]) BS((launch_sweep<3, true>(st, a, plan.nblocks, lds[3])));
        } else {
            if (plan.present[colour][0]) BS((launch_sweep<0, false>(st, a, plan.nblocks, lds[0])));
            if (plan.present[colour][1]) BS((launch_sweep<1, false>(st, a, plan.nblocks, lds[1])));
            if (plan.present[colour][2]) BS((launch_sweep<2, false>(st, a, plan.nblocks, lds[2])));
            if (plan.present[colour][3]) BS((launch_sweep<3, false>(st, a, plan.nblocks, lds[3])));
        }
    }
    return 0;
}

int sweep_energy(hipStream_t st, const SweepPlan& plan, const SweepCell* dev, const int16_t* states, double* energy) {
    hipLaunchKernelGGL(sweep_energy_kernel, dim3((unsigned)cdiv(plan.M, 256)), dim3(256), 0, st, dev, states, plan.Nx, plan.Ny, plan.M, energy);
    TN_CHECK_LAUNCH("sweep_energy_kernel");
    return 0;
}

}  // namespace tn

using namespace tn;

extern "C" {

int64_t tn_cell_sweep_ws_bytes(int64_t Nx, int64_t Ny, int64_t M) {
    if (Nx < 1 || Ny < 1 || M < 1 || M >= ((int64_t)1 << 31)) return 0;             // 0: a shape the call refuses
    int64_t n = 0, b = 0;
    if (__builtin_mul_overflow(Nx, Ny, &n) || n >= ((int64_t)1 << 31) || __builtin_mul_overflow(n, M, &b)) return 0;
    return sweep_layout(nullptr, Nx, Ny, M).bytes;
}

int tn_cell_sweep(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int16_t* states, int mode, double beta, int64_t sweeps,
                  const double* uniforms, int64_t ldu, double* energy_out, int32_t* moves_out, int32_t* last_moves_out, void* ws, int64_t ws_bytes,
                  void* stream) {
    TN_CHECK_ARG(Nx >= 1 && Ny >= 1 && cells, "Nx, Ny: non-positive, or cells: null");
    TN_CHECK_ARG(M >= 1 && M < ((int64_t)1 << 31), "M: outside 1 .. 2^31 - 1");
    TN_CHECK_ARG(mode == 0 || mode == 1, "mode: 0 (heat bath) or 1 (quench)");
    TN_CHECK_ARG(sweeps >= 0, "sweeps: negative");
    TN_CHECK_ARG(states && energy_out, "states / energy_out: null");
    if (mode == 0) {
        TN_CHECK_ARG(beta > 0.0 && beta <= std::numeric_limits<double>::max(), "beta: not positive or not finite");
        TN_CHECK_ARG(uniforms, "uniforms: null in heat-bath mode");
        TN_CHECK_ARG(ldu >= M, "ldu: rows of uniforms shorter than M");
    } else {
        TN_CHECK_ARG(!uniforms, "uniforms: must be null in quench mode");
    }
    const int64_t need = tn_cell_sweep_ws_bytes(Nx, Ny, M);
    TN_CHECK_ARG(need > 0, "Nx x Ny x M: too large");
    const int64_t ncell = Nx * Ny;
    SweepPlan plan;
    BS(sweep_plan(__func__, Nx, Ny, cells, M, plan));
    TN_CHECK_ARG(ws, "ws: null");
    if (ws_bytes < need) {
        set_error("tn_cell_sweep: workspace too small (%lld bytes, tn_cell_sweep_ws_bytes asks for %lld)", (long long)ws_bytes, (long long)need);
        return -3;
    }
    hipStream_t st = (hipStream_t)stream;
    const SweepWs w = sweep_layout(ws, Nx, Ny, M);
    BS(sweep_put_cells(st, plan, w.cells));
    const bool count = moves_out || last_moves_out;
    const unsigned mblk = (unsigned)cdiv(M, 256);
    const SweepBetas one{nullptr, nullptr, 0};
    for (int64_t j = 0; j < sweeps; ++j) {
        BS(sweep_once(st, plan, w.cells, states, mode, beta, one, mode == 0 ? uniforms + j * ncell * ldu : nullptr, ldu, count ? w.chg : nullptr));
        if (count) {
            hipLaunchKernelGGL(sweep_moves_kernel, dim3(mblk), dim3(256), 0, st, w.chg, ncell, M, j == 0 ? 1 : 0, moves_out, last_moves_out);
            TN_CHECK_LAUNCH("sweep_moves_kernel");
        }
    }
    if (sweeps == 0) {
        if (moves_out) BSH(hipMemsetAsync(moves_out, 0, (size_t)M * 4, st), "tn_cell_sweep: clear");
        if (last_moves_out) BSH(hipMemsetAsync(last_moves_out, 0, (size_t)M * 4, st), "tn_cell_sweep: clear");
    }
    return sweep_energy(st, plan, w.cells, states, energy_out);
}

}  // extern "C"
