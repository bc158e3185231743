// tn_anneal: population annealing (Hukushima, Iba; Machta) over M configurations along a schedule of inverse temperatures, whole steps
// on the stream (tnac4o.anneal_population).  A step from beta' to beta is
//   1. Emin = the smallest energy (one workgroup);                                           anneal_min_kernel
//   2. the weights exp(-(beta - beta')(E - Emin)), their running sums inside a tile of 256 rows
//      and the sum of every tile;                                                             anneal_weights_kernel
//   3. the running sums of the tile sums (one wave) -> W, sum w^2;                            anneal_tiles_kernel
//   4. the offsets O_m of systematic resampling from C_m / W * M + u;                         anneal_offsets_kernel
//   5. parent[j] by binary search over O, the family of every new row, the survivors;         anneal_parent_kernel, anneal_survivors_kernel
//   6. the rows themselves, states'[j] = states[parent[j]], into the other copy;              anneal_rows_kernel
//   7. `sweeps` heat-bath sweeps of tn_cell_sweep at beta and its energy pass (sweep.h).
// Every kernel here is a gather or a scan inside one workgroup: one thread owns what it writes, no global atomics, no barrier
// across workgroups, no loop that waits for another workgroup.  Nothing read from device memory is used as an index unchecked.
// The running sums are SEQUENTIAL at every level (lane after lane, wave after wave, tile after tile), so that C is non-decreasing
// in m whatever the weights: O is then non-decreasing without the running maximum of its definition.
#include <limits>

#include "sweep.h"

#pragma clang fp contract(off)

namespace tn {

namespace {

#define BS(call)                   \
    do {                           \
        const int rc__ = (call);   \
        if (rc__) return rc__;     \
    } while (0)

constexpr int ANNEAL_TILE = 256;                     // rows of a tile of the running sums = threads of its workgroup

__device__ __forceinline__ double lane_value(double x, int l) {          // x of lane l (l uniform over the wave)
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, l), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// Running sums of one value per lane, lane after lane on top of `carry` (uniform): returns the wave's inclusive sum of this lane,
// excl = the sum before it, total (uniform) = the sum after lane 63.
__device__ __forceinline__ double wave_running_sum(double x, double carry, double& excl, double& total) {
    const int lane = threadIdx.x & 63;
    double run = carry, inc = 0.0;
    excl = 0.0;
    for (int l = 0; l < 64; ++l) {
        const double xl = lane_value(x, l);
        if (lane == l) excl = run;
        run = run + xl;
        if (lane == l) inc = run;
    }
    total = run;
    return inc;
}

// Emin = the smallest E[m] that is no NaN (NaN when every one is): fmin is exact, so the order does not matter
__global__ __launch_bounds__(1024) void anneal_min_kernel(const double* __restrict__ E, int64_t M, double* __restrict__ emin) {
    __shared__ double red[16];
    double v = __longlong_as_double(0x7ff8000000000000ll);
    for (int64_t m = threadIdx.x; m < M; m += 1024) v = fmin(v, E[m]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) v = fmin(v, red[i]);
        emin[0] = v;
    }
}

// tile t = rows [256 t, 256 t + 256): w_m, cl[m] = the running sum of w inside the tile, tsum[t] = cl of its last row, tsq[t] = its
// sum of w^2 -- all in the sequential order of the header
__global__ __launch_bounds__(ANNEAL_TILE) void anneal_weights_kernel(const double* __restrict__ E, int64_t M, double db, const double* __restrict__ emin,
                                                                     double* __restrict__ cl, double* __restrict__ tsum, double* __restrict__ tsq) {
    __shared__ double sums[2][4];
    const int64_t m = (int64_t)blockIdx.x * ANNEAL_TILE + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    double w = 0.0;
    if (m < M) {
        const double d = E[m] - emin[0];
        const double x = db * d;
        w = exp(-x);
        if (!(w >= 0.0)) w = 0.0;                                        // (a NaN weight counts as 0)
    }
    double excl, total, sq_excl, sq_total;
    const double inc = wave_running_sum(w, 0.0, excl, total);
    wave_running_sum(w * w, 0.0, sq_excl, sq_total);
    if ((threadIdx.x & 63) == 0) { sums[0][wave] = total; sums[1][wave] = sq_total; }
    __syncthreads();
    double c = inc;
    if (wave > 0) {
        double base = sums[0][0];
        for (int i = 1; i < wave; ++i) base = base + sums[0][i];
        c = base + inc;
    }
    if (m < M) cl[m] = c;
    if (threadIdx.x == ANNEAL_TILE - 1) {
        tsum[blockIdx.x] = c;
        tsq[blockIdx.x] = ((sums[1][0] + sums[1][1]) + sums[1][2]) + sums[1][3];
    }
}

// one wave: toff[t] = the sum of the tiles before t, tile after tile; W and the sum of w^2 after the last
__global__ __launch_bounds__(64) void anneal_tiles_kernel(const double* __restrict__ tsum, const double* __restrict__ tsq, int64_t ntiles,
                                                          double* __restrict__ toff, double* __restrict__ wsum, double* __restrict__ w2sum) {
    double carry = 0.0, sq_carry = 0.0;
    for (int64_t t0 = 0; t0 < ntiles; t0 += 64) {
        const int64_t t = t0 + threadIdx.x;
        double excl, sq_excl;
        wave_running_sum(t < ntiles ? tsum[t] : 0.0, carry, excl, carry);
        wave_running_sum(t < ntiles ? tsq[t] : 0.0, sq_carry, sq_excl, sq_carry);
        if (t < ntiles) toff[t] = excl;
    }
    if (threadIdx.x == 0) { wsum[0] = carry; w2sum[0] = sq_carry; }
}

// O_m of the header; W zero or not finite: O_m = m + 1 (the identity)
__device__ __forceinline__ int64_t anneal_offset(int64_t m, int64_t M, double W, double u, const double* __restrict__ cl, const double* __restrict__ toff) {
    if (m < 0) return 0;
    if (m >= M - 1) return M;
    if (!(W > 0.0 && W <= std::numeric_limits<double>::max())) return m + 1;
    const double c = toff[m / ANNEAL_TILE] + cl[m];
    const double q = c / W;
    const double p = q * (double)M;
    const double f = floor(p + u);
    return f >= 0.0 ? (f < (double)M ? (int64_t)f : M) : 0;              // (a NaN gives 0)
}

__global__ __launch_bounds__(ANNEAL_TILE) void anneal_offsets_kernel(const double* __restrict__ cl, const double* __restrict__ toff, const double* __restrict__ wsum,
                                                                     const double* __restrict__ ures, int64_t M, int32_t* __restrict__ O,
                                                                     int32_t* __restrict__ tcount) {
    __shared__ int red[4];
    const int64_t m = (int64_t)blockIdx.x * ANNEAL_TILE + threadIdx.x;
    int alive = 0;
    if (m < M) {
        const double W = wsum[0], u = ures[0];
        const int64_t o = anneal_offset(m, M, W, u, cl, toff);
        alive = o > anneal_offset(m - 1, M, W, u, cl, toff);
        O[m] = (int32_t)o;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) alive += __shfl_xor(alive, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = alive;
    __syncthreads();
    if (threadIdx.x == 0) tcount[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void anneal_survivors_kernel(const int32_t* __restrict__ tcount, int64_t ntiles, int32_t* __restrict__ survivors) {
    __shared__ int red[4];
    int n = 0;
    for (int64_t t = threadIdx.x; t < ntiles; t += 256) n += tcount[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) survivors[0] = red[0] + red[1] + red[2] + red[3];
}

// parent[j] = the smallest m with O_m > j: at most 31 halvings of [0, M - 1], whatever O holds the result lies inside it
__global__ __launch_bounds__(256) void anneal_parent_kernel(const int32_t* __restrict__ O, int64_t M, const int32_t* __restrict__ family,
                                                            int32_t* __restrict__ parent, int32_t* __restrict__ family_new, int32_t* ptrace) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    int64_t lo = 0, hi = M - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int64_t mid = (lo + hi) >> 1;
        if (O[mid] > j) hi = mid;
        else lo = mid + 1;
    }
    parent[j] = (int32_t)lo;
    family_new[j] = family[lo];
    if (ptrace) ptrace[j] = (int32_t)lo;
}

// states'[j] = states[parent[j]] in pieces of V: one thread per piece, cpr pieces per row
template <typename V>
__global__ __launch_bounds__(256) void anneal_rows_kernel(const V* __restrict__ src, V* __restrict__ dst, const int32_t* __restrict__ parent, int64_t M,
                                                          int64_t cpr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * cpr) return;
    const int64_t j = i / cpr, c = i % cpr;
    int64_t p = parent[j];
    if (p < 0 || p >= M) p = j;
    dst[i] = src[p * cpr + c];
}

template <typename V>
int rows_launch(hipStream_t st, const int16_t* src, int16_t* dst, const int32_t* parent, int64_t M, int64_t row_bytes) {
    const int64_t cpr = row_bytes / (int64_t)sizeof(V);
    hipLaunchKernelGGL(anneal_rows_kernel<V>, dim3((unsigned)cdiv(M * cpr, 256)), dim3(256), 0, st, (const V*)src, (V*)dst, parent, M, cpr);
    TN_CHECK_LAUNCH("anneal_rows_kernel");
    return 0;
}

__global__ __launch_bounds__(256) void anneal_trace_kernel(const double* __restrict__ E, int64_t M, double* __restrict__ etrace) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m < M) etrace[m] = E[m];
}

// the workspace of tn_anneal: the table of the cells, the second copy of the rows and of the families, and what a step's scan holds
struct AnnealWs {
    SweepCell* cells;
    int16_t* rows;
    int32_t* family;
    double* cl;
    int32_t* O;
    int32_t* parent;
    double* tsum;
    double* tsq;
    double* toff;
    int32_t* tcount;
    int64_t bytes;
};
AnnealWs anneal_layout(void* ws, int64_t Nx, int64_t Ny, int64_t M) {
    WsCarve w{(char*)ws};
    AnnealWs s;
    const int64_t ntiles = cdiv(M, ANNEAL_TILE);
    s.cells = w.take<SweepCell>(sweep_cells_bytes(Nx, Ny));
    s.rows = w.take<int16_t>(M * Nx * Ny * 2);
    s.family = w.take<int32_t>(M * 4);
    s.cl = w.take<double>(M * 8);
    s.O = w.take<int32_t>(M * 4);
    s.parent = w.take<int32_t>(M * 4);
    s.tsum = w.take<double>(ntiles * 8);
    s.tsq = w.take<double>(ntiles * 8);
    s.toff = w.take<double>(ntiles * 8);
    s.tcount = w.take<int32_t>(ntiles * 4);
    s.bytes = w.total();
    return s;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int64_t tn_anneal_ws_bytes(int64_t Nx, int64_t Ny, int64_t M) {
    const int64_t two31 = (int64_t)1 << 31;
    if (Nx < 1 || Ny < 1 || M < 1 || M >= two31) return 0;                                    // 0: a shape the call refuses
    int64_t n = 0, b = 0;
    if (__builtin_mul_overflow(Nx, Ny, &n) || n >= two31 || __builtin_mul_overflow(n, M, &b) || cdiv(b, 256) >= two31) return 0;
    return anneal_layout(nullptr, Nx, Ny, M).bytes;
}

int tn_anneal(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t K, const double* betas, int16_t* states, int32_t* family,
              int64_t sweeps, const double* usweep, int64_t ldu, const double* ures, double* energy_out, double* emin_out, double* wsum_out,
              double* w2sum_out, int32_t* survivors_out, double* energy_trace, int32_t* parent_trace, void* ws, int64_t ws_bytes, void* stream) {
    const int64_t two31 = (int64_t)1 << 31;
    TN_CHECK_ARG(Nx >= 1 && Ny >= 1 && cells, "Nx, Ny: non-positive, or cells: null");
    TN_CHECK_ARG(M >= 1 && M < two31, "M: outside 1 .. 2^31 - 1");
    TN_CHECK_ARG(K >= 1 && K <= two31, "K: outside 1 .. 2^31");
    TN_CHECK_ARG(betas, "betas: null");
    TN_CHECK_ARG(betas[0] >= 0.0 && betas[0] <= std::numeric_limits<double>::max(), "betas: betas[0] is negative or not finite");
    for (int64_t s = 1; s < K; ++s) {
        TN_CHECK_ARG(betas[s] <= std::numeric_limits<double>::max(), "betas: an entry is not finite");
        TN_CHECK_ARG(betas[s] > betas[s - 1], "betas: not strictly increasing");
    }
    TN_CHECK_ARG(sweeps >= 0 && sweeps <= two31, "sweeps: negative, or above 2^31");
    TN_CHECK_ARG(states && family && energy_out, "states / family / energy_out: null");
    if (K > 1) {
        TN_CHECK_ARG(ures, "ures: null with K > 1");
        TN_CHECK_ARG(emin_out && wsum_out && w2sum_out && survivors_out, "emin_out / wsum_out / w2sum_out / survivors_out: null with K > 1");
        TN_CHECK_ARG(mul_fits({K - 1, M, 8}), "K x M: too large");
        if (sweeps > 0) {
            TN_CHECK_ARG(usweep, "usweep: null with sweeps > 0");
            TN_CHECK_ARG(ldu >= M, "ldu: rows of usweep shorter than M");
            TN_CHECK_ARG(mul_fits({K - 1, sweeps, Nx, Ny, ldu}), "K x sweeps x Nx x Ny x ldu: too large");
        }
    }
    const int64_t need = tn_anneal_ws_bytes(Nx, Ny, M);
    TN_CHECK_ARG(need > 0, "Nx x Ny x M: too large");
    SweepPlan plan;
    BS(sweep_plan(__func__, Nx, Ny, cells, M, plan));
    TN_CHECK_ARG(ws, "ws: null");
    if (ws_bytes < need) {
        set_error("tn_anneal: workspace too small (%lld bytes, tn_anneal_ws_bytes asks for %lld)", (long long)ws_bytes, (long long)need);
        return -3;
    }
    hipStream_t st = (hipStream_t)stream;
    const AnnealWs w = anneal_layout(ws, Nx, Ny, M);
    const int64_t ncell = Nx * Ny, ntiles = cdiv(M, ANNEAL_TILE), row_bytes = 2 * ncell;
    const unsigned mblk = (unsigned)cdiv(M, 256);
    // the widest piece (a power of two, at most 16 bytes) that divides a row and the address of both copies
    const uint64_t align = (uint64_t)(uintptr_t)states | (uint64_t)(uintptr_t)w.rows | (uint64_t)row_bytes;
    const int piece = (align & 15) == 0 ? 16 : (align & 7) == 0 ? 8 : (align & 3) == 0 ? 4 : 2;
    BS(sweep_put_cells(st, plan, w.cells));
    BS(sweep_energy(st, plan, w.cells, states, energy_out));
    int16_t *cur = states, *alt = w.rows;
    int32_t *fcur = family, *falt = w.family;
    const SweepBetas one{nullptr, nullptr, 0};
    for (int64_t s = 1; s < K; ++s) {
        const double db = betas[s] - betas[s - 1];
        hipLaunchKernelGGL(anneal_min_kernel, dim3(1), dim3(1024), 0, st, energy_out, M, emin_out + (s - 1));
        TN_CHECK_LAUNCH("anneal_min_kernel");
        hipLaunchKernelGGL(anneal_weights_kernel, dim3((unsigned)ntiles), dim3(ANNEAL_TILE), 0, st, energy_out, M, db, emin_out + (s - 1), w.cl, w.tsum, w.tsq);
        TN_CHECK_LAUNCH("anneal_weights_kernel");
        hipLaunchKernelGGL(anneal_tiles_kernel, dim3(1), dim3(64), 0, st, w.tsum, w.tsq, ntiles, w.toff, wsum_out + (s - 1), w2sum_out + (s - 1));
        TN_CHECK_LAUNCH("anneal_tiles_kernel");
        hipLaunchKernelGGL(anneal_offsets_kernel, dim3((unsigned)ntiles), dim3(ANNEAL_TILE), 0, st, w.cl, w.toff, wsum_out + (s - 1), ures + (s - 1), M, w.O,
                           w.tcount);
        TN_CHECK_LAUNCH("anneal_offsets_kernel");
        hipLaunchKernelGGL(anneal_survivors_kernel, dim3(1), dim3(256), 0, st, w.tcount, ntiles, survivors_out + (s - 1));
        TN_CHECK_LAUNCH("anneal_survivors_kernel");
        hipLaunchKernelGGL(anneal_parent_kernel, dim3(mblk), dim3(256), 0, st, w.O, M, fcur, w.parent, falt,
                           parent_trace ? parent_trace + (s - 1) * M : nullptr);
        TN_CHECK_LAUNCH("anneal_parent_kernel");
        if (piece == 16) BS(rows_launch<uint4>(st, cur, alt, w.parent, M, row_bytes));
        else if (piece == 8) BS(rows_launch<uint2>(st, cur, alt, w.parent, M, row_bytes));
        else if (piece == 4) BS(rows_launch<uint32_t>(st, cur, alt, w.parent, M, row_bytes));
        else BS(rows_launch<uint16_t>(st, cur, alt, w.parent, M, row_bytes));
        std::swap(cur, alt);
        std::swap(fcur, falt);
        for (int64_t j = 0; j < sweeps; ++j)
            BS(sweep_once(st, plan, w.cells, cur, 0, betas[s], one, usweep + ((s - 1) * sweeps + j) * ncell * ldu, ldu, nullptr));
        BS(sweep_energy(st, plan, w.cells, cur, energy_out));
        if (energy_trace) {
            hipLaunchKernelGGL(anneal_trace_kernel, dim3(mblk), dim3(256), 0, st, energy_out, M, energy_trace + (s - 1) * M);
            TN_CHECK_LAUNCH("anneal_trace_kernel");
        }
    }
    if (cur != states) {                                                 // an odd number of steps: the result goes home
        const hipError_t e1 = hipMemcpyAsync(states, cur, (size_t)(M * row_bytes), hipMemcpyDeviceToDevice, st);
        if (e1 != hipSuccess) return hip_fail(e1, "tn_anneal: copy of the rows");
        const hipError_t e2 = hipMemcpyAsync(family, fcur, (size_t)(M * 4), hipMemcpyDeviceToDevice, st);
        if (e2 != hipSuccess) return hip_fail(e2, "tn_anneal: copy of the families");
    }
    return 0;
}

}  // extern "C"
