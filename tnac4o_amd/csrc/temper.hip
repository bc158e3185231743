// tn_temper: parallel tempering with isoenergetic cluster moves (PT+ICM: Zhu, Ochoa, Katzgraber) over a population of R chains of T
// temperatures each, whole rounds on the stream (tnac4o.temper_samples).  A round is
//   1. `sweeps` heat-bath sweeps of tn_cell_sweep's move, row m at betas[tidx[m]]: the per-row-beta instances of relax.hip's kernels;
//   2. (nbits > 0) states -> packed spin bits, tn_cluster_exchange's move on the row pairs (slot[ca][t], slot[cb][t]) of every
//      temperature t >= cluster_from and every chain pair of the round -- exchange.hip's kernels through their launcher --, bits -> states;
//   3. the energy pass of tn_cell_sweep;
//   4. temperature swaps between t and t + 1 for t of the round's parity: labels move (two entries of slot, two of tidx), rows never.
// Every kernel here is a gather: one thread owns what it writes, no global atomics, no barrier across workgroups; the swap counters
// are reduced inside the one workgroup that serves a temperature.  Nothing read from slot, tidx, cpairs, cellbits or bitcell is used
// as an index unchecked.
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

constexpr int TEMPER_PUT = 32;                       // betas one launch of put_betas_kernel carries in its arguments
constexpr int TEMPER_MAX_CELL_BITS = 15;             // bits of a cell state (int16, q <= 32767)

struct BetaPack { double b[TEMPER_PUT]; };

__global__ __launch_bounds__(64) void put_betas_kernel(BetaPack pack, int n, double* out) {
    const int i = threadIdx.x;
    if (i < n) out[i] = pack.b[i];
}

__device__ __forceinline__ int in_cell(int s, int q) { return (s >= 0 && s < q) ? s : 0; }

// states -> bits: one thread per (row, word) gathers its 64 positions; row bit = 1 - state bit; a state outside its cell is read as 0
__global__ __launch_bounds__(256) void temper_to_bits_kernel(const SweepCell* __restrict__ cells, const int16_t* __restrict__ states, int64_t ncell, int64_t M,
                                                             int nbits, int nwords, const int32_t* __restrict__ bitcell, uint64_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * nwords) return;
    const int64_t m = i / nwords;
    const int w = (int)(i % nwords);
    const int16_t* row = states + m * ncell;
    uint64_t word = 0;
    for (int b = 0; b < 64; ++b) {
        const int pos = w * 64 + b;
        if (pos >= nbits) break;
        const int k = bitcell[2 * pos], j = bitcell[2 * pos + 1];
        if (k < 0 || k >= ncell || j < 0 || j >= TEMPER_MAX_CELL_BITS) continue;
        const int s = in_cell(row[k], cells[k].q);
        word |= (uint64_t)(1 - ((s >> j) & 1)) << b;
    }
    rows[i] = word;
}

// bits -> states: one thread per (row, cell); written only where the state differs from what the cell was read as
__global__ __launch_bounds__(256) void temper_from_bits_kernel(const SweepCell* __restrict__ cells, int16_t* __restrict__ states, int64_t ncell, int64_t M,
                                                               int nbits, int nwords, int nbmax, const int32_t* __restrict__ cellbits,
                                                               const uint64_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * ncell) return;
    const int64_t m = i / ncell, k = i % ncell;
    const int old = in_cell(states[i], cells[k].q);
    int s = old;
    for (int j = 0; j < nbmax; ++j) {
        const int pos = cellbits[k * nbmax + j];
        if (pos < 0 || pos >= nbits) continue;                           // beyond the cell's spins (-1), or no position of a row
        const int bit = (int)((rows[m * nwords + (pos >> 6)] >> (pos & 63)) & 1);
        s = (s & ~(1 << j)) | ((1 - bit) << j);
    }
    if (s != old) states[i] = (int16_t)s;
}

// the row pairs of a round: pair (tt, p) = (slot[ca][t], slot[cb][t]), t = cluster_from + tt; -1, -1 (a pair tn_cluster_exchange's
// kernels leave alone) when a chain index lies outside [0, R)
__global__ __launch_bounds__(256) void temper_pairs_kernel(const int32_t* __restrict__ slot, int64_t R, int64_t T, int64_t cluster_from, int64_t Tc,
                                                           const int32_t* __restrict__ cpairs, int64_t Pc, int32_t* __restrict__ pairs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= Tc * Pc) return;
    const int64_t t = cluster_from + i / Pc, p = i % Pc;
    const int64_t ca = cpairs[2 * p], cb = cpairs[2 * p + 1];
    const bool ok = ca >= 0 && ca < R && cb >= 0 && cb < R;
    pairs[2 * i] = ok ? slot[ca * T + t] : -1;
    pairs[2 * i + 1] = ok ? slot[cb * T + t] : -1;
}

// temperature swaps of one parity: workgroup t serves the pair (t, t + 1) of every chain, a thread a chain at a time
__global__ __launch_bounds__(256) void temper_swap_kernel(const double* __restrict__ betas, const double* __restrict__ E, const double* __restrict__ u,
                                                          int64_t R, int64_t T, int64_t M, int par, int32_t* __restrict__ slot, int32_t* __restrict__ tidx,
                                                          int32_t* __restrict__ accepted, int32_t* __restrict__ attempted) {
    __shared__ int red[2][4];
    const int64_t t = blockIdx.x;
    if ((t & 1) != par || t + 1 >= T) return;                            // (uniform over the workgroup)
    const double db = betas[t + 1] - betas[t];
    int acc = 0, att = 0;
    for (int64_t c = threadIdx.x; c < R; c += 256) {
        const int64_t a = slot[c * T + t], b = slot[c * T + t + 1];
        if (a < 0 || a >= M || b < 0 || b >= M || a == b) continue;
        ++att;
        const double dE = E[b] - E[a];
        const double delta = db * dE;
        if (delta >= 0.0 || u[c * (T - 1) + t] < exp(delta)) {           // (a NaN fails both)
            slot[c * T + t] = (int32_t)b;
            slot[c * T + t + 1] = (int32_t)a;
            tidx[a] = (int32_t)(t + 1);
            tidx[b] = (int32_t)t;
            ++acc;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        att += __shfl_xor(att, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = acc; red[1][threadIdx.x >> 6] = att; }
    __syncthreads();
    if (threadIdx.x == 0) {
        accepted[t] += red[0][0] + red[0][1] + red[0][2] + red[0][3];
        attempted[t] += red[1][0] + red[1][1] + red[1][2] + red[1][3];
    }
}

__global__ __launch_bounds__(256) void temper_trace_kernel(const double* __restrict__ E, const int32_t* __restrict__ tidx, int64_t M, double* etrace,
                                                           int32_t* ttrace) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    if (etrace) etrace[m] = E[m];
    if (ttrace) ttrace[m] = tidx[m];
}

// the workspace of tn_temper: the table of the cells, the betas, the packed rows, the row pairs of a round, and what the cluster
// kernels write when the caller takes no sizes
struct TemperWs {
    SweepCell* cells;
    double* betas;
    uint64_t* rows;
    int32_t* pairs;
    int32_t* size;
    int32_t* diff;
    int64_t bytes;
};
TemperWs temper_layout(void* ws, int64_t Nx, int64_t Ny, int64_t M, int64_t T, int64_t nbits, int64_t Pc) {
    WsCarve w{(char*)ws};
    TemperWs s;
    s.cells = w.take<SweepCell>(sweep_cells_bytes(Nx, Ny));
    s.betas = w.take<double>(T * 8);
    const int64_t np = nbits > 0 ? T * Pc : 0;
    s.rows = w.take<uint64_t>(nbits > 0 ? M * cdiv(nbits, 64) * 8 : 0);
    s.pairs = w.take<int32_t>(np * 8);
    s.size = w.take<int32_t>(np * 4);
    s.diff = w.take<int32_t>(np * 4);
    s.bytes = w.total();
    return s;
}

}  // namespace

// sweep.h: the launch of temper_to_bits_kernel, for tn_temper and tn_ladder_measure (ladder.hip)
int temper_to_bits_launch(hipStream_t st, const SweepCell* cells, const int16_t* states, int64_t ncell, int64_t M, int64_t nbits, const int32_t* bitcell,
                          uint64_t* rows) {
    const int64_t nwords = cdiv(nbits, 64);
    hipLaunchKernelGGL(temper_to_bits_kernel, dim3((unsigned)cdiv(M * nwords, 256)), dim3(256), 0, st, cells, states, ncell, M, (int)nbits, (int)nwords,
                       bitcell, rows);
    TN_CHECK_LAUNCH("temper_to_bits_kernel");
    return 0;
}

}  // namespace tn

using namespace tn;

extern "C" {

int64_t tn_temper_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t T, int64_t nbits, int64_t Pc) {
    const int64_t two31 = (int64_t)1 << 31;
    if (Nx < 1 || Ny < 1 || M < 1 || M >= two31 || T < 1 || T > M || M % T != 0) return 0;      // 0: a shape the call refuses
    if (nbits < 0 || nbits > cluster_exchange_max_nbits() || Pc < 0 || 2 * Pc > M / T) return 0;
    int64_t n = 0, b = 0;
    if (__builtin_mul_overflow(Nx, Ny, &n) || n >= two31 || __builtin_mul_overflow(n, M, &b) || cdiv(b, 256) >= two31) return 0;
    if (!mul_fits({M, cdiv(nbits, 64), 8}) || cdiv(M * cdiv(nbits, 64), 256) >= two31 || T * Pc >= two31) return 0;
    return temper_layout(nullptr, Nx, Ny, M, T, nbits, Pc).bytes;
}

int tn_temper(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t T, const double* betas, int16_t* states, int32_t* tidx,
              int32_t* slot, int64_t round0, int64_t rounds, int64_t sweeps, const double* usweep, int64_t ldu, int64_t nbits, int64_t nbmax,
              const int32_t* cellbits, const int32_t* bitcell, const int32_t* rowptr, const int32_t* cols, int64_t nnz, int64_t cluster_from,
              const int32_t* cpairs, int64_t Pc, const double* ucl, const double* uswap, double* energy_out, int32_t* swap_accepted,
              int32_t* swap_attempted, double* energy_trace, int32_t* tidx_trace, int32_t* size_out, int32_t* diff_out, void* ws, int64_t ws_bytes,
              void* stream) {
    const int64_t two31 = (int64_t)1 << 31;
    TN_CHECK_ARG(Nx >= 1 && Ny >= 1 && cells, "Nx, Ny: non-positive, or cells: null");
    TN_CHECK_ARG(M >= 1 && M < two31, "M: outside 1 .. 2^31 - 1");
    TN_CHECK_ARG(T >= 1 && T <= M && M % T == 0, "T: not positive, or M is no multiple of T");
    TN_CHECK_ARG(betas, "betas: null");
    for (int64_t t = 0; t < T; ++t) {
        TN_CHECK_ARG(betas[t] > 0.0 && betas[t] <= std::numeric_limits<double>::max(), "betas: an entry is not positive or not finite");
        TN_CHECK_ARG(t == 0 || betas[t] > betas[t - 1], "betas: not strictly increasing");
    }
    TN_CHECK_ARG(round0 >= 0 && rounds >= 0 && round0 <= two31 && rounds <= two31, "round0 / rounds: negative, or above 2^31");
    TN_CHECK_ARG(sweeps >= 0 && sweeps <= two31, "sweeps: negative, or above 2^31");
    TN_CHECK_ARG(states && tidx && slot && energy_out, "states / tidx / slot / energy_out: null");
    TN_CHECK_ARG(T == 1 || (swap_accepted && swap_attempted), "swap_accepted / swap_attempted: null with T > 1");
    TN_CHECK_ARG(T == 1 || rounds == 0 || uswap, "uswap: null with T > 1");
    const int64_t R = M / T;
    if (sweeps > 0 && rounds > 0) {
        TN_CHECK_ARG(usweep, "usweep: null with sweeps > 0");
        TN_CHECK_ARG(ldu >= M, "ldu: rows of usweep shorter than M");
        TN_CHECK_ARG(mul_fits({rounds, sweeps, Nx, Ny, ldu}), "rounds x sweeps x Nx x Ny x ldu: too large");
    }
    if (nbits < 0 || nbits > cluster_exchange_max_nbits()) {
        set_error("tn_temper: nbits = %lld outside 0 .. %lld", (long long)nbits, (long long)cluster_exchange_max_nbits());
        return -1;
    }
    int64_t Tc = 0;
    if (nbits > 0) {
        TN_CHECK_ARG(nbmax >= 1 && nbmax <= TEMPER_MAX_CELL_BITS, "nbmax: outside 1 .. 15 (the bits of a cell state)");
        TN_CHECK_ARG(cellbits && bitcell, "cellbits / bitcell: null with nbits > 0");
        TN_CHECK_ARG(nnz >= 0 && nnz < two31, "nnz negative or not below 2^31");
        TN_CHECK_ARG(rowptr && (cols || nnz == 0), "rowptr / cols: null with nbits > 0");
        TN_CHECK_ARG(cluster_from >= 0 && cluster_from <= T, "cluster_from: outside 0 .. T");
        TN_CHECK_ARG(Pc >= 0 && 2 * Pc <= R, "Pc: negative, or more than R / 2 disjoint pairs of R chains");
        Tc = T - cluster_from;
        TN_CHECK_ARG(Pc == 0 || Tc == 0 || rounds == 0 || (cpairs && ucl), "cpairs / ucl: null with cluster moves to make");
        TN_CHECK_ARG(mul_fits({rounds, Tc, Pc, 8}), "rounds x Tc x Pc: too large");
    } else {
        TN_CHECK_ARG(Pc >= 0 && 2 * Pc <= R, "Pc: negative, or more than R / 2 disjoint pairs of R chains");
    }
    const int64_t need = tn_temper_ws_bytes(Nx, Ny, M, T, nbits, Pc);
    TN_CHECK_ARG(need > 0, "Nx x Ny x M (x nbits): too large");
    SweepPlan plan;
    BS(sweep_plan(__func__, Nx, Ny, cells, M, plan));
    TN_CHECK_ARG(ws, "ws: null");
    if (ws_bytes < need) {
        set_error("tn_temper: workspace too small (%lld bytes, tn_temper_ws_bytes asks for %lld)", (long long)ws_bytes, (long long)need);
        return -3;
    }
    hipStream_t st = (hipStream_t)stream;
    const TemperWs w = temper_layout(ws, Nx, Ny, M, T, nbits, Pc);
    const int64_t ncell = Nx * Ny, nwords = cdiv(nbits, 64), np = Tc * Pc;
    const bool cluster = nbits > 0 && np > 0;
    BS(sweep_put_cells(st, plan, w.cells));
    for (int64_t t0 = 0; t0 < T; t0 += TEMPER_PUT) {
        BetaPack pack;
        const int n = (int)std::min<int64_t>(TEMPER_PUT, T - t0);
        for (int i = 0; i < TEMPER_PUT; ++i) pack.b[i] = i < n ? betas[t0 + i] : 0.0;
        hipLaunchKernelGGL(put_betas_kernel, dim3(1), dim3(64), 0, st, pack, n, w.betas + t0);
        TN_CHECK_LAUNCH("put_betas_kernel");
    }
    const SweepBetas rb{w.betas, tidx, T};
    const unsigned mblk = (unsigned)cdiv(M, 256);
    for (int64_t r = 0; r < rounds; ++r) {
        for (int64_t j = 0; j < sweeps; ++j)
            BS(sweep_once(st, plan, w.cells, states, 0, 0.0, rb, usweep + (r * sweeps + j) * ncell * ldu, ldu, nullptr));
        if (cluster) {
            BS(temper_to_bits_launch(st, w.cells, states, ncell, M, nbits, bitcell, w.rows));
            hipLaunchKernelGGL(temper_pairs_kernel, dim3((unsigned)cdiv(np, 256)), dim3(256), 0, st, slot, R, T, cluster_from, Tc, cpairs + r * Pc * 2, Pc,
                               w.pairs);
            TN_CHECK_LAUNCH("temper_pairs_kernel");
            BS(cluster_exchange_launch(st, w.rows, M, nbits, nwords, rowptr, cols, nnz, w.pairs, np, ucl + r * np, size_out ? size_out + r * np : w.size,
                                       diff_out ? diff_out + r * np : w.diff));
            hipLaunchKernelGGL(temper_from_bits_kernel, dim3((unsigned)cdiv(M * ncell, 256)), dim3(256), 0, st, w.cells, states, ncell, M, (int)nbits,
                               (int)nwords, (int)nbmax, cellbits, w.rows);
            TN_CHECK_LAUNCH("temper_from_bits_kernel");
        }
        BS(sweep_energy(st, plan, w.cells, states, energy_out));
        if (T > 1) {
            hipLaunchKernelGGL(temper_swap_kernel, dim3((unsigned)(T - 1)), dim3(256), 0, st, w.betas, energy_out, uswap + r * R * (T - 1), R, T, M,
                               (int)((round0 + r) & 1), slot, tidx, swap_accepted, swap_attempted);
            TN_CHECK_LAUNCH("temper_swap_kernel");
        }
        if (energy_trace || tidx_trace) {
            hipLaunchKernelGGL(temper_trace_kernel, dim3(mblk), dim3(256), 0, st, energy_out, tidx, M, energy_trace ? energy_trace + r * M : nullptr,
                               tidx_trace ? tidx_trace + r * M : nullptr);
            TN_CHECK_LAUNCH("temper_trace_kernel");
        }
    }
    if (rounds == 0) BS(sweep_energy(st, plan, w.cells, states, energy_out));
    return 0;
}

}  // extern "C"
