// tn_ladder_measure: one measurement of the overlap histograms of a tempering ladder, added to accumulators on the device
// (tnac4o.temper_samples(measure=)).  The M = R T rows of tn_temper are T groups of R rows addressed through slot;
// for every temperature the distances of its chain pairs are counted, over the spin bits and (optionally) over the link bits.
//   1. states -> packed spin bits: temper.hip's kernel through its launcher (one source of the conversion);
//   2. ladder_links_kernel: link row bit l = row bit links[l][0] XOR row bit links[l][1], one thread per (row, word);
//   3. ladder_pair_kernel, once for both row sets (blockIdx.y): the chain pairs of a temperature in tiles of 16 x 16 chains, 256 threads
//      with one pair each; the 32 rows of a tile pass through LDS in chunks of LD_CW words (word-major: the 16 threads that share a row
//      read one address, the 16 rows of the other side consecutive ones).  G workgroups share the tiles of a temperature (tile g, g + G,
//      ...); a workgroup counts into its own uint32 histogram in LDS with integer atomics and writes it once, into its slab of the
//      workspace.  At most R (R - 1) / 2 < 2^32 pairs (R <= 65536) reach one workgroup: no bin can wrap;
//   4. ladder_reduce_kernel adds the slabs of a temperature into the caller's 64-bit accumulators, one thread per bin;
//   5. ladder_energy_kernel: one thread per temperature adds E and E^2 of its rows in ascending chain order (fp64, not contracted).
// Integer counts throughout 1 - 4: the result does not depend on G, on the tile order or on the run.  Nothing read from slot, links or
// bitcell is used as an index unchecked; a workgroup writes its own slab, a thread its own bins: no global atomics, no barrier across
// workgroups, no host synchronisation.
#include "sweep.h"

#pragma clang fp contract(off)

namespace tn {

namespace {

#define BS(call)                   \
    do {                           \
        const int rc__ = (call);   \
        if (rc__) return rc__;     \
    } while (0)

constexpr int LD_TILE = 16;                              // chains on each side of a tile
constexpr int LD_ROWS = 2 * LD_TILE;                     // rows of a tile in LDS
constexpr int LD_CW = 32;                                // words of a row per chunk
constexpr int LD_PITCH = LD_ROWS + 1;                    // words between two chunk words in LDS (odd: the staging stores spread over the banks)
constexpr int64_t LD_LDS = 160 * 1024;                   // LDS of a compute unit
constexpr int64_t LD_STAGE_BYTES = (int64_t)LD_CW * LD_PITCH * 8 + LD_ROWS * 4;     // the chunk and the row of every chain of the tile
constexpr int64_t LD_MAX_BINS = (LD_LDS - LD_STAGE_BYTES) / 4;
constexpr int64_t LD_MAX_NBITS = LD_MAX_BINS - 1;        // 38815 (include/tnpeps.h, K19)
constexpr int64_t LD_MAX_R = 65536;                      // R (R - 1) / 2 < 2^32
constexpr int64_t LD_DEFAULT_WGS = 4 * 256;              // workgroups of the pair kernel per row set: 4 on each of 256 compute units
constexpr int64_t LD_MAX_WGS = 4096;                     // workgroups per temperature at most
static_assert(LD_MAX_NBITS == 38815 && LD_MAX_NBITS >= 16384, "the limit include/tnpeps.h states");

struct LadderSet {                                       // a set of packed rows and where its counts go
    const uint64_t* rows;                                // M rows of nwords words
    uint32_t* slabs;                                     // T x G slabs of nbins bins
    unsigned long long* hist;                            // T x nbins accumulators
    int64_t nwords, nbins;
    uint64_t last_mask;
};
struct LadderSets { LadderSet s[2]; };

inline uint64_t ladder_last_mask(int64_t nbits) {
    const int used = (int)(nbits - (cdiv(nbits, 64) - 1) * 64);
    return used == 64 ? ~(uint64_t)0 : (((uint64_t)1 << used) - 1);
}

// tiles of the chain pairs of one temperature.  split = 0: the upper triangle of the n x n blocks of 16 chains, diagonal included,
// folded into a rectangle (row r of the triangle beside row n - r or n - 1 - r: integers only); split > 0: the rectangle of the blocks of
// the chains [0, split) times the blocks of the chains [split, R)
__host__ __device__ __forceinline__ int64_t ld_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }      // (common.h's cdiv is host only)
__host__ __device__ __forceinline__ int64_t ladder_tiles(int64_t R, int64_t split) {
    if (split > 0) return ld_cdiv(split, LD_TILE) * ld_cdiv(R - split, LD_TILE);
    if (R < 2) return 0;
    const int64_t n = ld_cdiv(R, LD_TILE);
    return n * (n + 1) / 2;
}
__device__ __forceinline__ void ladder_decode(int64_t tile, int64_t R, int64_t split, int64_t& a0, int64_t& b0) {
    if (split > 0) {
        const int64_t nb = ld_cdiv(R - split, LD_TILE);
        a0 = tile / nb * LD_TILE;
        b0 = split + tile % nb * LD_TILE;
        return;
    }
    const int64_t n = ld_cdiv(R, LD_TILE), W = n | 1, r = tile / W, c = tile % W;
    int64_t bi = r, bj = r + c;
    if (c >= n - r) {
        bi = n - r - ((n & 1) ? 0 : 1);
        bj = bi + (c - (n - r));
    }
    a0 = bi * LD_TILE;
    b0 = bj * LD_TILE;
}

// link rows: one thread per (row, word) gathers its 64 links; an entry of links outside [0, nbits) makes the link bit 0
__global__ __launch_bounds__(256) void ladder_links_kernel(const uint64_t* __restrict__ rows, int64_t M, int nbits, int nwords,
                                                           const int32_t* __restrict__ links, int nlinks, int lwords, uint64_t* __restrict__ lrows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * lwords) return;
    const int64_t m = i / lwords;
    const int w = (int)(i % lwords);
    const uint64_t* row = rows + m * nwords;
    uint64_t word = 0;
    for (int b = 0; b < 64; ++b) {
        const int l = w * 64 + b;
        if (l >= nlinks) break;
        const int p = links[2 * l], q = links[2 * l + 1];
        if (p < 0 || p >= nbits || q < 0 || q >= nbits) continue;
        word |= (((row[p >> 6] >> (p & 63)) ^ (row[q >> 6] >> (q & 63))) & 1) << b;
    }
    lrows[i] = word;
}

__global__ __launch_bounds__(256) void ladder_pair_kernel(LadderSets sets, const int32_t* __restrict__ slot, int64_t M, int64_t R, int64_t T,
                                                          int64_t split, int64_t ntile, int64_t G) {
    extern __shared__ uint64_t ld_lds[];
    uint64_t* stage = ld_lds;
    int32_t* rowidx = (int32_t*)(stage + LD_CW * LD_PITCH);
    uint32_t* hist = (uint32_t*)(rowidx + LD_ROWS);
    const LadderSet S = sets.s[blockIdx.y];
    const int64_t t = blockIdx.x / G, g = blockIdx.x % G;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    for (int64_t d = tid; d < S.nbins; d += 256) hist[d] = 0;
    for (int64_t tile = g; tile < ntile; tile += G) {
        int64_t a0, b0;
        ladder_decode(tile, R, split, a0, b0);
        __syncthreads();                                       // the previous tile has been read (first pass: the histogram is cleared)
        if (tid < LD_ROWS) {                                   // the row of every chain of the tile; -1: no such chain, or a slot entry out of range
            const int64_t c = tid < LD_TILE ? a0 + tid : b0 + (tid - LD_TILE);
            const int64_t end = (tid < LD_TILE && split > 0) ? split : R;
            int32_t row = -1;
            if (c < end) {
                const int32_t s = slot[c * T + t];
                if (s >= 0 && s < M) row = s;
            }
            rowidx[tid] = row;
        }
        __syncthreads();
        unsigned dist = 0;
        for (int64_t k0 = 0; k0 < S.nwords; k0 += LD_CW) {
            if (k0) __syncthreads();                           // the previous chunk has been read
            const int k = tid & (LD_CW - 1);
            for (int r = tid / LD_CW; r < LD_ROWS; r += 256 / LD_CW) {
                const int64_t row = rowidx[r], w = k0 + k;
                uint64_t v = 0;
                if (row >= 0 && w < S.nwords) {
                    v = S.rows[row * S.nwords + w];
                    if (w == S.nwords - 1) v &= S.last_mask;
                }
                stage[k * LD_PITCH + r] = v;
            }
            __syncthreads();
            const int kn = (int)(S.nwords - k0 < LD_CW ? S.nwords - k0 : LD_CW);
            for (int k2 = 0; k2 < kn; ++k2) dist += (unsigned)__popcll(stage[k2 * LD_PITCH + ti] ^ stage[k2 * LD_PITCH + LD_TILE + tj]);
        }
        // ca < cb; with a split ca < split <= cb holds for every pair of the rectangle
        if (rowidx[ti] >= 0 && rowidx[LD_TILE + tj] >= 0 && a0 + ti < b0 + tj) atomicAdd(&hist[dist], 1u);
    }
    __syncthreads();
    uint32_t* out = S.slabs + (t * G + g) * S.nbins;
    for (int64_t d = tid; d < S.nbins; d += 256) out[d] = hist[d];
}

// hist[t][d] += the slabs of temperature t, one thread per bin
__global__ __launch_bounds__(256) void ladder_reduce_kernel(LadderSets sets, int64_t T, int64_t G) {
    const LadderSet S = sets.s[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * S.nbins) return;
    const int64_t t = i / S.nbins, d = i % S.nbins;
    unsigned long long sum = 0;
    for (int64_t g = 0; g < G; ++g) sum += S.slabs[(t * G + g) * S.nbins + d];
    S.hist[i] += sum;
}

// esums[3 t ..] += 1, sum E, sum E^2 over the rows of temperature t, chains ascending; a slot entry out of range is skipped
__global__ __launch_bounds__(256) void ladder_energy_kernel(const int32_t* __restrict__ slot, const double* __restrict__ E, int64_t M, int64_t R, int64_t T,
                                                            double* __restrict__ esums) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t c = 0; c < R; ++c) {
        const int32_t s = slot[c * T + t];
        if (s < 0 || s >= M) continue;
        const double e = E[s];
        s1 += e;
        s2 += e * e;
    }
    esums[3 * t] += 1.0;
    esums[3 * t + 1] += s1;
    esums[3 * t + 2] += s2;
}

// workgroups that share the tiles of one temperature: TN_LADDER_WGS (read per call) where it is positive, else as many as give the
// pair kernel LD_DEFAULT_WGS workgroups over the T temperatures; never more than `tiles`, than LD_MAX_WGS, or than a grid of 2^31 - 1 takes
inline int64_t ladder_wgs(int64_t T, int64_t tiles) {
    const int64_t asked = env_i64("TN_LADDER_WGS", 0);
    const int64_t g = asked > 0 ? asked : std::max<int64_t>(1, LD_DEFAULT_WGS / T);
    return std::max<int64_t>(1, std::min(std::min(g, tiles), std::min(LD_MAX_WGS, (((int64_t)1 << 31) - 1) / T)));
}

struct LadderWs {
    SweepCell* cells;
    uint64_t* rows;
    uint64_t* lrows;
    uint32_t* slabs;
    uint32_t* lslabs;
    int64_t bytes;
};
// G: the workgroups per temperature of the largest tile count a split can give (split = 0)
LadderWs ladder_layout(void* ws, int64_t Nx, int64_t Ny, int64_t M, int64_t T, int64_t nbits, int64_t nlinks) {
    WsCarve w{(char*)ws};
    LadderWs s;
    const int64_t tiles = ladder_tiles(M / T, 0), G = tiles > 0 ? ladder_wgs(T, tiles) : 0;      // (R < 2: no pair, no slab)
    s.cells = w.take<SweepCell>(sweep_cells_bytes(Nx, Ny));
    s.rows = w.take<uint64_t>(M * cdiv(nbits, 64) * 8);
    s.lrows = w.take<uint64_t>(M * cdiv(nlinks, 64) * 8);
    s.slabs = w.take<uint32_t>(T * G * (nbits + 1) * 4);
    s.lslabs = w.take<uint32_t>(nlinks > 0 ? T * G * (nlinks + 1) * 4 : 0);
    s.bytes = w.total();
    return s;
}

inline bool ladder_shape_ok(int64_t Nx, int64_t Ny, int64_t M, int64_t T, int64_t nbits, int64_t nlinks) {
    const int64_t two31 = (int64_t)1 << 31;
    if (Nx < 1 || Ny < 1 || M < 0 || M >= two31 || T < 1 || T >= two31 || M % T != 0 || M / T > LD_MAX_R) return false;
    if (nbits < 1 || nbits > LD_MAX_NBITS || nlinks < 0 || nlinks > LD_MAX_NBITS) return false;
    int64_t n = 0;
    if (__builtin_mul_overflow(Nx, Ny, &n) || n >= two31) return false;
    const int64_t nw = cdiv(nbits, 64), lw = cdiv(nlinks, 64);
    if (!mul_fits({M, nw, 8}) || !mul_fits({M, lw, 8}) || cdiv(M * nw, 256) >= two31 || cdiv(M * lw, 256) >= two31) return false;
    return mul_fits({T, LD_MAX_WGS, std::max(nbits, nlinks) + 1, 4}) && cdiv(T * (std::max(nbits, nlinks) + 1), 256) < two31;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int64_t tn_ladder_measure_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t T, int64_t nbits, int64_t nlinks) {
    if (!ladder_shape_ok(Nx, Ny, M, T, nbits, nlinks)) return 0;                              // 0: a shape the call refuses
    return ladder_layout(nullptr, Nx, Ny, M, T, nbits, nlinks).bytes;
}

int tn_ladder_measure(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t T, const int16_t* states, const int32_t* slot,
                      int64_t nbits, const int32_t* bitcell, const int32_t* links, int64_t nlinks, int64_t split, const double* energy,
                      uint64_t* spin_hist, uint64_t* link_hist, double* esums, void* ws, int64_t ws_bytes, void* stream) {
    const int64_t two31 = (int64_t)1 << 31;
    TN_CHECK_ARG(Nx >= 1 && Ny >= 1 && cells, "Nx, Ny: non-positive, or cells: null");
    TN_CHECK_ARG(M >= 0 && M < two31, "M: outside 0 .. 2^31 - 1");
    TN_CHECK_ARG(T >= 1 && T < two31 && M % T == 0, "T: not positive, or M is no multiple of T");
    const int64_t R = M / T;
    if (R > LD_MAX_R) {
        set_error("tn_ladder_measure: R = M / T = %lld exceeds the limit of %lld (the pairs of one temperature must stay below 2^32)", (long long)R,
                  (long long)LD_MAX_R);
        return -1;
    }
    if (nbits < 1 || nbits > LD_MAX_NBITS || nlinks < 0 || nlinks > LD_MAX_NBITS) {
        set_error("tn_ladder_measure: nbits = %lld outside 1 .. %lld or nlinks = %lld outside 0 .. %lld (the histogram, 4 bytes per bin, and the staging "
                  "must fit 160 KiB of LDS)", (long long)nbits, (long long)LD_MAX_NBITS, (long long)nlinks, (long long)LD_MAX_NBITS);
        return -1;
    }
    TN_CHECK_ARG(states && slot && bitcell && spin_hist, "states / slot / bitcell / spin_hist: null");
    TN_CHECK_ARG(nlinks == 0 || !link_hist || links, "links: null with nlinks > 0 and a link_hist");
    TN_CHECK_ARG(split >= 0 && split <= R, "split: outside 0 .. R");
    TN_CHECK_ARG(ladder_shape_ok(Nx, Ny, M, T, nbits, nlinks), "Nx x Ny, M x words of a row or T x bins: too large");
    SweepPlan plan;
    BS(sweep_plan(__func__, Nx, Ny, cells, M, plan));
    TN_CHECK_ARG(ws, "ws: null");
    const int64_t need = tn_ladder_measure_ws_bytes(Nx, Ny, M, T, nbits, nlinks);
    if (ws_bytes < need) {
        set_error("tn_ladder_measure: workspace too small (%lld bytes, tn_ladder_measure_ws_bytes asks for %lld)", (long long)ws_bytes, (long long)need);
        return -3;
    }
    hipStream_t st = (hipStream_t)stream;
    const LadderWs w = ladder_layout(ws, Nx, Ny, M, T, nbits, nlinks);
    const int64_t nwords = cdiv(nbits, 64), lwords = cdiv(nlinks, 64), ntile = ladder_tiles(R, split);
    const bool with_links = nlinks > 0 && link_hist;
    if (ntile > 0) {
        BS(sweep_put_cells(st, plan, w.cells));
        BS(temper_to_bits_launch(st, w.cells, states, Nx * Ny, M, nbits, bitcell, w.rows));
        if (with_links) {
            hipLaunchKernelGGL(ladder_links_kernel, dim3((unsigned)cdiv(M * lwords, 256)), dim3(256), 0, st, w.rows, M, (int)nbits, (int)nwords, links,
                               (int)nlinks, (int)lwords, w.lrows);
            TN_CHECK_LAUNCH("ladder_links_kernel");
        }
        const int64_t G = ladder_wgs(T, ntile);
        LadderSets sets;
        sets.s[0] = LadderSet{w.rows, w.slabs, (unsigned long long*)spin_hist, nwords, nbits + 1, ladder_last_mask(nbits)};
        sets.s[1] = with_links ? LadderSet{w.lrows, w.lslabs, (unsigned long long*)link_hist, lwords, nlinks + 1, ladder_last_mask(nlinks)} : sets.s[0];
        const unsigned nset = with_links ? 2u : 1u;
        const int64_t maxbins = std::max(nbits, with_links ? nlinks : 0) + 1;
        const size_t lds = (size_t)(LD_STAGE_BYTES + 4 * maxbins);
        if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)ladder_pair_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(ladder_pair_kernel, dim3((unsigned)(T * G), nset), dim3(256), lds, st, sets, slot, M, R, T, split, ntile, G);
        TN_CHECK_LAUNCH("ladder_pair_kernel");
        hipLaunchKernelGGL(ladder_reduce_kernel, dim3((unsigned)cdiv(T * maxbins, 256), nset), dim3(256), 0, st, sets, T, G);
        TN_CHECK_LAUNCH("ladder_reduce_kernel");
    }
    if (energy && esums) {
        hipLaunchKernelGGL(ladder_energy_kernel, dim3((unsigned)cdiv(T, 256)), dim3(256), 0, st, slot, energy, M, R, T, esums);
        TN_CHECK_LAUNCH("ladder_energy_kernel");
    }
    return 0;
}

}  // extern "C"
