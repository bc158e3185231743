// Weighted histogram of the pairwise distances of M packed rows (tn_pair_hist): hist[d] = sum_{a<b} w_a w_b [dist(a, b) = d], an exact
// integer in two 64-bit limbs.  Behind tnac4o.calculate_overlap_distribution: the overlap distribution P(q) of a set of samples is
// this histogram over the bit-packed spins (dist = popcount(a XOR b)) or over the 16-bit cell states (dist = lanes that differ).
//
// pair_hist_kernel: the upper triangle of the pair matrix in tiles of 64 x 64 rows, 256 threads with a 4 x 4 sub-tile each.  Both row
// blocks pass through LDS in chunks of PH_CW words (word-major, so a thread reads its four rows with two 16-byte loads); the 16
// running distances stay in registers.  After the last chunk the 16 products w_a w_b go into the workgroup's own histogram in LDS
// with integer atomics: a 64-bit add on the low limb whose returned old value tells whether this add wrapped, in which case 1 goes
// to the high limb -- every wrap is seen by exactly one add, so the two limbs are exact whatever the interleaving.  Products of one
// thread that fall into the same bin in a row are added up in registers first (identical rows: 16 times fewer atomics).  The grid is
// persistent: workgroup g takes tiles g, g + G, ... and writes its histogram once, into slab g of the workspace;
// pair_hist_reduce_kernel adds the slabs bin by bin with carry and writes every bin of the result.  Integer sums: the result does not
// depend on G, on the tile order or on the run.
#include "common.h"

namespace tn {

namespace {

constexpr int PH_TILE = 64;                      // rows per block of a tile
constexpr int PH_CW = 16;                        // words of a row per chunk
constexpr int PH_PITCH = PH_TILE + 2;            // words between two chunk words in LDS (16-byte aligned, spreads the staging stores)
constexpr int64_t PH_LDS = 160 * 1024;           // LDS of a compute unit
constexpr int64_t PH_STAGE_BYTES = 2 * PH_CW * PH_PITCH * 8;
constexpr int64_t PH_MAX_BINS = (PH_LDS - PH_STAGE_BYTES) / 16;
constexpr int PH_MAX_WGS = 4096;

template <bool LANES16>
__device__ __forceinline__ unsigned pair_dist(uint64_t a, uint64_t b) {
    const uint64_t x = a ^ b;
    if (!LANES16) return (unsigned)__popcll(x);
    const uint64_t low = 0x7fff7fff7fff7fffull;  // bit 15 of a lane of t: some bit of that lane of x is set
    const uint64_t t = (((x & low) + low) | x) & ~low;
    return (unsigned)__popcll(t);
}

// rows [r0, r0 + 64) x words [k0, k0 + PH_CW) into dst[k * PH_PITCH + r]; rows >= M and words >= nwords read as 0 and are never
// addressed, the last word of a row is cut to nbits
__device__ __forceinline__ void stage_block(uint64_t* dst, const uint64_t* __restrict__ rows, int64_t M, int64_t ldr, int64_t r0, int64_t k0,
                                            int64_t nwords, uint64_t last_mask) {
    const int k = threadIdx.x & (PH_CW - 1);
    for (int r = threadIdx.x / PH_CW; r < PH_TILE; r += 256 / PH_CW) {
        const int64_t row = r0 + r, w = k0 + k;
        uint64_t v = 0;
        if (row < M && w < nwords) {
            v = rows[row * ldr + w];
            if (w == nwords - 1) v &= last_mask;
        }
        dst[k * PH_PITCH + r] = v;
    }
}

// acc += p into bin d of the workgroup's histogram (interleaved lo, hi), exactly
__device__ __forceinline__ void hist_add(unsigned long long* hist, unsigned d, unsigned long long lo, unsigned long long hi) {
    const unsigned long long old = atomicAdd(&hist[2 * d], lo);
    if (old + lo < old) ++hi;
    if (hi) atomicAdd(&hist[2 * d + 1], hi);
}

template <bool LANES16>
__global__ __launch_bounds__(256) void pair_hist_kernel(const uint64_t* __restrict__ rows, int64_t M, int64_t nwords, int64_t ldr, uint64_t last_mask,
                                                        const uint32_t* __restrict__ weights, int64_t nbins, int64_t ntiles,
                                                        unsigned long long* __restrict__ slabs) {
    extern __shared__ unsigned long long ph_lds[];
    uint64_t* sA = (uint64_t*)ph_lds;
    uint64_t* sB = sA + PH_CW * PH_PITCH;
    unsigned long long* hist = ph_lds + 2 * PH_CW * PH_PITCH;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    for (int64_t i = tid; i < 2 * nbins; i += 256) hist[i] = 0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        // tile t of the upper triangle, column by column: bj = the largest j with j (j + 1) / 2 <= t, bi = t - bj (bj + 1) / 2 <= bj
        int64_t bj = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while (bj > 0 && bj * (bj + 1) / 2 > t) --bj;
        while ((bj + 1) * (bj + 2) / 2 <= t) ++bj;
        const int64_t bi = t - bj * (bj + 1) / 2;
        const int64_t a0 = bi * PH_TILE, b0 = bj * PH_TILE;
        unsigned dist[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) dist[i][j] = 0;
        for (int64_t k0 = 0; k0 < nwords; k0 += PH_CW) {
            __syncthreads();                                   // the previous chunk has been read (first pass: the histogram is cleared)
            stage_block(sA, rows, M, ldr, a0, k0, nwords, last_mask);
            stage_block(sB, rows, M, ldr, b0, k0, nwords, last_mask);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < PH_CW; ++k) {
                uint64_t a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[i] = sA[k * PH_PITCH + ty * 4 + i];
                    b[i] = sB[k * PH_PITCH + tx * 4 + i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) dist[i][j] += pair_dist<LANES16>(a[i], b[j]);
            }
        }
        // weights of the thread's rows: 0 for a row past the end, so that its pairs drop out below
        unsigned long long wa[4], wb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t ra = a0 + ty * 4 + i, rb = b0 + tx * 4 + i;
            wa[i] = ra < M ? (weights ? weights[ra] : 1u) : 0u;
            wb[i] = rb < M ? (weights ? weights[rb] : 1u) : 0u;
        }
        unsigned cur = 0;
        unsigned long long lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long p = wa[i] * wb[j];
                if (p == 0 || a0 + ty * 4 + i >= b0 + tx * 4 + j) continue;       // (diagonal tiles keep a < b)
                const unsigned d = dist[i][j];
                if (d != cur) {
                    if (lo | hi) hist_add(hist, cur, lo, hi);
                    cur = d; lo = 0; hi = 0;
                }
                lo += p;
                if (lo < p) ++hi;
            }
        if (lo | hi) hist_add(hist, cur, lo, hi);
    }
    __syncthreads();
    ulonglong2* out = (ulonglong2*)(slabs + (int64_t)blockIdx.x * 2 * nbins);
    for (int64_t d = tid; d < nbins; d += 256) out[d] = make_ulonglong2(hist[2 * d], hist[2 * d + 1]);
}

// hist_out[d] = sum over the slabs, with carry; every bin is written (nslab = 0: zeros)
__global__ __launch_bounds__(256) void pair_hist_reduce_kernel(const unsigned long long* __restrict__ slabs, int64_t nslab, int64_t nbins,
                                                               unsigned long long* __restrict__ hist_out) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= nbins) return;
    unsigned long long lo = 0, hi = 0;
    for (int64_t s = 0; s < nslab; ++s) {
        const ulonglong2 v = ((const ulonglong2*)(slabs + s * 2 * nbins))[d];
        lo += v.x;
        hi += v.y + (lo < v.x ? 1u : 0u);
    }
    ((ulonglong2*)hist_out)[d] = make_ulonglong2(lo, hi);
}

inline int64_t pair_hist_nwords(int64_t nbits, int lanes16) { return lanes16 ? cdiv(nbits, 4) : cdiv(nbits, 64); }
inline int64_t pair_hist_tiles(int64_t M) {
    if (M < 2) return 0;
    const int64_t nblk = cdiv(M, PH_TILE);
    return nblk * (nblk + 1) / 2;
}
// workgroups of the persistent grid: as many as fit the device's 256 compute units with this much LDS each (at most 4 per unit), or
// TN_PAIR_HIST_WGS (read per call); never more than there are tiles
inline int64_t pair_hist_wgs(int64_t M, int64_t nbins) {
    const int64_t tiles = pair_hist_tiles(M);
    int64_t g = env_i64("TN_PAIR_HIST_WGS", 0);
    if (g <= 0) g = 256 * std::min<int64_t>(4, PH_LDS / (PH_STAGE_BYTES + 16 * nbins));
    return std::min<int64_t>(std::min<int64_t>(g, PH_MAX_WGS), tiles);
}
inline bool pair_hist_shape_ok(int64_t M, int64_t nbits) { return M >= 0 && M < ((int64_t)1 << 31) && nbits >= 1 && nbits + 1 <= PH_MAX_BINS; }

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int64_t tn_pair_hist_ws_bytes(int64_t M, int64_t nbits, int lanes16) {
    (void)lanes16;
    if (!pair_hist_shape_ok(M, nbits)) return 0;
    return std::max<int64_t>(pair_hist_wgs(M, nbits + 1), 1) * (nbits + 1) * 16;
}

int tn_pair_hist(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const uint32_t* weights, int lanes16, uint64_t* hist_out, void* ws,
                 int64_t ws_bytes, void* stream) {
    TN_CHECK_ARG(M >= 0 && M < ((int64_t)1 << 31), "M negative or not below 2^31");
    TN_CHECK_ARG(nbits >= 1, "nbits must be positive");
    if (nbits + 1 > PH_MAX_BINS) {
        set_error("tn_pair_hist: nbits = %lld exceeds the limit of %lld (the histogram, 16 bytes per bin, and the staging must fit 160 KiB of LDS)",
                  (long long)nbits, (long long)(PH_MAX_BINS - 1));
        return -1;
    }
    const int64_t nwords = pair_hist_nwords(nbits, lanes16), nbins = nbits + 1;
    TN_CHECK_ARG(rows && hist_out && ws, "null operand");
    TN_CHECK_ARG(ldr >= nwords, "ldr shorter than a row");
    const int64_t need = tn_pair_hist_ws_bytes(M, nbits, lanes16);
    if (ws_bytes < need) {
        set_error("tn_pair_hist: workspace too small (%lld bytes, tn_pair_hist_ws_bytes asks for %lld)", (long long)ws_bytes, (long long)need);
        return -3;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t ntiles = pair_hist_tiles(M), nwg = pair_hist_wgs(M, nbins);
    unsigned long long* slabs = (unsigned long long*)ws;
    if (nwg > 0) {
        const int per = lanes16 ? 4 : 64, used = (int)(nbits - (nwords - 1) * per);            // bits or lanes of the last word that belong to the row
        const uint64_t last_mask = used == per ? ~(uint64_t)0 : (((uint64_t)1 << (used * (lanes16 ? 16 : 1))) - 1);
        const size_t lds = (size_t)(PH_STAGE_BYTES + 16 * nbins);
        const void* fn = lanes16 ? (const void*)pair_hist_kernel<true> : (const void*)pair_hist_kernel<false>;
        if (lds > 48 * 1024) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        prof_begin(st, PROF_MISC);
        if (lanes16)
            hipLaunchKernelGGL(pair_hist_kernel<true>, dim3((unsigned)nwg), dim3(256), lds, st, rows, M, nwords, ldr, last_mask, weights, nbins,
                               ntiles, slabs);
        else
            hipLaunchKernelGGL(pair_hist_kernel<false>, dim3((unsigned)nwg), dim3(256), lds, st, rows, M, nwords, ldr, last_mask, weights, nbins,
                               ntiles, slabs);
        prof_end(st, PROF_MISC, 0.0, 0.0);
        TN_CHECK_LAUNCH("pair_hist_kernel");
    }
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(pair_hist_reduce_kernel, dim3((unsigned)cdiv(nbins, 256)), dim3(256), 0, st, slabs, nwg, nbins,
                                                     (unsigned long long*)hist_out));
    TN_CHECK_LAUNCH("pair_hist_reduce_kernel");
    return 0;
}

}  // extern "C"
