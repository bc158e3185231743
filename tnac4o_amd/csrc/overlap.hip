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
//
// Second moments of the distances within word groups of the rows (tn_pair_moments), behind tnac4o.calculate_overlap_correlations:
// described where its kernels start, further down.
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

// bin d summed over the slabs (nbins bins of two limbs each), with carry (nslab = 0: zero)
__device__ __forceinline__ ulonglong2 slab_sum(const unsigned long long* __restrict__ slabs, int64_t nslab, int64_t nbins, int64_t d) {
    unsigned long long lo = 0, hi = 0;
    for (int64_t s = 0; s < nslab; ++s) {
        const ulonglong2 v = ((const ulonglong2*)(slabs + s * 2 * nbins))[d];
        lo += v.x;
        hi += v.y + (lo < v.x ? 1u : 0u);
    }
    return make_ulonglong2(lo, hi);
}

// hist_out[d] = sum over the slabs, with carry; every bin is written (nslab = 0: zeros)
__global__ __launch_bounds__(256) void pair_hist_reduce_kernel(const unsigned long long* __restrict__ slabs, int64_t nslab, int64_t nbins,
                                                               unsigned long long* __restrict__ hist_out) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= nbins) return;
    ((ulonglong2*)hist_out)[d] = slab_sum(slabs, nslab, nbins, d);
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

// ---- tn_pair_moments: out[i][j] = sum_{a<b} w_a w_b d_i(a, b) d_j(a, b), d_g the distance within word group g of the row, d_G = 1 -----
// pair_moments_kernel: tiles of 32 x 32 rows of the upper triangle, 256 threads, 2 x 2 pairs each; pair q = (2 i + j) 256 + tid of a
// tile.  Phase 1 passes the groups through LDS in chunks of up to PM_CW words (whole groups; word-major as stage_block) and writes
// the distances of every group into the table D[g][q] (uint16, a row of PM_DPITCH entries per group; row G holds the constant 1)
// and the products p[q] = w_a w_b (0 for b <= a, rows >= M, zero weights) next to it.  Phase 2: the ne = (G+1)(G+2)/2 elements
// i <= j (row-major over the upper triangle) times nsl = EPT 256 / ne slices of the pairs are dealt to the threads as units, EPT per
// thread (3 for G <= 26, else 9), so that few lanes idle whatever ne is; a unit walks its slice two pairs at a time (one dword of D
// holds two pairs) and adds p d_i d_j to a 128-bit accumulator in registers that lives across all tiles of the persistent loop
// (within a tile: 32 x 32 -> 64-bit multiply-adds on the two halves of p, which cannot overflow).  The slices of an element are
// added up once, at the end, through LDS.  Threads of a wave hold consecutive j of (mostly) one i: the d_i read is a broadcast, the
// d_j reads fall on consecutive banks because a row of D is 513 dwords.  Integer adds only, one slab of ne elements per workgroup:
// pair_moments_reduce_kernel adds the slabs with carry and writes [i][j] and [j][i].
constexpr int PM_TILE = 32;                      // rows per block of a tile
constexpr int PM_PAIRS = PM_TILE * PM_TILE;      // pairs of a tile
constexpr int PM_CW = 32;                        // words of a row per chunk: at least one whole group
constexpr int PM_PITCH = PM_TILE + 2;            // words between two chunk words in LDS (16-byte aligned)
constexpr int PM_DPITCH = PM_PAIRS + 2;          // uint16 entries between two groups of the distance table: 513 dwords, an odd number
constexpr int PM_MAX_G = 64, PM_MAX_WPG = 32;
constexpr int64_t PM_STAGE_BYTES = 2 * PM_CW * PM_PITCH * 8;
constexpr int64_t PM_P_BYTES = PM_PAIRS * 8;
static_assert(PM_STAGE_BYTES + PM_P_BYTES + (PM_MAX_G + 1) * PM_DPITCH * 2 <= PH_LDS, "the largest G must fit the LDS");
static_assert((uint64_t)PM_PAIRS * (64 * PM_MAX_WPG) * (64 * PM_MAX_WPG) <= ((uint64_t)1 << 32), "a tile's sum of half-products stays below 2^64");

inline int64_t pair_moments_lds(int64_t G) { return PM_STAGE_BYTES + PM_P_BYTES + (G + 1) * PM_DPITCH * 2; }
inline int64_t pair_moments_ne(int64_t G) { return (G + 1) * (G + 2) / 2; }

// element e of the upper triangle of a (G + 1) x (G + 1) matrix, row-major: (i, j) with i <= j
__host__ __device__ __forceinline__ void pair_moments_ij(int e, int G, int& i, int& j) {
    i = 0;
    while (e >= G + 1 - i) {
        e -= G + 1 - i;
        ++i;
    }
    j = i + e;
}

// rows [r0, r0 + 32) x words [k0, k0 + cw) into dst[k * PM_PITCH + r]; rows >= M read as 0 and are never addressed
__device__ __forceinline__ void stage_group_block(uint64_t* dst, const uint64_t* __restrict__ rows, int64_t M, int64_t ldr, int64_t r0, int64_t k0,
                                                  int cw) {
    const int k = threadIdx.x & (PM_CW - 1);
    for (int r = threadIdx.x / PM_CW; r < PM_TILE; r += 256 / PM_CW) {
        const int64_t row = r0 + r;
        dst[k * PM_PITCH + r] = (row < M && k < cw) ? rows[row * ldr + k0 + k] : 0;
    }
}

template <bool LANES16, int EPT>
__global__ __launch_bounds__(256) void pair_moments_kernel(const uint64_t* __restrict__ rows, int64_t M, int G, int wpg, int64_t ldr,
                                                           const uint32_t* __restrict__ weights, uint32_t wmax, int ne, int64_t ntiles,
                                                           unsigned long long* __restrict__ slabs) {
    extern __shared__ unsigned long long pm_lds[];
    uint64_t* sA = (uint64_t*)pm_lds;
    uint64_t* sB = sA + PM_CW * PM_PITCH;
    unsigned long long* P = pm_lds + 2 * PM_CW * PM_PITCH;
    uint16_t* D = (uint16_t*)(P + PM_PAIRS);
    const uint32_t* D2 = (const uint32_t*)D;                   // two pairs per dword
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    for (int q = tid; q < PM_PAIRS; q += 256) D[G * PM_DPITCH + q] = 1;       // the pseudo-group: read after the barriers of the first tile
    // the thread's units: unit u = tid + 256 n is element u % ne of slice u / ne of the pairs; there are nsl = EPT 256 / ne >= 1 slices,
    // slice s takes the pair dwords s, s + nsl, ...; a unit beyond nsl ne starts behind the last pair and never runs
    const int nsl = EPT * 256 / ne;
    unsigned oi[EPT], oj[EPT];
    int q0[EPT];
    unsigned long long lo[EPT], hi[EPT];
#pragma unroll
    for (int n = 0; n < EPT; ++n) {
        const int u = tid + 256 * n, sl = u / ne;
        int i, j;
        pair_moments_ij(u % ne, G, i, j);
        oi[n] = (unsigned)i * (PM_DPITCH / 2);
        oj[n] = (unsigned)j * (PM_DPITCH / 2);
        q0[n] = sl < nsl ? sl : PM_PAIRS / 2;
        lo[n] = 0;
        hi[n] = 0;
    }
    const int gpc = PM_CW / wpg;                               // whole groups per chunk
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t bj = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);        // as pair_hist_kernel
        while (bj > 0 && bj * (bj + 1) / 2 > t) --bj;
        while ((bj + 1) * (bj + 2) / 2 <= t) ++bj;
        const int64_t bi = t - bj * (bj + 1) / 2;
        const int64_t a0 = bi * PM_TILE, b0 = bj * PM_TILE;
        // ---- phase 1: distances and products of the tile's pairs
        for (int g0 = 0; g0 < G; g0 += gpc) {
            const int ng = min(gpc, G - g0);
            __syncthreads();                                   // the previous chunk, or phase 2 of the previous tile, has been read
            stage_group_block(sA, rows, M, ldr, a0, (int64_t)g0 * wpg, ng * wpg);
            stage_group_block(sB, rows, M, ldr, b0, (int64_t)g0 * wpg, ng * wpg);
            if (g0 == 0) {
                unsigned long long wa[2], wb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int64_t ra = a0 + ty * 2 + i, rb = b0 + tx * 2 + i;
                    wa[i] = ra < M ? (weights ? min(weights[ra], wmax) : 1u) : 0u;
                    wb[i] = rb < M ? (weights ? min(weights[rb], wmax) : 1u) : 0u;
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) P[(i * 2 + j) * 256 + tid] = a0 + ty * 2 + i < b0 + tx * 2 + j ? wa[i] * wb[j] : 0ull;
            }
            __syncthreads();
            for (int gg = 0; gg < ng; ++gg) {
                unsigned dist[2][2] = {{0, 0}, {0, 0}};
                for (int k = gg * wpg; k < (gg + 1) * wpg; ++k) {
                    const ulonglong2 a = *(const ulonglong2*)&sA[k * PM_PITCH + ty * 2];
                    const ulonglong2 b = *(const ulonglong2*)&sB[k * PM_PITCH + tx * 2];
                    dist[0][0] += pair_dist<LANES16>(a.x, b.x);
                    dist[0][1] += pair_dist<LANES16>(a.x, b.y);
                    dist[1][0] += pair_dist<LANES16>(a.y, b.x);
                    dist[1][1] += pair_dist<LANES16>(a.y, b.y);
                }
                uint16_t* dg = D + (g0 + gg) * PM_DPITCH + tid;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) dg[(i * 2 + j) * 256] = (uint16_t)dist[i][j];
            }
        }
        __syncthreads();
        // ---- phase 2: acc[i][j] += p d_i d_j over the tile's pairs.  Within a tile the two 32-bit halves of p are multiplied and added
        // up apart, in 64 bits: d_i d_j <= 2^22, so a term is below 2^54 and the at most 1024 terms of a tile stay below 2^64; the two
        // sums are folded into the 128-bit accumulator once per tile
        unsigned long long sl0[EPT], sh0[EPT];
#pragma unroll
        for (int n = 0; n < EPT; ++n) {
            sl0[n] = 0;
            sh0[n] = 0;
        }
        for (int k = 0; k < PM_PAIRS / 2; k += nsl) {
#pragma unroll
            for (int n = 0; n < EPT; ++n) {
                const int q2 = q0[n] + k;
                if (q2 < PM_PAIRS / 2) {
                    const ulonglong2 p = ((const ulonglong2*)P)[q2];
                    const uint32_t di = D2[oi[n] + q2], dj = D2[oj[n] + q2];
                    const uint32_t dd0 = (di & 0xffffu) * (dj & 0xffffu), dd1 = (di >> 16) * (dj >> 16);
                    sl0[n] += (unsigned long long)(uint32_t)p.x * dd0;
                    sh0[n] += (unsigned long long)(uint32_t)(p.x >> 32) * dd0;
                    sl0[n] += (unsigned long long)(uint32_t)p.y * dd1;
                    sh0[n] += (unsigned long long)(uint32_t)(p.y >> 32) * dd1;
                }
            }
        }
#pragma unroll
        for (int n = 0; n < EPT; ++n) {
            const unsigned long long t = sh0[n] << 32;
            lo[n] += sl0[n];
            hi[n] += lo[n] < sl0[n] ? 1u : 0u;
            lo[n] += t;
            hi[n] += (sh0[n] >> 32) + (lo[n] < t ? 1u : 0u);
        }
    }
    __syncthreads();
    ulonglong2* out = (ulonglong2*)(slabs + (int64_t)blockIdx.x * 2 * ne);
    ulonglong2* red = (ulonglong2*)pm_lds;                     // the slices of an element, added with carry: EPT 256 units
#pragma unroll
    for (int n = 0; n < EPT; ++n) red[tid + 256 * n] = make_ulonglong2(lo[n], hi[n]);
    __syncthreads();
    for (int e = tid; e < ne; e += 256) {
        unsigned long long l = 0, h = 0;
        for (int sl = 0; sl < nsl; ++sl) {
            const ulonglong2 v = red[sl * ne + e];
            l += v.x;
            h += v.y + (l < v.x ? 1u : 0u);
        }
        out[e] = make_ulonglong2(l, h);
    }
}

// out[i][j] = out[j][i] = element (i, j) summed over the slabs, with carry; every entry is written (nslab = 0: zeros)
__global__ __launch_bounds__(256) void pair_moments_reduce_kernel(const unsigned long long* __restrict__ slabs, int64_t nslab, int G, int ne,
                                                                  unsigned long long* __restrict__ out) {
    const int e = (int)blockIdx.x * 256 + threadIdx.x;
    if (e >= ne) return;
    const ulonglong2 v = slab_sum(slabs, nslab, ne, e);
    int i, j;
    pair_moments_ij(e, G, i, j);
    ((ulonglong2*)out)[i * (G + 1) + j] = v;
    ((ulonglong2*)out)[j * (G + 1) + i] = v;
}

inline int64_t pair_moments_tiles(int64_t M) {
    if (M < 2) return 0;
    const int64_t nblk = cdiv(M, PM_TILE);
    return nblk * (nblk + 1) / 2;
}
// workgroups of the persistent grid: what fits 256 compute units with this much LDS each (at most 4 per unit), or TN_PAIR_MOMENTS_WGS
// (read per call); never more than there are tiles
inline int64_t pair_moments_wgs(int64_t M, int64_t G) {
    int64_t g = env_i64("TN_PAIR_MOMENTS_WGS", 0);
    if (g <= 0) g = 256 * std::min<int64_t>(4, PH_LDS / pair_moments_lds(G));
    return std::min<int64_t>(std::min<int64_t>(g, PH_MAX_WGS), pair_moments_tiles(M));
}
inline int64_t pair_moments_dmax(int64_t wpg, int lanes16) { return (lanes16 ? 4 : 64) * wpg; }
inline bool pair_moments_shape_ok(int64_t M, int64_t G, int64_t wpg) {
    return M >= 0 && M < ((int64_t)1 << 31) && G >= 1 && G <= PM_MAX_G && wpg >= 1 && wpg <= PM_MAX_WPG;
}

template <bool LANES16, int EPT>
void pair_moments_launch(hipStream_t st, int64_t nwg, size_t lds, const uint64_t* rows, int64_t M, int G, int wpg, int64_t ldr, const uint32_t* weights,
                         uint32_t wmax, int ne, int64_t ntiles, unsigned long long* slabs) {
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)pair_moments_kernel<LANES16, EPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    prof_begin(st, PROF_MISC);
    hipLaunchKernelGGL((pair_moments_kernel<LANES16, EPT>), dim3((unsigned)nwg), dim3(256), lds, st, rows, M, G, wpg, ldr, weights, wmax, ne, ntiles,
                       slabs);
    prof_end(st, PROF_MISC, 0.0, 0.0);
}
// elements per thread: 3 while that gives every element at least two slices of the pairs, else 9
constexpr int PM_EPT_SMALL = 3, PM_EPT_LARGE = 9, PM_NE_SMALL = PM_EPT_SMALL * 256 / 2;
static_assert((PM_MAX_G + 1) * (PM_MAX_G + 2) / 2 <= PM_EPT_LARGE * 256, "nine elements per thread cover the largest G");
static_assert(PM_STAGE_BYTES >= PM_EPT_SMALL * 256 * 16, "the staging area holds the units of the final sum at three per thread");
static_assert(PM_STAGE_BYTES + PM_P_BYTES + 2 * PM_DPITCH * 28 >= PM_EPT_LARGE * 256 * 16 && 28 * 29 / 2 > PM_NE_SMALL,
              "and the whole LDS of G >= 27 those at nine per thread");
template <bool LANES16, typename... A>
void pair_moments_launch_ept(int ne, A... a) {
    if (ne <= PM_NE_SMALL) pair_moments_launch<LANES16, PM_EPT_SMALL>(a...);
    else pair_moments_launch<LANES16, PM_EPT_LARGE>(a...);
}

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

int64_t tn_pair_moments_ws_bytes(int64_t M, int64_t G, int64_t wpg, int lanes16) {
    (void)lanes16;
    if (!pair_moments_shape_ok(M, G, wpg)) return 0;
    return std::max<int64_t>(pair_moments_wgs(M, G), 1) * pair_moments_ne(G) * 16;
}

int tn_pair_moments(const uint64_t* rows, int64_t M, int64_t G, int64_t wpg, int64_t ldr, const uint32_t* weights, uint32_t wmax, int lanes16,
                    uint64_t* out, void* ws, int64_t ws_bytes, void* stream) {
    TN_CHECK_ARG(M >= 0 && M < ((int64_t)1 << 31), "M negative or not below 2^31");
    TN_CHECK_ARG(G >= 1 && G <= PM_MAX_G, "G outside 1 .. 64 (the number of groups)");
    TN_CHECK_ARG(wpg >= 1 && wpg <= PM_MAX_WPG, "wpg outside 1 .. 32 (the words of a group)");
    TN_CHECK_ARG(wmax >= 1, "wmax must be at least 1");
    const int64_t dmax = pair_moments_dmax(wpg, lanes16);
    if ((uint64_t)wmax * (uint64_t)dmax > 0xffffffffull) {
        set_error("tn_pair_moments: wmax * dmax = %llu * %lld exceeds the limit of 2^32 - 1 = 4294967295 (every term w_a w_b d_i d_j must stay below 2^64)",
                  (unsigned long long)wmax, (long long)dmax);
        return -1;
    }
    TN_CHECK_ARG(rows && out && ws, "null operand");
    TN_CHECK_ARG(ldr >= G * wpg, "ldr shorter than a row of G * wpg words");
    const int64_t need = tn_pair_moments_ws_bytes(M, G, wpg, lanes16);
    if (ws_bytes < need) {
        set_error("tn_pair_moments: workspace too small (%lld bytes, tn_pair_moments_ws_bytes asks for %lld)", (long long)ws_bytes, (long long)need);
        return -3;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t ntiles = pair_moments_tiles(M), nwg = pair_moments_wgs(M, G);
    const int ne = (int)pair_moments_ne(G);
    unsigned long long* slabs = (unsigned long long*)ws;
    if (nwg > 0) {
        const size_t lds = (size_t)pair_moments_lds(G);
        if (lanes16)
            pair_moments_launch_ept<true>(ne, st, nwg, lds, rows, M, (int)G, (int)wpg, ldr, weights, wmax, ne, ntiles, slabs);
        else
            pair_moments_launch_ept<false>(ne, st, nwg, lds, rows, M, (int)G, (int)wpg, ldr, weights, wmax, ne, ntiles, slabs);
        TN_CHECK_LAUNCH("pair_moments_kernel");
    }
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(pair_moments_reduce_kernel, dim3((unsigned)cdiv(ne, 256)), dim3(256), 0, st, slabs, nwg, (int)G, ne,
                                                     (unsigned long long*)out));
    TN_CHECK_LAUNCH("pair_moments_reduce_kernel");
    return 0;
}

}  // extern "C"
