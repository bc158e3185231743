// Exact integer statistics of M packed rows, the samples of tnac4o: four entries, each a persistent grid over the tiles of an upper
// triangle (tn_pair_rowsums: of the full square) whose workgroups write partial sums into slabs of the workspace, and a kernel that
// adds the slabs.  Integer sums throughout: no result depends on the grid, on the tile order or on the run.
//   tn_pair_hist     hist[d] = sum_{a<b} w_a w_b [dist(a, b) = d]                  tnac4o.calculate_overlap_distribution
//   tn_pair_moments  out[i][j] = sum_{a<b} w_a w_b d_i(a, b) d_j(a, b)             tnac4o.calculate_overlap_correlations
//   tn_spin_moments  out[i][j] = sum_a w_a [x_a,i != x_a,j]                        tnac4o.calculate_sample_correlations
//   tn_pair_rowsums  out[a][k] = sum_{b != a} w_b dist(a, b)^k, k = 0 .. 4, ...    tnac4o.calculate_overlap_errors
// dist = popcount(a XOR b) over bit-packed spins, or the 16-bit lanes (cell states) that differ.  Each family is described where its
// kernels start; what they share comes first.
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

// tile t of the upper triangle of a matrix of blocks, column by column: bj = the largest j with j (j + 1) / 2 <= t, bi = t - bj (bj + 1) / 2
// <= bj
__host__ __device__ __forceinline__ void tri_decode(int64_t t, int64_t& bi, int64_t& bj) {
    bj = (int64_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (bj > 0 && bj * (bj + 1) / 2 > t) --bj;
    while ((bj + 1) * (bj + 2) / 2 <= t) ++bj;
    bi = t - bj * (bj + 1) / 2;
}
// tiles of `tile` x `tile` rows in the upper triangle of the M x M pairs, the diagonal ones included (no pair: none)
inline int64_t tri_tiles(int64_t M, int tile) {
    if (M < 2) return 0;
    const int64_t nblk = cdiv(M, tile);
    return nblk * (nblk + 1) / 2;
}

// (lo, hi) += (vlo, vhi): a 128-bit add on two 64-bit limbs.  (Inlined, it is the carry written out by hand, but the compiler's
// schedule and register allocation follow the order in which values are formed: with `run` as one struct in pair_hist_kernel and the
// shifted high sum formed first in pair_moments_kernel, the loops of both compile to the instructions and registers they had before
// this helper; in pair_moments_kernel the fold itself, once per tile, comes out in another order.)
__host__ __device__ __forceinline__ void add128(unsigned long long& lo, unsigned long long& hi, unsigned long long vlo, unsigned long long vhi) {
    lo += vlo;
    hi += vhi + (lo < vlo ? 1u : 0u);
}

// mask of the last word of a row of nbits bits (lanes16: 16-bit lanes): what lies behind the row in that word is cut
inline uint64_t last_word_mask(int64_t nbits, int lanes16) {
    const int per = lanes16 ? 4 : 64, used = (int)(nbits - (cdiv(nbits, per) - 1) * per);
    return used == per ? ~(uint64_t)0 : (((uint64_t)1 << (used * (lanes16 ? 16 : 1))) - 1);
}

// workgroups of a persistent grid: the value of the entry's switch (read per call) where it is positive, else `dflt`; at most PH_MAX_WGS
// and never more than there are units of work
inline int64_t persistent_wgs(int64_t asked, int64_t dflt, int64_t work) {
    return std::min<int64_t>(std::min<int64_t>(asked > 0 ? asked : dflt, PH_MAX_WGS), work);
}

// launch of a persistent kernel of 256 threads with `lds` bytes of dynamic LDS, which it has to be allowed first above 48 KiB
template <typename... P, typename... A>
void launch_persistent(void (*kernel)(P...), hipStream_t st, int64_t nwg, size_t lds, A... args) {
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    prof_begin(st, PROF_MISC);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nwg), dim3(256), lds, st, args...);
    prof_end(st, PROF_MISC, 0.0, 0.0);
}

// What the three entries refuse alike, as TN_CHECK_ARG does (-1, "<entry>: <what>"), and a workspace below what <entry>_ws_bytes asks
// for (-3); 0: nothing to refuse
inline int refuse(const char* entry, const char* what) {
    set_error("%s: %s", entry, what);
    return -1;
}
inline int check_pair_count(const char* entry, int64_t M) {
    return M >= 0 && M < ((int64_t)1 << 31) ? 0 : refuse(entry, "M negative or not below 2^31");
}
inline int check_operands(const char* entry, bool all, int64_t ldr, int64_t nwords, const char* short_row) {
    if (!all) return refuse(entry, "null operand");
    return ldr >= nwords ? 0 : refuse(entry, short_row);
}
inline int check_workspace(const char* entry, int64_t ws_bytes, int64_t need) {
    if (ws_bytes >= need) return 0;
    set_error("%s: workspace too small (%lld bytes, %s_ws_bytes asks for %lld)", entry, (long long)ws_bytes, entry, (long long)need);
    return -3;
}

// ---- tn_pair_hist: hist[d] = sum_{a<b} w_a w_b [dist(a, b) = d], an exact integer in two 64-bit limbs ---------------------------------
// pair_hist_kernel: the upper triangle of the pair matrix in tiles of 64 x 64 rows, 256 threads with a 4 x 4 sub-tile each.  Both row
// blocks pass through LDS in chunks of PH_CW words (word-major, so a thread reads its four rows with two 16-byte loads); the 16
// running distances stay in registers.  After the last chunk the 16 products w_a w_b go into the workgroup's own histogram in LDS
// with integer atomics: a 64-bit add on the low limb whose returned old value tells whether this add wrapped, in which case 1 goes
// to the high limb -- every wrap is seen by exactly one add, so the two limbs are exact whatever the interleaving.  Products of one
// thread that fall into the same bin in a row are added up in registers first (identical rows: 16 times fewer atomics).  The grid is
// persistent: workgroup g takes tiles g, g + G, ... and writes its histogram once, into slab g of the workspace;
// pair_hist_reduce_kernel adds the slabs bin by bin with carry and writes every bin of the result.

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
        int64_t bi, bj;
        tri_decode(t, bi, bj);
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
        struct { unsigned d; unsigned long long lo, hi; } run = {0, 0, 0};             // the pairs in a row that share a bin: the bin, their sum
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long p = wa[i] * wb[j];
                if (p == 0 || a0 + ty * 4 + i >= b0 + tx * 4 + j) continue;       // (diagonal tiles keep a < b)
                const unsigned d = dist[i][j];
                if (d != run.d) {
                    if (run.lo | run.hi) hist_add(hist, run.d, run.lo, run.hi);
                    run.d = d; run.lo = 0; run.hi = 0;
                }
                add128(run.lo, run.hi, p, 0);
            }
        if (run.lo | run.hi) hist_add(hist, run.d, run.lo, run.hi);
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
        add128(lo, hi, v.x, v.y);
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
// the persistent grid: TN_PAIR_HIST_WGS, or as many workgroups as fit the device's 256 compute units with this much LDS each (at most 4
// per unit)
inline int64_t pair_hist_wgs(int64_t M, int64_t nbins) {
    return persistent_wgs(env_i64("TN_PAIR_HIST_WGS", 0), 256 * std::min<int64_t>(4, PH_LDS / (PH_STAGE_BYTES + 16 * nbins)), tri_tiles(M, PH_TILE));
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
        int64_t bi, bj;
        tri_decode(t, bi, bj);
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
            const unsigned long long t = sh0[n] << 32;                            // (formed first: see add128)
            add128(lo[n], hi[n], sl0[n], 0);
            add128(lo[n], hi[n], t, sh0[n] >> 32);
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
            add128(l, h, v.x, v.y);
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

// the persistent grid: TN_PAIR_MOMENTS_WGS, or what fits 256 compute units with this much LDS each (at most 4 per unit)
inline int64_t pair_moments_wgs(int64_t M, int64_t G) {
    return persistent_wgs(env_i64("TN_PAIR_MOMENTS_WGS", 0), 256 * std::min<int64_t>(4, PH_LDS / pair_moments_lds(G)), tri_tiles(M, PM_TILE));
}
inline int64_t pair_moments_dmax(int64_t wpg, int lanes16) { return (lanes16 ? 4 : 64) * wpg; }
inline bool pair_moments_shape_ok(int64_t M, int64_t G, int64_t wpg) {
    return M >= 0 && M < ((int64_t)1 << 31) && G >= 1 && G <= PM_MAX_G && wpg >= 1 && wpg <= PM_MAX_WPG;
}

// elements per thread: 3 while that gives every element at least two slices of the pairs, else 9
constexpr int PM_EPT_SMALL = 3, PM_EPT_LARGE = 9, PM_NE_SMALL = PM_EPT_SMALL * 256 / 2;
static_assert((PM_MAX_G + 1) * (PM_MAX_G + 2) / 2 <= PM_EPT_LARGE * 256, "nine elements per thread cover the largest G");
static_assert(PM_STAGE_BYTES >= PM_EPT_SMALL * 256 * 16, "the staging area holds the units of the final sum at three per thread");
static_assert(PM_STAGE_BYTES + PM_P_BYTES + 2 * PM_DPITCH * 28 >= PM_EPT_LARGE * 256 * 16 && 28 * 29 / 2 > PM_NE_SMALL,
              "and the whole LDS of G >= 27 those at nine per thread");
template <bool LANES16>
auto* pair_moments_instance(int ne) {
    return ne <= PM_NE_SMALL ? &pair_moments_kernel<LANES16, PM_EPT_SMALL> : &pair_moments_kernel<LANES16, PM_EPT_LARGE>;
}

// ---- tn_spin_moments: out[i][j] = sum_a w_a [x_a,i != x_a,j] over every pair of BITS i, j of the rows, two constant pseudo-bits appended -
// The Gram matrix of the rows over the sample index.  spin_transpose_kernel turns the sample-major rows into the bit-major matrix T:
// row i of T holds bit i of the samples 64 c .. 64 c + 63 in word c (KW = ceil(M / 64) words; NB blocks of 64 rows; row n is the
// constant 0, row n + 1 the constant 1, the rows behind them 0), and the weights into P = bit length of wmax plane words
// Wp[p][c] = bit p of min(w_a, wmax) of those samples (0 for a sample >= M, so nothing else needs a mask).  A wave holds word wb of 64
// samples; ballot b is row 64 wb + b of T, kept by lane b and written through LDS so that a row's 16 words leave as one segment.
// spin_moments_kernel is pair_hist_kernel's loop run on T: tiles of 64 x 64 bits of the upper triangle, 256 threads, 4 x 4 each, both
// blocks staged word-major as stage_block does, the chunk's plane words next to them, each chunk fetched into registers while the one
// before it is counted; per word and pair sum_p 2^p popcount((a ^ b) & Wp[p]) by
// Horner over the planes in two halves of at most 16 planes (64 (2^16 - 1) < 2^22 per word and half, 16 words of a chunk < 2^26 in 32
// bits), folded into 16 uint64 sums once per chunk.  The unit of work is (tile, chunk of 16 words), tile-major, and the persistent grid
// cuts the sequence of all units into equal contiguous shares, one per workgroup, so that every workgroup has the same work whatever
// the number of tiles (6 at n = 128).  A share is the end of one tile, whole tiles, and the start of another: a whole tile is written
// into out, [i][j] and [j][i]; the at most two part tiles of workgroup g go to the slabs 2 g (its first piece) and 2 g + 1 of 4096
// partial sums, and spin_moments_reduce_kernel adds the pieces of every tile that was cut.  Integer adds, no atomics: the same integers
// for every grid.
constexpr int SM_TC = 16;                        // word columns of T (blocks of 64 samples) per workgroup of the transposition
constexpr int SM_TPITCH = SM_TC + 1;
constexpr int SM_MAX_P = 32;
constexpr int64_t SM_MAX_NBITS = 65534;          // n + 2 <= 2^16: at most 1024 blocks of 64 rows of T
constexpr int64_t SM_TILE_WORDS = PH_TILE * PH_TILE;

__global__ __launch_bounds__(256) void spin_transpose_kernel(const uint64_t* __restrict__ rows, int64_t M, int64_t nbits, int64_t nwords, int64_t ldr,
                                                             uint64_t last_mask, const uint32_t* __restrict__ weights, uint32_t wmax, int P, int64_t NB,
                                                             int64_t KW, uint64_t* __restrict__ T, uint64_t* __restrict__ Wp) {
    __shared__ uint64_t tile[64 * SM_TPITCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t wb = blockIdx.y, c0 = (int64_t)blockIdx.x * SM_TC;
    const bool planes = wb == NB;                // the last grid row makes the weight planes
    for (int q = 0; q < SM_TC / 4; ++q) {
        const int cl = wave * (SM_TC / 4) + q;
        const int64_t a = (c0 + cl) * 64 + lane;
        const bool valid = a < M;
        uint64_t v = 0;
        if (planes) {
            if (valid) v = weights ? (uint64_t)min(weights[a], wmax) : 1u;
        } else {
            if (valid && wb < nwords) {
                v = rows[a * ldr + wb];
                if (wb == nwords - 1) v &= last_mask;
            }
            if (valid && (nbits + 1) / 64 == wb) v |= (uint64_t)1 << ((nbits + 1) & 63);          // the constant 1; bit n stays 0
        }
        uint64_t mine = 0;
#pragma unroll
        for (int b = 0; b < 64; ++b) {
            const uint64_t m = __ballot((int)((v >> b) & 1u));
            if (lane == b) mine = m;
        }
        tile[lane * SM_TPITCH + cl] = mine;
    }
    __syncthreads();
    const int nrow = planes ? P : 64;
    uint64_t* dst = planes ? Wp : T + wb * 64 * KW;
    for (int e = tid; e < nrow * SM_TC; e += 256) {
        const int r = e / SM_TC, cl = e % SM_TC;
        if (c0 + cl < KW) dst[(int64_t)r * KW + c0 + cl] = tile[r * SM_TPITCH + cl];
    }
}

// share of workgroup g of the nwg: units [spin_share(g), spin_share(g + 1))
__host__ __device__ __forceinline__ int64_t spin_share(int64_t g, int64_t total, int64_t nwg) { return g * total / nwg; }

// UNIT: one plane (wmax = 1 or no weights)
template <bool UNIT>
__global__ __launch_bounds__(256) void spin_moments_kernel(const uint64_t* __restrict__ T, const uint64_t* __restrict__ Wp, int64_t KW,
                                                           int P, int64_t ntiles, int64_t nchunks, int64_t nrows, uint64_t* __restrict__ out,
                                                           int64_t ldo, uint64_t* __restrict__ slabs) {
    __shared__ uint64_t sA[PH_CW * PH_PITCH], sB[PH_CW * PH_PITCH], sW[PH_CW * SM_MAX_P];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t total = ntiles * nchunks;                            // units (tile, chunk), tile-major; this workgroup's share:
    const int64_t end = spin_share((int64_t)blockIdx.x + 1, total, gridDim.x);
    const int plo = min(P, 16);
    int piece = 0;
    for (int64_t u = spin_share(blockIdx.x, total, gridDim.x); u < end; ++piece) {
        const int64_t t = u / nchunks, c0 = u % nchunks, c1 = c0 + end - u < nchunks ? c0 + end - u : nchunks;
        u += c1 - c0;
        int64_t bi, bj;
        tri_decode(t, bi, bj);
        const int64_t a0 = bi * PH_TILE, b0 = bj * PH_TILE;
        uint64_t acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0;
        // the thread's words of a chunk, in stage_block's layout: word k = tid % 16 of the rows tid / 16 + 16 q of both blocks, and two
        // of the chunk's plane words; fetched into registers a chunk ahead, so that the loads are in flight under the popcounts
        uint64_t ra[4], rb[4], rw[2];
        auto fetch = [&](int64_t ch) {
            const int64_t w = ch * PH_CW + (tid & (PH_CW - 1));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t r = tid / PH_CW + (256 / PH_CW) * q;
                ra[q] = w < KW ? T[(a0 + r) * KW + w] : 0;
                rb[q] = w < KW ? T[(b0 + r) * KW + w] : 0;
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int e = tid + 256 * q, k = e / P, p = e % P;
                rw[q] = e < PH_CW * P && ch * PH_CW + k < KW ? Wp[(int64_t)p * KW + ch * PH_CW + k] : 0;
            }
        };
        fetch(c0);
        for (int64_t ch = c0; ch < c1; ++ch) {
            __syncthreads();                                   // the previous chunk has been read
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int at = (tid & (PH_CW - 1)) * PH_PITCH + tid / PH_CW + (256 / PH_CW) * q;
                sA[at] = ra[q];
                sB[at] = rb[q];
            }
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int e = tid + 256 * q;
                if (e < PH_CW * P) sW[(e / P) * SM_MAX_P + e % P] = rw[q];
            }
            __syncthreads();
            if (ch + 1 < c1) fetch(ch + 1);
            unsigned s0[4][4], s1[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) s0[i][j] = s1[i][j] = 0;
#pragma unroll 1                                               // (unrolled, the 16 x 6 operations of a word cost the third workgroup its registers)
            for (int k = 0; k < PH_CW; ++k) {
                uint64_t x[4][4];
                {
                    uint64_t a[4], b[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        a[i] = sA[k * PH_PITCH + ty * 4 + i];
                        b[i] = sB[k * PH_PITCH + tx * 4 + i];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) x[i][j] = a[i] ^ b[j];
                }
                if (UNIT) {
                    const uint64_t w = sW[k * SM_MAX_P];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) s0[i][j] += (unsigned)__popcll(x[i][j] & w);
                } else {
                    unsigned h[4][4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) h[i][j] = 0;
                    for (int p = P - 1; p >= 16; --p) {        // planes 16 .. P-1, in units of 2^16
                        const uint64_t w = sW[k * SM_MAX_P + p];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) h[i][j] = 2 * h[i][j] + (unsigned)__popcll(x[i][j] & w);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            s1[i][j] += h[i][j];
                            h[i][j] = 0;
                        }
                    for (int p = plo - 1; p >= 0; --p) {       // planes 0 .. 15
                        const uint64_t w = sW[k * SM_MAX_P + p];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) h[i][j] = 2 * h[i][j] + (unsigned)__popcll(x[i][j] & w);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) s0[i][j] += h[i][j];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += (uint64_t)s0[i][j] + ((uint64_t)s1[i][j] << 16);
        }
        if (c0 > 0 || c1 < nchunks) {                          // part of a tile: the first piece of the share, or its last
            uint64_t* slab = slabs + (2 * (int64_t)blockIdx.x + (piece ? 1 : 0)) * SM_TILE_WORDS;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) slab[(ty * 4 + i) * PH_TILE + tx * 4 + j] = acc[i][j];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t gi = a0 + ty * 4 + i, gj = b0 + tx * 4 + j;
                    if (gi < nrows && gj < nrows) {
                        out[gi * ldo + gj] = acc[i][j];
                        if (bi != bj) out[gj * ldo + gi] = acc[i][j];          // (a diagonal tile holds both triangles itself)
                    }
                }
        }
    }
}

// out[i][j] (and out[j][i] off the diagonal tiles) = entry (r, c) of tile t summed over its pieces, for every tile that was cut.  The
// workgroups that hold units of tile t, [t nchunks, (t + 1) nchunks), are consecutive; a tile that one of them holds whole is in out
// already.  The piece of workgroup g is in slab 2 g when its share starts inside the tile, else in slab 2 g + 1.
__global__ __launch_bounds__(256) void spin_moments_reduce_kernel(const uint64_t* __restrict__ slabs, int64_t ntiles, int64_t nchunks, int64_t nwg,
                                                                  int64_t nrows, uint64_t* __restrict__ out, int64_t ldo) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ntiles * SM_TILE_WORDS) return;
    const int64_t t = e / SM_TILE_WORDS, total = ntiles * nchunks, lo = t * nchunks, hi = lo + nchunks;
    int64_t g = lo * nwg / total;                                      // the workgroup that holds unit lo
    while (g > 0 && spin_share(g, total, nwg) > lo) --g;
    while (spin_share(g + 1, total, nwg) <= lo) ++g;
    if (spin_share(g + 1, total, nwg) >= hi) return;                   // (it starts at or before lo: the tile is whole)
    const int r = (int)(e % SM_TILE_WORDS) / PH_TILE, c = (int)(e % PH_TILE);
    int64_t bi, bj;
    tri_decode(t, bi, bj);
    const int64_t gi = bi * PH_TILE + r, gj = bj * PH_TILE + c;
    if (gi >= nrows || gj >= nrows) return;
    uint64_t s = 0;
    for (; g < nwg && spin_share(g, total, nwg) < hi; ++g)
        s += slabs[(2 * g + (spin_share(g, total, nwg) >= lo ? 0 : 1)) * SM_TILE_WORDS + r * PH_TILE + c];
    out[gi * ldo + gj] = s;
    if (bi != bj) out[gj * ldo + gi] = s;
}

inline int spin_moments_planes(uint32_t wmax) {
    int P = 0;
    while (wmax) {
        ++P;
        wmax >>= 1;
    }
    return P;
}
inline bool spin_moments_shape_ok(int64_t M, int64_t nbits, uint32_t wmax) {
    return M >= 0 && M < ((int64_t)1 << 32) && nbits >= 1 && nbits <= SM_MAX_NBITS && wmax >= 1;
}
struct SpinMomentsPlan {
    int64_t NB, KW, ntiles, nchunks, nwg;
    int P;
    int64_t t_words, w_words, slab_words;
};
// The persistent grid: TN_SPIN_MOMENTS_WGS (read per call) or what the registers admit on the 256 compute units, 3 workgroups each with
// one plane (160 VGPRs) and 2 with more (234); never more than there are units.  M = 0 keeps one chunk (of zeros) per tile.
inline SpinMomentsPlan spin_moments_plan(int64_t M, int64_t nbits, uint32_t wmax) {
    SpinMomentsPlan p;
    p.NB = cdiv(nbits + 2, PH_TILE);
    p.KW = cdiv(M, 64);
    p.P = spin_moments_planes(wmax);
    p.ntiles = p.NB * (p.NB + 1) / 2;
    p.nchunks = std::max<int64_t>(1, cdiv(p.KW, PH_CW));
    p.nwg = persistent_wgs(env_i64("TN_SPIN_MOMENTS_WGS", 0), 256 * (p.P == 1 ? 3 : 2), p.ntiles * p.nchunks);
    p.t_words = p.NB * PH_TILE * p.KW;
    p.w_words = (int64_t)p.P * p.KW;
    p.slab_words = p.nwg > 1 ? 2 * p.nwg * SM_TILE_WORDS : 0;
    return p;
}

// ---- tn_pair_rowsums: out[a][k] = sum_{b != a} w_b d(a, b)^k (k = 0 .. 4), out[a][5] = sum_{b != a} w_b |nbits - 2 d(a, b)| -----------------
// The pair matrix reduced per ROW instead of per distance bin.  pair_rowsums_kernel walks the full SQUARE of the pair matrix: a unit of
// work is a block of 64 rows a and one of the S segments of the nblk blocks of 64 rows b; the tile loop is pair_hist_kernel's (chunks
// of PH_CW words of both blocks through LDS, a 4 x 4 register block of distances per thread), the diagonal pairs a = b and the rows
// >= M drop out through a weight of 0.  After the K loop of a tile the 4096 distances pass through LDS once (uint16, with the weights
// of the 64 rows b next to them) and are dealt out again, row-wise: thread t takes row a = t / 4 and the 16 rows b of quarter t % 4, so
// that it holds the six 128-bit sums of ONE row, 24 registers that live across the tiles of the unit, and not of the four rows of its
// register block (that form, with the high limbs cut to what the bounds allow, took 155 VGPRs, left 3 waves per SIMD and ran 2 to 3 %
// slower).  Per pair:
// w d^2 in 64 bits, d^3 and d^4 as (w d^2) d and (w d^2) d^2 by a 64 x 64 -> 128 multiply; the sums of w, w d and w |n - 2 d| over the
// 16 pairs stay in 64 bits (below 2^36, 2^52, 2^52) and are folded once per tile.  At the end of a unit the 4 threads of a row --
// 4 consecutive lanes -- are added up with carry by shuffles, and the first of them writes the six sums into slab s of the
// workspace.  The grid is persistent: workgroup g takes the units g, g + G, ...  pair_rowsums_reduce_kernel adds the S slabs of an
// entry with carry (slab_sum) and writes every entry of out.  Integer adds, no atomics, no floating point: the same integers for
// every grid and split.
constexpr int64_t PR_MAX_NBITS = 65535;
constexpr int64_t PR_MAX_ROWS = (int64_t)1 << 31;                  // M stays below
constexpr int64_t PR_DEFAULT_WGS = 4 * 256;                        // 4 workgroups on each of 256 compute units
constexpr int PR_DPITCH = PH_TILE + 8;                             // uint16 entries between two rows a of the distance table (16-byte aligned)
static_assert(PR_MAX_NBITS < (1 << 16), "a distance fits the uint16 of the table");
static_assert((unsigned __int128)0xffffffffull * PR_MAX_NBITS * PR_MAX_NBITS < ((unsigned __int128)1 << 64), "w d^2 fits one limb");
static_assert((unsigned __int128)16 * 0xffffffffull * PR_MAX_NBITS < ((unsigned __int128)1 << 64), "the 16 terms w d, w |n - 2 d| of a tile fit one limb");
static_assert(PR_MAX_NBITS * PR_MAX_NBITS < ((int64_t)1 << 32) && PR_MAX_ROWS <= ((int64_t)1 << 31),
              "w d^4 = (w d^2) d^2 < 2^96 and fewer than 2^31 terms: a row's sum stays below 2^127");

struct PairRowsumsPlan {
    int64_t nblk, S, nwg, ws_bytes;
};
// The one layout of the workspace, for the size query and the call: S slabs of M rows x 6 entries of 16 bytes.  The grid asked for is
// TN_PAIR_ROWSUMS_WGS (read per call) or 4 workgroups per compute unit; the blocks b of a row block are cut into S segments so that
// there are at least that many units, at most one segment per block, and the grid never exceeds the units.
inline PairRowsumsPlan pair_rowsums_plan(int64_t M) {
    PairRowsumsPlan p;
    p.nblk = cdiv(M, PH_TILE);
    const int64_t asked = env_i64("TN_PAIR_ROWSUMS_WGS", 0), want = std::min<int64_t>(asked > 0 ? asked : PR_DEFAULT_WGS, PH_MAX_WGS);
    p.S = p.nblk > 0 ? std::min<int64_t>(cdiv(want, p.nblk), p.nblk) : 0;
    p.nwg = std::min<int64_t>(want, p.nblk * p.S);
    p.ws_bytes = std::max<int64_t>(16, p.S * M * 6 * 16);
    return p;
}
inline bool pair_rowsums_shape_ok(int64_t M, int64_t nbits) { return M >= 0 && M < PR_MAX_ROWS && nbits >= 1 && nbits <= PR_MAX_NBITS; }

template <bool LANES16>
__global__ __launch_bounds__(256) void pair_rowsums_kernel(const uint64_t* __restrict__ rows, int64_t M, int64_t nwords, int64_t ldr, uint64_t last_mask,
                                                           const uint32_t* __restrict__ weights, int nbits, int64_t nblk, int64_t S,
                                                           ulonglong2* __restrict__ slabs) {
    __shared__ uint64_t sA[PH_CW * PH_PITCH], sB[PH_CW * PH_PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t sD[PH_TILE * PR_DPITCH];
    __shared__ uint32_t sW[PH_TILE];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int r = tid >> 2, q = tid & 3;                       // after the K loop: row a0 + r against the rows b0 + 16 q .. b0 + 16 q + 15
    for (int64_t u = blockIdx.x; u < nblk * S; u += gridDim.x) {
        const int64_t ba = u / S, s = u % S, a0 = ba * PH_TILE;
        unsigned long long lo[6], hi[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) lo[k] = hi[k] = 0;
        for (int64_t bb = s * nblk / S; bb < (s + 1) * nblk / S; ++bb) {
            const int64_t b0 = bb * PH_TILE;
            unsigned dist[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) dist[i][j] = 0;
            for (int64_t k0 = 0; k0 < nwords; k0 += PH_CW) {
                __syncthreads();                               // the previous chunk has been read
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
            // The tile's distances, and the weights of its rows b (0 for a row past the end, so that its pairs drop out below), through
            // LDS.  Every thread has passed the barriers of this tile's K loop since it read the table of the tile before.
#pragma unroll
            for (int i = 0; i < 4; ++i)
                *(uint64_t*)&sD[(ty * 4 + i) * PR_DPITCH + tx * 4] =
                    (uint64_t)dist[i][0] | (uint64_t)dist[i][1] << 16 | (uint64_t)dist[i][2] << 32 | (uint64_t)dist[i][3] << 48;
            if (tid < PH_TILE) sW[tid] = b0 + tid < M ? (weights ? weights[b0 + tid] : 1u) : 0u;
            __syncthreads();
            ulonglong2 dv[2];
            dv[0] = *(const ulonglong2*)&sD[r * PR_DPITCH + q * 16];
            dv[1] = *(const ulonglong2*)&sD[r * PR_DPITCH + q * 16 + 8];
            unsigned long long t0 = 0, t1 = 0, t5 = 0;                 // of the 16 pairs: below 2^36, 2^52, 2^52
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const unsigned long long word = j & 4 ? dv[j >> 3].y : dv[j >> 3].x;
                const unsigned long long d = (word >> (16 * (j & 3))) & 0xffffu, dd = d * d;
                const unsigned long long w = a0 + r == b0 + q * 16 + j ? 0ull : (unsigned long long)sW[q * 16 + j];       // (the diagonal pair)
                const unsigned long long p2 = w * dd;
                const int fold = nbits - 2 * (int)d;
                t0 += w;
                t1 += w * d;
                t5 += w * (unsigned long long)(fold < 0 ? -fold : fold);
                add128(lo[2], hi[2], p2, 0);
                add128(lo[3], hi[3], p2 * d, __umul64hi(p2, d));
                add128(lo[4], hi[4], p2 * dd, __umul64hi(p2, dd));
            }
            lo[0] += t0;                                               // (below 2^63 over all rows b: no carry)
            add128(lo[1], hi[1], t1, 0);
            add128(lo[5], hi[5], t5, 0);
        }
        // the 4 threads of a row: lanes 4 r' .. 4 r' + 3 of a wave
#pragma unroll
        for (int m = 1; m < 4; m *= 2)
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const unsigned long long vlo = __shfl_xor(lo[k], m), vhi = __shfl_xor(hi[k], m);
                add128(lo[k], hi[k], vlo, vhi);
            }
        if (q == 0 && a0 + r < M) {
#pragma unroll
            for (int k = 0; k < 6; ++k) slabs[(s * M + a0 + r) * 6 + k] = make_ulonglong2(lo[k], hi[k]);
        }
    }
}

// out[e] = entry e = 6 a + k summed over the S slabs, with carry; every entry is written
__global__ __launch_bounds__(256) void pair_rowsums_reduce_kernel(const unsigned long long* __restrict__ slabs, int64_t nslab, int64_t nent,
                                                                  unsigned long long* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nent) return;
    ((ulonglong2*)out)[e] = slab_sum(slabs, nslab, nent, e);
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
    if (int rc = check_pair_count(__func__, M)) return rc;
    TN_CHECK_ARG(nbits >= 1, "nbits must be positive");
    if (nbits + 1 > PH_MAX_BINS) {
        set_error("tn_pair_hist: nbits = %lld exceeds the limit of %lld (the histogram, 16 bytes per bin, and the staging must fit 160 KiB of LDS)",
                  (long long)nbits, (long long)(PH_MAX_BINS - 1));
        return -1;
    }
    const int64_t nwords = pair_hist_nwords(nbits, lanes16), nbins = nbits + 1;
    if (int rc = check_operands(__func__, rows && hist_out && ws, ldr, nwords, "ldr shorter than a row")) return rc;
    if (int rc = check_workspace(__func__, ws_bytes, tn_pair_hist_ws_bytes(M, nbits, lanes16))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t ntiles = tri_tiles(M, PH_TILE), nwg = pair_hist_wgs(M, nbins);
    unsigned long long* slabs = (unsigned long long*)ws;
    if (nwg > 0) {
        launch_persistent(lanes16 ? &pair_hist_kernel<true> : &pair_hist_kernel<false>, st, nwg, (size_t)(PH_STAGE_BYTES + 16 * nbins), rows, M, nwords, ldr,
                          last_word_mask(nbits, lanes16), weights, nbins, ntiles, slabs);
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
    if (int rc = check_pair_count(__func__, M)) return rc;
    TN_CHECK_ARG(G >= 1 && G <= PM_MAX_G, "G outside 1 .. 64 (the number of groups)");
    TN_CHECK_ARG(wpg >= 1 && wpg <= PM_MAX_WPG, "wpg outside 1 .. 32 (the words of a group)");
    TN_CHECK_ARG(wmax >= 1, "wmax must be at least 1");
    const int64_t dmax = pair_moments_dmax(wpg, lanes16);
    if ((uint64_t)wmax * (uint64_t)dmax > 0xffffffffull) {
        set_error("tn_pair_moments: wmax * dmax = %llu * %lld exceeds the limit of 2^32 - 1 = 4294967295 (every term w_a w_b d_i d_j must stay below 2^64)",
                  (unsigned long long)wmax, (long long)dmax);
        return -1;
    }
    if (int rc = check_operands(__func__, rows && out && ws, ldr, G * wpg, "ldr shorter than a row of G * wpg words")) return rc;
    if (int rc = check_workspace(__func__, ws_bytes, tn_pair_moments_ws_bytes(M, G, wpg, lanes16))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t ntiles = tri_tiles(M, PM_TILE), nwg = pair_moments_wgs(M, G);
    const int ne = (int)pair_moments_ne(G);
    unsigned long long* slabs = (unsigned long long*)ws;
    if (nwg > 0) {
        launch_persistent(lanes16 ? pair_moments_instance<true>(ne) : pair_moments_instance<false>(ne), st, nwg, (size_t)pair_moments_lds(G), rows, M, (int)G,
                          (int)wpg, ldr, weights, wmax, ne, ntiles, slabs);
        TN_CHECK_LAUNCH("pair_moments_kernel");
    }
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(pair_moments_reduce_kernel, dim3((unsigned)cdiv(ne, 256)), dim3(256), 0, st, slabs, nwg, (int)G, ne,
                                                     (unsigned long long*)out));
    TN_CHECK_LAUNCH("pair_moments_reduce_kernel");
    return 0;
}

int64_t tn_spin_moments_ws_bytes(int64_t M, int64_t nbits, uint32_t wmax) {
    if (!spin_moments_shape_ok(M, nbits, wmax)) return 0;
    const SpinMomentsPlan p = spin_moments_plan(M, nbits, wmax);
    return std::max<int64_t>(16, 8 * (p.t_words + p.w_words + p.slab_words));
}

int tn_spin_moments(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const uint32_t* weights, uint32_t wmax, uint64_t* out, int64_t ldo,
                    void* ws, int64_t ws_bytes, void* stream) {
    TN_CHECK_ARG(M >= 0 && M < ((int64_t)1 << 32), "M negative or not below 2^32 = 4294967296 (an entry, at most M (2^32 - 1), must fit 64 bits)");
    if (nbits < 1 || nbits > SM_MAX_NBITS) {
        set_error("tn_spin_moments: nbits = %lld outside 1 .. %lld (n + 2 rows and columns, at most 2^16)", (long long)nbits, (long long)SM_MAX_NBITS);
        return -1;
    }
    TN_CHECK_ARG(wmax >= 1, "wmax must be at least 1");
    const int64_t nwords = cdiv(nbits, 64), nrows = nbits + 2;
    if (int rc = check_operands(__func__, rows && out && ws, ldr, nwords, "ldr shorter than a row")) return rc;
    TN_CHECK_ARG(ldo >= nrows, "ldo shorter than a row of nbits + 2 entries");
    if (int rc = check_workspace(__func__, ws_bytes, tn_spin_moments_ws_bytes(M, nbits, wmax))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const SpinMomentsPlan p = spin_moments_plan(M, nbits, wmax);
    uint64_t* T = (uint64_t*)ws;
    uint64_t* Wp = T + p.t_words;
    uint64_t* slabs = Wp + p.w_words;
    const int P = weights ? p.P : 1;                       // without weights there is one plane, whatever wmax
    if (p.KW > 0) {
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(spin_transpose_kernel, dim3((unsigned)cdiv(p.KW, SM_TC), (unsigned)(p.NB + 1)), dim3(256), 0, st,
                                                         rows, M, nbits, nwords, ldr, last_word_mask(nbits, 0), weights, wmax, P, p.NB, p.KW, T, Wp));
        TN_CHECK_LAUNCH("spin_transpose_kernel");
    }
    launch_persistent(P == 1 ? &spin_moments_kernel<true> : &spin_moments_kernel<false>, st, p.nwg, 0, T, Wp, p.KW, P, p.ntiles, p.nchunks, nrows, out, ldo,
                      slabs);
    TN_CHECK_LAUNCH("spin_moments_kernel");
    if (p.nwg > 1) {
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(spin_moments_reduce_kernel, dim3((unsigned)cdiv(p.ntiles * SM_TILE_WORDS, 256)), dim3(256), 0, st,
                                                         slabs, p.ntiles, p.nchunks, p.nwg, nrows, out, ldo));
        TN_CHECK_LAUNCH("spin_moments_reduce_kernel");
    }
    return 0;
}

int64_t tn_pair_rowsums_ws_bytes(int64_t M, int64_t nbits, int lanes16) {
    (void)lanes16;
    if (!pair_rowsums_shape_ok(M, nbits)) return 0;
    return pair_rowsums_plan(M).ws_bytes;
}

int tn_pair_rowsums(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const uint32_t* weights, int lanes16, uint64_t* out, void* ws,
                    int64_t ws_bytes, void* stream) {
    if (int rc = check_pair_count(__func__, M)) return rc;
    if (nbits < 1 || nbits > PR_MAX_NBITS) {
        set_error("tn_pair_rowsums: nbits = %lld outside 1 .. %lld (w d^2 must stay below 2^64 and a row's sum of w d^4 below 2^127)", (long long)nbits,
                  (long long)PR_MAX_NBITS);
        return -1;
    }
    const int64_t nwords = pair_hist_nwords(nbits, lanes16);
    if (int rc = check_operands(__func__, rows && (out || M == 0) && ws, ldr, nwords, "ldr shorter than a row")) return rc;
    const PairRowsumsPlan p = pair_rowsums_plan(M);
    if (int rc = check_workspace(__func__, ws_bytes, p.ws_bytes)) return rc;
    if (M == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    launch_persistent(lanes16 ? &pair_rowsums_kernel<true> : &pair_rowsums_kernel<false>, st, p.nwg, 0, rows, M, nwords, ldr, last_word_mask(nbits, lanes16),
                      weights, (int)nbits, p.nblk, p.S, (ulonglong2*)ws);
    TN_CHECK_LAUNCH("pair_rowsums_kernel");
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(pair_rowsums_reduce_kernel, dim3((unsigned)cdiv(M * 6, 256)), dim3(256), 0, st,
                                                     (const unsigned long long*)ws, p.S, M * 6, (unsigned long long*)out));
    TN_CHECK_LAUNCH("pair_rowsums_reduce_kernel");
    return 0;
}

}  // extern "C"
