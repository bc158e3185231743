// tn_state_linkage: the single-linkage tree of M packed rows (tnac4o.calculate_state_linkage).
//
// Rows in tn_pair_hist's layout; d(a, b) = popcount(a XOR b) (lanes16: the 16-bit lanes that differ), with fold d' = min(d, nbits - d).
// Edges are ordered by the strict total order key(a, b) = (d(a, b), min(a, b), max(a, b)); the tree is the unique minimum spanning tree
// of the complete graph on the rows under that order, its M - 1 edges reported in ascending key order.  The nearest other row of a is
// the b != a that minimises (d(a, b), b).
//
// Boruvka's algorithm in a fixed number of ceil(log2 M) rounds of ordinary launches on one stream; the host never waits.  A round:
//   1. linkage_pair_kernel: for every row a the minimum of (d(a, b), b) over the b of another component -- pair_hist_kernel's loop on
//      the tiles of the upper triangle (64 x 64 row blocks, chunks of 16 words in LDS, 4 x 4 distances per thread), with a min where
//      the histogram is, on both sides: a distance is offered to its row a and to its row b; the threads that share a row reduce by
//      shuffles and offer the minimum to row_best[row] with a 64-bit atomicMin (read first: most offers lose).
//      linkage_reduce_kernel feeds the row's minimum, as the 64-bit key d:16 | lo:24 | hi:24, to an atomicMin on the best edge of
//      the row's component.  In round 1 every row is a component of its own, so the row minima are the nearest other rows.
//   2. linkage_hook_kernel: every component hooks onto the component at the other end of its best edge (a mutual pair keeps the
//      smaller label as the root) and appends that edge once (a mutual pair from the smaller label); linkage_jump_kernel follows the
//      parents, eight steps per launch, ceil(log8 M) launches reach every root; linkage_relabel_kernel renames the rows.
// Under a strict total order the best edges of the components form no cycle but the mutual pairs, so the hooks are a forest.  A round
// at least halves the components: ceil(log2 M) rounds suffice.  Once M - 1 edges are there (a device counter) the kernels of the
// rounds that are left return at once.  No kernel waits for another workgroup; no floating point; the only atomics are the two
// atomicMin above (a minimum does not depend on the order of its operands) and the counter of the edges.  The order in which the edges
// are appended depends on the run, the set does not: the keys are sorted (rocPRIM's radix sort, as beamsearch.hip) and unpacked.  Every
// result is a function of the inputs alone.
//
// stage_block, pair_dist and last_word_mask are second copies of overlap.hip's, tri_decode is its order in integers: overlap.hip stays
// as it is.
#include "common.h"

#include <algorithm>
#include <rocprim/rocprim.hpp>

namespace tn {

namespace {

constexpr int LK_TILE = 64;                      // rows per block of a tile
constexpr int LK_CW = 16;                        // words of a row per chunk
constexpr int LK_PITCH = LK_TILE + 2;            // words between two chunk words in LDS (16-byte aligned, spreads the staging stores)
constexpr int LK_MAX_WGS = 4096;
constexpr int64_t LK_MAX_M = (int64_t)1 << 24;   // a row index takes 24 bits of the key
constexpr int64_t LK_MAX_NBITS = 65534;          // a distance takes 16 bits of the key, and the key of all ones is "none"
constexpr int LK_HOPS = 8;                       // parents followed per launch of linkage_jump_kernel
constexpr unsigned long long LK_NONE = ~0ull;

template <bool LANES16>
__device__ __forceinline__ unsigned pair_dist(uint64_t a, uint64_t b) {
    const uint64_t x = a ^ b;
    if (!LANES16) return (unsigned)__popcll(x);
    const uint64_t low = 0x7fff7fff7fff7fffull;  // bit 15 of a lane of t: some bit of that lane of x is set
    const uint64_t t = (((x & low) + low) | x) & ~low;
    return (unsigned)__popcll(t);
}

// mask of the last word of a row of nbits bits (lanes16: 16-bit lanes): what lies behind the row in that word is cut
inline uint64_t last_word_mask(int64_t nbits, int lanes16) {
    const int per = lanes16 ? 4 : 64, used = (int)(nbits - (cdiv(nbits, per) - 1) * per);
    return used == per ? ~(uint64_t)0 : (((uint64_t)1 << (used * (lanes16 ? 16 : 1))) - 1);
}

// rows [r0, r0 + 64) x words [k0, k0 + LK_CW) into dst[k * LK_PITCH + r]; rows >= M and words >= nwords read as 0 and are never
// addressed, the last word of a row is cut to nbits
__device__ __forceinline__ void stage_block(uint64_t* dst, const uint64_t* __restrict__ rows, int64_t M, int64_t ldr, int64_t r0, int64_t k0,
                                            int64_t nwords, uint64_t last_mask) {
    const int k = threadIdx.x & (LK_CW - 1);
    for (int r = threadIdx.x / LK_CW; r < LK_TILE; r += 256 / LK_CW) {
        const int64_t row = r0 + r, w = k0 + k;
        uint64_t v = 0;
        if (row < M && w < nwords) {
            v = rows[row * ldr + w];
            if (w == nwords - 1) v &= last_mask;
        }
        dst[k * LK_PITCH + r] = v;
    }
}

__device__ __forceinline__ unsigned long long umin64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// the key of the edge {a, b} at distance d
__device__ __forceinline__ unsigned long long edge_key(unsigned d, unsigned a, unsigned b) {
    return ((unsigned long long)d << 48) | ((unsigned long long)min(a, b) << 24) | (unsigned long long)max(a, b);
}

// the scalars of a call on the device
struct LinkageFlags {
    int32_t edges;                               // edges appended so far; M - 1: one component is left
    int32_t done;                                // set by linkage_reduce_kernel, read by linkage_hook_kernel (which moves `edges`)
};

// comp[a] = a, no best edge; no edge yet, no round; M = 1: the row has no nearest other row
__global__ __launch_bounds__(256) void linkage_init_kernel(int64_t M, int32_t* __restrict__ comp, unsigned long long* __restrict__ comp_best,
                                                           unsigned long long* __restrict__ row_best, LinkageFlags* __restrict__ flags,
                                                           int32_t* __restrict__ rounds_out, int32_t* __restrict__ nn_index,
                                                           int32_t* __restrict__ nn_dist) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a == 0) {
        *rounds_out = 0;
        if (flags) {
            flags->edges = 0;
            flags->done = 0;
        }
        if (M == 1 && nn_index) {
            nn_index[0] = -1;
            nn_dist[0] = -1;
        }
    }
    if (a < M && comp) {
        comp[a] = (int32_t)a;
        comp_best[a] = LK_NONE;
        row_best[a] = LK_NONE;
    }
}

// tile t of the upper triangle of a matrix of blocks, column by column (overlap.hip's order, in integers): bj = the largest j with
// j (j + 1) / 2 <= t, bi = t - bj (bj + 1) / 2 <= bj
__device__ __forceinline__ void tri_decode(int64_t t, int64_t nblk, int64_t& bi, int64_t& bj) {
    int64_t lo = 0, hi = nblk;                                 // lo (lo + 1) / 2 <= t < hi (hi + 1) / 2
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (mid * (mid + 1) / 2 <= t) lo = mid;
        else hi = mid;
    }
    bj = lo;
    bi = t - bj * (bj + 1) / 2;
}

// row_best[r] = min(row_best[r], key); most keys lose against what is there already, and a stale read is a larger one: the atomic decides
__device__ __forceinline__ void offer(unsigned long long* __restrict__ slot, unsigned long long key) {
    if (key != LK_NONE && *slot > key) atomicMin(slot, key);
}

// ---- step 1: row_best[a] = min over the rows b with comp[b] != comp[a] of d(a, b) << 32 | b, for every row a.  The tiles of the upper
// triangle of the pair matrix (the diagonal ones included), as pair_hist_kernel walks them; workgroup g takes the tiles
// [g ntiles / G, (g + 1) ntiles / G).  A distance serves both of its rows: the thread's 4 x 4 distances go into four minima of its rows
// a (over b) and four of its rows b (over a); the 16 threads of a row a are 16 consecutive lanes, the threads of a row b are the
// lanes l, l + 16, l + 32, l + 48 of the four waves: shuffles reduce each within the wave, and the survivors are offered to row_best.
// A diagonal tile is computed in full, its row side holds both directions.  fold_n: nbits with fold, else -1
template <bool LANES16>
__global__ __launch_bounds__(256) void linkage_pair_kernel(const uint64_t* __restrict__ rows, int64_t M, int64_t nwords, int64_t ldr, uint64_t last_mask,
                                                           int fold_n, const int32_t* __restrict__ comp, const LinkageFlags* __restrict__ flags,
                                                           int64_t nblk, int64_t ntiles, unsigned long long* __restrict__ row_best) {
    __shared__ uint64_t sA[LK_CW * LK_PITCH], sB[LK_CW * LK_PITCH];
    if (flags->edges >= M - 1) return;                         // (uniform: no launch of a round changes it but the hook)
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t t0 = (int64_t)blockIdx.x * ntiles / gridDim.x, t1 = ((int64_t)blockIdx.x + 1) * ntiles / gridDim.x;
    if (t0 >= t1) return;
    int64_t bi, bj;
    tri_decode(t0, nblk, bi, bj);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t a0 = bi * LK_TILE, b0 = bj * LK_TILE;
        const bool diag = bi == bj;
        int ca[4], cb[4];                                      // -1 for a row past the end
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t ra = a0 + ty * 4 + i, rb = b0 + tx * 4 + i;
            ca[i] = ra < M ? comp[ra] : -1;
            cb[i] = rb < M ? comp[rb] : -1;
        }
        unsigned dist[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) dist[i][j] = 0;
        for (int64_t k0 = 0; k0 < nwords; k0 += LK_CW) {
            __syncthreads();                                   // the previous chunk has been read
            stage_block(sA, rows, M, ldr, a0, k0, nwords, last_mask);
            stage_block(sB, rows, M, ldr, b0, k0, nwords, last_mask);
            __syncthreads();
#pragma unroll
            for (int k = 0; k < LK_CW; ++k) {
                uint64_t a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[i] = sA[k * LK_PITCH + ty * 4 + i];
                    b[i] = sB[k * LK_PITCH + tx * 4 + i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) dist[i][j] += pair_dist<LANES16>(a[i], b[j]);
            }
        }
        unsigned long long best_a[4], best_b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) best_a[i] = best_b[i] = LK_NONE;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned d = dist[i][j];
                if (fold_n >= 0) d = min(d, (unsigned)fold_n - d);
                if ((ca[i] | cb[j]) >= 0 && ca[i] != cb[j]) {  // both rows exist, in two components
                    best_a[i] = umin64(best_a[i], ((unsigned long long)d << 32) | (unsigned)(b0 + tx * 4 + j));
                    best_b[j] = umin64(best_b[j], ((unsigned long long)d << 32) | (unsigned)(a0 + ty * 4 + i));
                }
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) best_a[i] = umin64(best_a[i], __shfl_xor(best_a[i], o, 64));
            if (tx == 0 && ca[i] >= 0) offer(&row_best[a0 + ty * 4 + i], best_a[i]);
        }
        if (!diag) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int o = 32; o >= 16; o >>= 1) best_b[j] = umin64(best_b[j], __shfl_xor(best_b[j], o, 64));
                if ((ty & 3) == 0 && cb[j] >= 0) offer(&row_best[b0 + tx * 4 + j], best_b[j]);
            }
        }
        if (++bi > bj) {
            bi = 0;
            ++bj;
        }
    }
}

// row_best of row a (taken, and cleared for the next round): the nearest other row in round 1 (nn_index given), and the candidate of
// the row's component
__global__ __launch_bounds__(256) void linkage_reduce_kernel(int64_t M, unsigned long long* __restrict__ row_best, const int32_t* __restrict__ comp,
                                                             unsigned long long* __restrict__ comp_best, LinkageFlags* __restrict__ flags,
                                                             int32_t* __restrict__ rounds_out, int32_t* __restrict__ nn_index,
                                                             int32_t* __restrict__ nn_dist) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (flags->edges >= M - 1) {
        if (a == 0) flags->done = 1;
        return;
    }
    if (a == 0) *rounds_out += 1;
    if (a >= M) return;
    const unsigned long long k = row_best[a];
    row_best[a] = LK_NONE;
    if (k == LK_NONE) return;                                  // (more than one component is left: every row sees another one)
    const unsigned b = (unsigned)(k & 0xffffffffu), d = (unsigned)(k >> 32);
    if (nn_index) {
        nn_index[a] = (int32_t)b;
        nn_dist[a] = (int32_t)d;
    }
    const unsigned long long key = edge_key(d, (unsigned)a, b);
    unsigned long long* slot = &comp_best[comp[a]];
    if (*slot > key) atomicMin(slot, key);                     // (a stale read is a larger one: the atomic decides)
}

// ---- step 2: parent[] of every row; a root hooks onto the component at the other end of its best edge and appends the edge
__global__ __launch_bounds__(256) void linkage_hook_kernel(int64_t M, const int32_t* __restrict__ comp, const unsigned long long* __restrict__ comp_best,
                                                           int32_t* __restrict__ parent, LinkageFlags* __restrict__ flags,
                                                           unsigned long long* __restrict__ edges) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (flags->done || c >= M) return;
    int32_t p = comp[c];
    if (p == c) {
        const unsigned long long key = comp_best[c];
        const int64_t lo = (int64_t)((key >> 24) & 0xffffffu), hi = (int64_t)(key & 0xffffffu);
        if (key != LK_NONE && lo < M && hi < M) {
            const int32_t cl = comp[lo], oc = cl == c ? comp[hi] : cl;
            const bool mutual = comp_best[oc] == key;
            if (!mutual || c > oc) p = oc;
            if (!mutual || c < oc) {
                const int32_t at = atomicAdd(&flags->edges, 1);
                if (at < M - 1) edges[at] = key;
            }
        }
    }
    parent[c] = p;
}

// parent[a] = the ancestor LK_HOPS + 1 steps up (or the root); in place: another thread's newer entry is an ancestor too
__global__ __launch_bounds__(256) void linkage_jump_kernel(int64_t M, int32_t* __restrict__ parent, const LinkageFlags* __restrict__ flags) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (flags->done || a >= M) return;
    int32_t p = parent[a];
#pragma unroll 1
    for (int h = 0; h < LK_HOPS; ++h) {
        const int32_t q = parent[p];
        if (q == p) break;
        p = q;
    }
    parent[a] = p;
}

__global__ __launch_bounds__(256) void linkage_relabel_kernel(int64_t M, const int32_t* __restrict__ parent, int32_t* __restrict__ comp,
                                                              unsigned long long* __restrict__ comp_best, const LinkageFlags* __restrict__ flags) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (flags->done || a >= M) return;
    comp[a] = parent[a];
    comp_best[a] = LK_NONE;
}

// ---- step 3: the sorted keys as (lo, hi, d)
__global__ __launch_bounds__(256) void linkage_unpack_kernel(int64_t n, const unsigned long long* __restrict__ keys, int32_t* __restrict__ edge_lo,
                                                             int32_t* __restrict__ edge_hi, int32_t* __restrict__ edge_dist) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const unsigned long long k = keys[e];
    edge_lo[e] = (int32_t)((k >> 24) & 0xffffffu);
    edge_hi[e] = (int32_t)(k & 0xffffffu);
    edge_dist[e] = (int32_t)(k >> 48);
}

inline int64_t linkage_nwords(int64_t nbits, int lanes16) { return lanes16 ? cdiv(nbits, 4) : cdiv(nbits, 64); }
inline bool linkage_shape_ok(int64_t M, int64_t nbits) { return M >= 0 && M <= LK_MAX_M && nbits >= 1 && nbits <= LK_MAX_NBITS; }
inline int linkage_rounds(int64_t M) {
    int r = 0;
    while (((int64_t)1 << r) < M) ++r;
    return r;
}

struct LinkageWs {
    LinkageFlags* flags;
    int32_t* comp;
    int32_t* parent;
    unsigned long long* comp_best;
    unsigned long long* row_best;
    unsigned long long* edges;
    unsigned long long* sorted;
    char* sort_tmp;
    size_t sort_bytes;
    int64_t nblk, ntiles, nwg, bytes;
};

// The workspace of a call and the grid of its pair pass: TN_LINKAGE_WGS (read per call) or 4 workgroups on each of the 256 compute
// units (90 VGPRs and 16.5 KiB of LDS admit 5), never more than there are tiles; every workgroup takes an equal share of the tiles.
LinkageWs linkage_layout(void* ws, int64_t M) {
    WsCarve w{(char*)ws};
    LinkageWs s{};
    const int64_t asked = env_i64("TN_LINKAGE_WGS", 0), G = std::min<int64_t>(asked > 0 ? asked : 256 * 4, LK_MAX_WGS);
    s.nblk = cdiv(M, LK_TILE);
    s.ntiles = s.nblk * (s.nblk + 1) / 2;
    s.nwg = std::max<int64_t>(1, std::min<int64_t>(G, s.ntiles));
    if (M >= 2) {
        s.flags = w.take<LinkageFlags>(sizeof(LinkageFlags));
        s.comp = w.take<int32_t>(M * 4);
        s.parent = w.take<int32_t>(M * 4);
        s.comp_best = w.take<unsigned long long>(M * 8);
        s.row_best = w.take<unsigned long long>(M * 8);
        s.edges = w.take<unsigned long long>((M - 1) * 8);
        s.sorted = w.take<unsigned long long>((M - 1) * 8);
        (void)rocprim::radix_sort_keys(nullptr, s.sort_bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)(M - 1), 0, 64,
                                       (hipStream_t) nullptr);
        s.sort_tmp = w.take<char>((int64_t)s.sort_bytes);
    }
    s.bytes = w.total();
    return s;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int64_t tn_state_linkage_ws_bytes(int64_t M, int64_t nbits, int lanes16) {
    (void)lanes16;
    if (!linkage_shape_ok(M, nbits)) return 0;
    return linkage_layout(nullptr, M).bytes;
}

int tn_state_linkage(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, int lanes16, int fold, int32_t* nn_index, int32_t* nn_dist,
                     int32_t* edge_lo, int32_t* edge_hi, int32_t* edge_dist, int32_t* rounds_out, void* ws, int64_t ws_bytes, void* stream) {
    if (M < 0 || M > LK_MAX_M) {
        set_error("tn_state_linkage: M = %lld outside 0 .. 2^24 = %lld (a row index takes 24 bits of an edge's key)", (long long)M, (long long)LK_MAX_M);
        return -1;
    }
    if (nbits < 1 || nbits > LK_MAX_NBITS) {
        set_error("tn_state_linkage: nbits = %lld outside 1 .. %lld (a distance takes 16 bits of an edge's key)", (long long)nbits,
                  (long long)LK_MAX_NBITS);
        return -1;
    }
    TN_CHECK_ARG(!(fold && lanes16), "fold is defined for bits only (lanes16 = 0)");
    const int64_t nwords = linkage_nwords(nbits, lanes16);
    TN_CHECK_ARG(ldr >= nwords, "ldr shorter than a row");
    TN_CHECK_ARG(rounds_out && (M == 0 || rows) && (M < 2 || (edge_lo && edge_hi && edge_dist)), "null operand");
    TN_CHECK_ARG((nn_index == nullptr) == (nn_dist == nullptr), "nn_index and nn_dist: both or neither");
    const LinkageWs w = linkage_layout(ws, M);
    if (ws_bytes < w.bytes) {
        set_error("tn_state_linkage: workspace too small (%lld bytes, tn_state_linkage_ws_bytes asks for %lld)", (long long)ws_bytes, (long long)w.bytes);
        return -3;
    }
    TN_CHECK_ARG(w.bytes == 0 || (ws && ((uintptr_t)ws & 255) == 0), "ws null or not aligned to 256 bytes");
    hipStream_t st = (hipStream_t)stream;
    const unsigned mblk = (unsigned)std::max<int64_t>(cdiv(M, 256), 1);
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(linkage_init_kernel, dim3(mblk), dim3(256), 0, st, M, w.comp, w.comp_best, w.row_best, w.flags, rounds_out,
                                                     nn_index, nn_dist));
    TN_CHECK_LAUNCH("linkage_init_kernel");
    if (M < 2) return 0;
    const uint64_t last_mask = last_word_mask(nbits, lanes16);
    const int fold_n = fold ? (int)nbits : -1;
    const int R = linkage_rounds(M), J = (R + 2) / 3;         // 8^J >= M: the deepest forest of hooks is flat after J launches
    for (int r = 0; r < R; ++r) {
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(lanes16 ? &linkage_pair_kernel<true> : &linkage_pair_kernel<false>, dim3((unsigned)w.nwg), dim3(256),
                                                         0, st, rows, M, nwords, ldr, last_mask, fold_n, w.comp, w.flags, w.nblk, w.ntiles, w.row_best));
        TN_CHECK_LAUNCH("linkage_pair_kernel");
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(linkage_reduce_kernel, dim3(mblk), dim3(256), 0, st, M, w.row_best, w.comp, w.comp_best,
                                                         w.flags, rounds_out, r == 0 ? nn_index : nullptr, r == 0 ? nn_dist : nullptr));
        TN_CHECK_LAUNCH("linkage_reduce_kernel");
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(linkage_hook_kernel, dim3(mblk), dim3(256), 0, st, M, w.comp, w.comp_best, w.parent, w.flags,
                                                         w.edges));
        TN_CHECK_LAUNCH("linkage_hook_kernel");
        for (int j = 0; j < J; ++j) {
            TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(linkage_jump_kernel, dim3(mblk), dim3(256), 0, st, M, w.parent, w.flags));
            TN_CHECK_LAUNCH("linkage_jump_kernel");
        }
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(linkage_relabel_kernel, dim3(mblk), dim3(256), 0, st, M, w.parent, w.comp, w.comp_best, w.flags));
        TN_CHECK_LAUNCH("linkage_relabel_kernel");
    }
    size_t sort_bytes = w.sort_bytes;
    const hipError_t e = rocprim::radix_sort_keys(w.sort_tmp, sort_bytes, (const unsigned long long*)w.edges, w.sorted, (size_t)(M - 1), 0, 64, st);
    if (e != hipSuccess) return hip_fail(e, "tn_state_linkage: sort of the edges");
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(linkage_unpack_kernel, dim3((unsigned)cdiv(M - 1, 256)), dim3(256), 0, st, M - 1, w.sorted, edge_lo,
                                                     edge_hi, edge_dist));
    TN_CHECK_LAUNCH("linkage_unpack_kernel");
    return 0;
}

}  // extern "C"
