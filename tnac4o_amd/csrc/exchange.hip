// tn_cluster_exchange: one round of isoenergetic cluster moves (Houdayer's move in its form for arbitrary graphs) over P disjoint pairs
// of bit-packed rows, in place (tnac4o.exchange_clusters).  For a pair (a, b): D = row_a XOR row_b, the seed is the r-th set bit of D,
// C = what the seed reaches along the arcs of a CSR graph through bits of D, and both rows are XORed with C.
//
// C is grown from the seed by passes over a FRONTIER, all of it in bitmasks: V (reached so far) lives in LDS, every lane keeps P = the
// value of its words of V it has already expanded.  In a pass a lane reads its words of V, takes the new bits F = V & ~P as its
// frontier, sets P = V, and for every bit of F walks the arcs of that bit: a neighbour j that lies in D is ORed into V with an LDS
// atomic.  A bit enters a frontier exactly once, whenever in a pass its OR lands, so the arcs of C are walked once in all; the passes
// end when NO lane found a frontier bit, which is decided on a value every lane agrees on (a ballot of the wave, or the OR that the
// workgroup barrier returns) and only after every OR of the previous pass is visible (a wave's LDS operations complete in order and
// are waited for before the next read; the workgroup form has a barrier between two passes).  An empty frontier everywhere means that
// nothing was ORed since the last look: V is the fixed point, the same set for every schedule.  The passes are bounded by nbits by
// construction: every pass but the last adds at least one bit.
//
// Two forms.  nbits <= 4096 (EX_WAVE_BITS): one WAVE per pair, one 64-bit word of D, V and P per lane, four pairs per workgroup of 256
// threads and no workgroup barrier at all (the waves of a workgroup run different numbers of passes).  Above: one WORKGROUP per
// pair, up to four words per thread, the same loop with __syncthreads_or.  The CSR stays in global memory: it is shared by all
// pairs and lives in L2.  Nothing read from rowptr, cols or pairs is used as an index unchecked.
#include "common.h"
#include "sweep.h"

namespace tn {

namespace {

constexpr int64_t EX_MAX_NBITS = 65534;          // the largest row (tn_spin_moments' limit: the rows are the same)
constexpr int EX_WAVE_BITS = 4096;               // the largest row of the one-wave form: one word per lane
constexpr int EX_WAVES = 4;                      // pairs per workgroup of the one-wave form
constexpr int EX_WPT = 4;                        // words per thread of the workgroup form: 256 * 4 * 64 = 65536 bits
constexpr int EX_MAX_WORDS = 256 * EX_WPT;

// the k-th set bit of w (k below its popcount), ascending
__device__ __forceinline__ int nth_set_bit(uint64_t w, int k) {
    for (int i = 0; i < k; ++i) w &= w - 1;
    return __ffsll((unsigned long long)w) - 1;
}

// r = min(floor(u cnt), cnt - 1): one IEEE multiplication and a floor; whatever is not a number in [0, 1) still gives an r in [0, cnt)
__device__ __forceinline__ int seed_rank(double u, int cnt) {
    const double x = u * (double)cnt;
    if (x >= (double)cnt) return cnt - 1;
    return x >= 0.0 ? min((int)x, cnt - 1) : 0;
}

// the arcs of the frontier bits `f` of word w: every neighbour inside [0, nbits) that is a bit of D joins V
__device__ __forceinline__ void expand(uint64_t f, int w, const uint64_t* Dl, unsigned long long* Vl, const int32_t* __restrict__ rowptr,
                                       const int32_t* __restrict__ cols, int nnz, int nbits) {
    while (f) {
        const int i = w * 64 + (__ffsll((unsigned long long)f) - 1);
        f &= f - 1;
        const int beg = max(rowptr[i], 0), end = min(rowptr[i + 1], nnz);           // (i < nbits: rowptr has nbits + 1 entries)
        for (int e = beg; e < end; ++e) {
            const int j = cols[e];
            if (j < 0 || j >= nbits) continue;
            const uint64_t bit = (uint64_t)1 << (j & 63);
            if (Dl[j >> 6] & bit) __hip_atomic_fetch_or(&Vl[j >> 6], (unsigned long long)bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// a pair's row indices; false (and -1 in both outputs) when one lies outside [0, M)
__device__ __forceinline__ bool pair_rows(const int32_t* __restrict__ pairs, int64_t p, int64_t M, int64_t& a, int64_t& b) {
    a = pairs[2 * p];
    b = pairs[2 * p + 1];
    return a >= 0 && a < M && b >= 0 && b < M;
}

// ---- one wave per pair ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * EX_WAVES) exchange_wave_kernel(uint64_t* __restrict__ rows, int64_t M, int nbits, int nwords, int64_t ldr,
                                                                      uint64_t last_mask, const int32_t* __restrict__ rowptr,
                                                                      const int32_t* __restrict__ cols, int nnz, const int32_t* __restrict__ pairs,
                                                                      int64_t P, const double* __restrict__ uniforms, int32_t* __restrict__ size_out,
                                                                      int32_t* __restrict__ diff_out) {
    __shared__ uint64_t Ds[EX_WAVES][64];
    __shared__ unsigned long long Vs[EX_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * EX_WAVES + wave;
    if (p >= P) return;                                                  // (wave-uniform; no workgroup barrier below)
    int64_t a, b;
    if (!pair_rows(pairs, p, M, a, b)) {
        if (lane == 0) size_out[p] = diff_out[p] = -1;
        return;
    }
    const bool mine = lane < nwords;
    uint64_t ra = 0, rb = 0;
    if (mine) {
        ra = rows[a * ldr + lane];
        rb = rows[b * ldr + lane];
    }
    const uint64_t d = (ra ^ rb) & (lane == nwords - 1 ? last_mask : ~(uint64_t)0);
    // the seed: the r-th set bit of D, from the popcounts before this lane
    const int c = __popcll(d);
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const int cnt = __shfl(incl, 63, 64);
    if (cnt == 0) {                                                      // (a == b ends here too)
        if (lane == 0) { size_out[p] = 0; diff_out[p] = 0; }
        return;
    }
    const int r = seed_rank(uniforms[p], cnt);
    const int before = incl - c;
    uint64_t* Dl = Ds[wave];
    unsigned long long* Vl = Vs[wave];
    Dl[lane] = d;
    Vl[lane] = (r >= before && r < incl) ? (unsigned long long)1 << nth_set_bit(d, r - before) : 0ull;
    uint64_t prev = 0;
    for (int pass = 0; pass < nbits; ++pass) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");          // the wave's LDS writes and ORs so far have landed
        __builtin_amdgcn_wave_barrier();
        const uint64_t v = __hip_atomic_load(&Vl[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const uint64_t f = v & ~prev;
        prev = v;
        if (__ballot(f != 0) == 0) break;                               // no frontier in any lane: V is the fixed point
        expand(f, lane, Dl, Vl, rowptr, cols, nnz, nbits);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const uint64_t cl = __hip_atomic_load(&Vl[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (mine && cl) {
        rows[a * ldr + lane] = ra ^ cl;
        rows[b * ldr + lane] = rb ^ cl;
    }
    int sz = __popcll(cl);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sz += __shfl_xor(sz, o, 64);
    if (lane == 0) { size_out[p] = sz; diff_out[p] = cnt; }
}

// ---- one workgroup per pair ----------------------------------------------------------------------------------------------------
// thread t owns the words t, t + 256, ... (at most EX_WPT); red: the popcounts of the four waves
__global__ void __launch_bounds__(256) exchange_block_kernel(uint64_t* __restrict__ rows, int64_t M, int nbits, int nwords, int64_t ldr, uint64_t last_mask,
                                                             const int32_t* __restrict__ rowptr, const int32_t* __restrict__ cols, int nnz,
                                                             const int32_t* __restrict__ pairs, int64_t P, const double* __restrict__ uniforms,
                                                             int32_t* __restrict__ size_out, int32_t* __restrict__ diff_out) {
    __shared__ uint64_t Dl[EX_MAX_WORDS];
    __shared__ unsigned long long Vl[EX_MAX_WORDS];
    __shared__ int cum[EX_MAX_WORDS];                                    // set bits of D up to and including a word
    __shared__ int red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p = blockIdx.x;
    int64_t a, b;
    if (!pair_rows(pairs, p, M, a, b)) {                                 // (uniform over the workgroup, as every exit below)
        if (tid == 0) size_out[p] = diff_out[p] = -1;
        return;
    }
    uint64_t ra[EX_WPT], rb[EX_WPT], prev[EX_WPT];
#pragma unroll
    for (int k = 0; k < EX_WPT; ++k) {
        const int w = tid + 256 * k;
        ra[k] = rb[k] = prev[k] = 0;
        if (w < nwords) {
            ra[k] = rows[a * ldr + w];
            rb[k] = rows[b * ldr + w];
            Dl[w] = (ra[k] ^ rb[k]) & (w == nwords - 1 ? last_mask : ~(uint64_t)0);
            Vl[w] = 0;
        }
    }
    __syncthreads();
    // the seed: thread t scans the words [t wps, (t + 1) wps), the waves and the workgroup add up through shuffles and LDS
    const int wps = (nwords + 255) / 256, w0 = tid * wps, w1 = min(w0 + wps, nwords);
    int c = 0;
    for (int w = w0; w < w1; ++w) {
        c += __popcll(Dl[w]);
        cum[w] = c;
    }
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    int before = incl - c;
    for (int k = 0; k < wave; ++k) before += red[k];
    const int cnt = red[0] + red[1] + red[2] + red[3];
    if (cnt == 0) {
        if (tid == 0) { size_out[p] = 0; diff_out[p] = 0; }
        return;
    }
    const int r = seed_rank(uniforms[p], cnt);
    for (int w = w0; w < w1; ++w) {
        const int lo = before + cum[w] - __popcll(Dl[w]);                // set bits before word w
        if (r >= lo && r < before + cum[w]) Vl[w] = (unsigned long long)1 << nth_set_bit(Dl[w], r - lo);
    }
    __syncthreads();
    for (int pass = 0; pass < nbits; ++pass) {
        uint64_t f[EX_WPT];
        bool any = false;
#pragma unroll
        for (int k = 0; k < EX_WPT; ++k) {
            const int w = tid + 256 * k;
            f[k] = 0;
            if (w < nwords) {
                const uint64_t v = __hip_atomic_load(&Vl[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                f[k] = v & ~prev[k];
                prev[k] = v;
                any |= f[k] != 0;
            }
        }
#pragma unroll
        for (int k = 0; k < EX_WPT; ++k) expand(f[k], tid + 256 * k, Dl, Vl, rowptr, cols, nnz, nbits);
        if (!__syncthreads_or(any)) break;                               // no frontier in any thread: nothing was ORed in this pass
    }
    __syncthreads();
    int sz = 0;
#pragma unroll
    for (int k = 0; k < EX_WPT; ++k) {
        const int w = tid + 256 * k;
        if (w < nwords) {
            const uint64_t cl = Vl[w];
            sz += __popcll(cl);
            if (cl) {
                rows[a * ldr + w] = ra[k] ^ cl;
                rows[b * ldr + w] = rb[k] ^ cl;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sz += __shfl_xor(sz, o, 64);
    __syncthreads();                                                     // (red is read above by every thread)
    if (lane == 0) red[wave] = sz;
    __syncthreads();
    if (tid == 0) { size_out[p] = red[0] + red[1] + red[2] + red[3]; diff_out[p] = cnt; }
}

}  // namespace

int64_t cluster_exchange_max_nbits() { return EX_MAX_NBITS; }

// the launch of a round (sweep.h): tn_cluster_exchange below and tn_temper, which has checked the same limits
int cluster_exchange_launch(hipStream_t st, uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const int32_t* rowptr, const int32_t* cols,
                            int64_t nnz, const int32_t* pairs, int64_t P, const double* uniforms, int32_t* size_out, int32_t* diff_out) {
    const int64_t nwords = cdiv(nbits, 64);
    const int used = (int)(nbits - (nwords - 1) * 64);
    const uint64_t last_mask = used == 64 ? ~(uint64_t)0 : (((uint64_t)1 << used) - 1);
    if (nbits <= EX_WAVE_BITS) {
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(exchange_wave_kernel, dim3((unsigned)cdiv(P, EX_WAVES)), dim3(64 * EX_WAVES), 0, st, rows, M,
                                                         (int)nbits, (int)nwords, ldr, last_mask, rowptr, cols, (int)nnz, pairs, P, uniforms, size_out,
                                                         diff_out));
        TN_CHECK_LAUNCH("exchange_wave_kernel");
    } else {
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(exchange_block_kernel, dim3((unsigned)P), dim3(256), 0, st, rows, M, (int)nbits, (int)nwords, ldr,
                                                         last_mask, rowptr, cols, (int)nnz, pairs, P, uniforms, size_out, diff_out));
        TN_CHECK_LAUNCH("exchange_block_kernel");
    }
    return 0;
}

}  // namespace tn

using namespace tn;

extern "C" {

int tn_cluster_exchange(uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const int32_t* rowptr, const int32_t* cols, int64_t nnz,
                        const int32_t* pairs, int64_t P, const double* uniforms, int32_t* size_out, int32_t* diff_out, void* stream) {
    const int64_t two31 = (int64_t)1 << 31;
    TN_CHECK_ARG(M >= 0 && M < two31, "M negative or not below 2^31");
    if (nbits < 1 || nbits > EX_MAX_NBITS) {
        set_error("tn_cluster_exchange: nbits = %lld outside 1 .. %lld", (long long)nbits, (long long)EX_MAX_NBITS);
        return -1;
    }
    TN_CHECK_ARG(nnz >= 0 && nnz < two31, "nnz negative or not below 2^31");
    TN_CHECK_ARG(P >= 0, "P negative");
    TN_CHECK_ARG(P < two31, "P not below 2^31 (disjoint pairs of fewer than 2^31 rows)");
    const int64_t nwords = cdiv(nbits, 64);
    TN_CHECK_ARG(ldr >= nwords, "ldr shorter than a row of ceil(nbits / 64) words");
    if (P == 0) return 0;
    TN_CHECK_ARG(rows && rowptr && pairs && uniforms && size_out && diff_out && (cols || nnz == 0), "null operand");
    return cluster_exchange_launch((hipStream_t)stream, rows, M, nbits, ldr, rowptr, cols, nnz, pairs, P, uniforms, size_out, diff_out);
}

}  // extern "C"
