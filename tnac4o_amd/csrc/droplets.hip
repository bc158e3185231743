// tn_droplets: the droplets of M bit-packed rows relative to a reference row (tnac4o.calculate_droplets).  For a row x: D = x XOR ref,
// the droplets are the connected components of the subgraph that D induces on a CSR graph over the bits, numbered by ascending root
// (the smallest bit of a droplet), each with its size and its excitation energy
//     dE_C = E(ref with C flipped) - E(ref) = -2 (sum_{i in C, j not in C} J_ij g_i g_j + sum_{i in C} h_i g_i),  g = 2 ref - 1.
//
// ONE WALK of the arcs serves both: a neighbour j of a droplet bit that lies in D belongs to the droplet, so every arc that leaves the
// droplet ends outside D.  When the arcs of a frontier bit i are walked, a neighbour in D is ORed into V (the growth of exchange.hip),
// a neighbour outside D adds its term -J_ij g_i g_j to the walking thread's sum; the field term of i goes in front of its arcs.
//
// The droplets of a row are grown one after the other: the seed is the lowest bit of D that no finished droplet holds, so the roots
// ascend by construction.  The growth is the frontier search of exchange.hip (V in LDS, P = what a thread has expanded of its words,
// F = V & ~P; the end is an empty frontier everywhere), with ONE difference that makes the floating-point sums a function of the
// inputs alone: every thread has read its frontier of a pass before any thread ORs in that pass (the wave form: the ballot sits
// between the read and the walk; the workgroup form: the barrier that decides the exit sits there, a second one ends the pass).  The
// frontier of pass p is then the p-th level of the breadth-first search from the root, and a thread adds its terms in the order
// (level, bit ascending, field, arcs as listed); the threads' sums are added in a fixed tree.  No sum depends on the grid, on M or on
// the schedule.  Terms are vals[e] * (+-1): for exactly summable couplings the energies are exact.
//
// A CSR with one-way arcs can lead from a later root into a bit that an earlier droplet holds; such a bit is ORed into V like any bit
// of D and dropped by its owner (the read of V is masked with what is left of D): it neither joins again nor adds a term.  The
// droplets are a partition of D for every CSR.
//
// Two forms, as exchange.hip.  nbits <= 4096: one WAVE per row, one word per lane, four rows per workgroup, no workgroup barrier.
// Above: one WORKGROUP per row, up to four words per thread.  expand_droplet below is a second copy of exchange.hip's expand with the
// energy terms in it: exchange.hip stays as it is.  Nothing read from rowptr, cols or rows is used as an index unchecked.
#include "common.h"
#include "sweep.h"

namespace tn {

namespace {

constexpr int DR_WAVE_BITS = 4096;               // the largest row of the one-wave form: one word per lane
constexpr int DR_WAVES = 4;                      // rows per workgroup of the one-wave form
constexpr int DR_WPT = 4;                        // words per thread of the workgroup form: 256 * 4 * 64 = 65536 bits
constexpr int DR_MAX_WORDS = 256 * DR_WPT;
constexpr int DR_NONE = 0x7fffffff;              // "no bit left" in the search of the next root

struct DropletGraph {                            // the CSR with its couplings and the fields (device pointers; field may be null)
    const int32_t* rowptr;
    const int32_t* cols;
    const double* vals;
    const double* field;
    int nnz, nbits;
};

struct DropletOut {                              // the outputs (device pointers; labels may be null)
    int32_t* count;
    int32_t* diff;
    int32_t* largest;
    double* de_total;
    int32_t* root;
    int32_t* size;
    double* de;
    unsigned long long* size_hist;
    int32_t* labels;
    int64_t ldl;
    int K;
};

// the arcs of the frontier bits `f` of word w: a neighbour inside [0, nbits) that is a bit of D joins V, one that is not adds
// -vals[e] g_i g_j to acc; the field of i adds -field[i] g_i
__device__ __forceinline__ void expand_droplet(uint64_t f, int w, const uint64_t* Dl, const uint64_t* Rl, unsigned long long* Vl, const DropletGraph& g,
                                               double& acc) {
    while (f) {
        const int b = __ffsll((unsigned long long)f) - 1;
        const int i = w * 64 + b;
        f &= f - 1;
        const uint64_t gi = (Rl[w] >> b) & 1;
        if (g.field) acc += gi ? -g.field[i] : g.field[i];
        const int beg = max(g.rowptr[i], 0), end = min(g.rowptr[i + 1], g.nnz);     // (i < nbits: rowptr has nbits + 1 entries)
        for (int e = beg; e < end; ++e) {
            const int j = g.cols[e];
            if (j < 0 || j >= g.nbits) continue;
            const uint64_t bit = (uint64_t)1 << (j & 63);
            if (Dl[j >> 6] & bit) {
                __hip_atomic_fetch_or(&Vl[j >> 6], (unsigned long long)bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                const uint64_t gj = (Rl[j >> 6] >> (j & 63)) & 1;
                acc += gi == gj ? -g.vals[e] : g.vals[e];
            }
        }
    }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {                   // a fixed tree: the same bits in every lane
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// what one thread (lane 0 of the wave, thread 0 of the workgroup) keeps of a row while its droplets are emitted
struct RowTotals {
    int count = 0, largest = 0;
    double de_total = 0.0;
    __device__ __forceinline__ void emit(const DropletOut& o, int64_t m, int root, int size, double de) {
        if (count < o.K) {
            o.root[m * o.K + count] = root;
            o.size[m * o.K + count] = size;
            o.de[m * o.K + count] = de;
        }
        ++count;
        largest = max(largest, size);
        de_total += de;
    }
    __device__ __forceinline__ void finish(const DropletOut& o, int64_t m, int diff) const {
        o.count[m] = count;
        o.diff[m] = diff;
        o.largest[m] = largest;
        o.de_total[m] = de_total;
    }
};

// ---- one wave per row -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * DR_WAVES) droplets_wave_kernel(const uint64_t* __restrict__ rows, int64_t M, int nwords, int64_t ldr,
                                                                      uint64_t last_mask, const uint64_t* __restrict__ ref, DropletGraph g,
                                                                      DropletOut o) {
    __shared__ uint64_t Ds[DR_WAVES][64];
    __shared__ uint64_t Rs[DR_WAVES][64];
    __shared__ unsigned long long Vs[DR_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m = (int64_t)blockIdx.x * DR_WAVES + wave;
    if (m >= M) return;                                                  // (wave-uniform; no workgroup barrier below)
    const uint64_t mask = lane < nwords ? (lane == nwords - 1 ? last_mask : ~(uint64_t)0) : 0;
    uint64_t x = 0, r = 0;
    if (lane < nwords) {
        x = rows[m * ldr + lane];
        r = ref[lane] & mask;
    }
    const uint64_t d = (x ^ r) & mask;
    uint64_t* Dl = Ds[wave];
    uint64_t* Rl = Rs[wave];
    unsigned long long* Vl = Vs[wave];
    Dl[lane] = d;
    Rl[lane] = r;
    const int cnt = wave_sum((int)__popcll(d));
    int32_t* lab = o.labels ? o.labels + m * o.ldl : nullptr;
    if (lab) {                                                           // -1 where the row equals the reference; the bits of D follow
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int w = 0; w < nwords; ++w) {
            const int i = w * 64 + lane;
            if (i < g.nbits && !((Dl[w] >> lane) & 1)) lab[i] = -1;
        }
    }
    RowTotals tot;
    int small = 0;                                                       // lane s: the droplets of size s so far, 1 <= s < 64
    uint64_t rem = d;                                                    // the bits of D in no finished droplet
    for (int k = 0; k < cnt; ++k) {
        const unsigned long long left = __ballot(rem != 0);
        if (left == 0) break;
        const int first = __ffsll(left) - 1;                             // the lowest lane with a bit left: the root is its lowest bit
        const int rbit = __shfl(__ffsll((unsigned long long)rem) - 1, first, 64);
        Vl[lane] = lane == first ? (unsigned long long)1 << rbit : 0ull;
        uint64_t prev = 0;
        double acc = 0.0;
        for (int pass = 0; pass <= g.nbits; ++pass) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // the wave's LDS writes and ORs so far have landed
            __builtin_amdgcn_wave_barrier();
            const uint64_t v = __hip_atomic_load(&Vl[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & rem;
            const uint64_t f = v & ~prev;
            prev = v;
            if (__ballot(f != 0) == 0) break;                           // no frontier in any lane: V is the fixed point
            expand_droplet(f, lane, Dl, Rl, Vl, g, acc);
        }
        const uint64_t cl = prev;                                        // (the last look found nothing new: prev is V)
        rem &= ~cl;
        const int size = wave_sum((int)__popcll(cl));
        const double de = 2.0 * wave_sum(acc);
        if (lab) {
            unsigned long long words = __ballot(cl != 0);
            while (words) {
                const int w = __ffsll(words) - 1;
                words &= words - 1;
                if ((__shfl((unsigned long long)cl, w, 64) >> lane) & 1) lab[w * 64 + lane] = k;
            }
        }
        if (size < 64) small += lane == size;
        else if (lane == 0) atomicAdd(&o.size_hist[size], 1ull);
        if (lane == 0) tot.emit(o, m, first * 64 + rbit, size, de);
    }
    if (small) atomicAdd(&o.size_hist[lane], (unsigned long long)small);
    const int count = __shfl(tot.count, 0, 64);
    if (lane == 0) tot.finish(o, m, cnt);
    for (int k = count + lane; k < o.K; k += 64) {
        o.root[m * o.K + k] = -1;
        o.size[m * o.K + k] = 0;
        o.de[m * o.K + k] = 0.0;
    }
}

// ---- one workgroup per row ------------------------------------------------------------------------------------------------------
// thread t owns the words t, t + 256, ... (at most DR_WPT)
__global__ void __launch_bounds__(256) droplets_block_kernel(const uint64_t* __restrict__ rows, int64_t M, int nwords, int64_t ldr, uint64_t last_mask,
                                                             const uint64_t* __restrict__ ref, DropletGraph g, DropletOut o) {
    __shared__ uint64_t Dl[DR_MAX_WORDS];
    __shared__ uint64_t Rl[DR_MAX_WORDS];
    __shared__ unsigned long long Vl[DR_MAX_WORDS];
    __shared__ int redi[4], reds[4];
    __shared__ double redd[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = blockIdx.x;
    uint64_t rem[DR_WPT], prev[DR_WPT];
    int c = 0;
#pragma unroll
    for (int q = 0; q < DR_WPT; ++q) {
        const int w = tid + 256 * q;
        rem[q] = 0;
        if (w < nwords) {
            const uint64_t mask = w == nwords - 1 ? last_mask : ~(uint64_t)0;
            const uint64_t r = ref[w] & mask;
            rem[q] = (rows[m * ldr + w] ^ r) & mask;
            Dl[w] = rem[q];
            Rl[w] = r;
            c += __popcll(rem[q]);
        }
    }
    c = wave_sum(c);
    if (lane == 0) reds[wave] = c;
    __syncthreads();
    const int cnt = reds[0] + reds[1] + reds[2] + reds[3];
    int32_t* lab = o.labels ? o.labels + m * o.ldl : nullptr;
    if (lab)
        for (int i = tid; i < g.nbits; i += 256)
            if (!((Dl[i >> 6] >> (i & 63)) & 1)) lab[i] = -1;
    RowTotals tot;
    int small = 0;                                                       // thread s: the droplets of size s so far, 1 <= s < 256
    for (int k = 0; k < cnt; ++k) {                                      // (every exit below is uniform over the workgroup)
        int lo = DR_NONE;
#pragma unroll
        for (int q = DR_WPT - 1; q >= 0; --q)
            if (rem[q]) lo = (tid + 256 * q) * 64 + __ffsll((unsigned long long)rem[q]) - 1;
        lo = wave_min(lo);
        __syncthreads();                                                 // (reds, redd of the droplet before have been read)
        if (lane == 0) redi[wave] = lo;
        __syncthreads();
        const int root = min(min(redi[0], redi[1]), min(redi[2], redi[3]));
        if (root == DR_NONE) break;
#pragma unroll
        for (int q = 0; q < DR_WPT; ++q) {
            const int w = tid + 256 * q;
            prev[q] = 0;
            if (w < nwords) Vl[w] = w == (root >> 6) ? (unsigned long long)1 << (root & 63) : 0ull;
        }
        double acc = 0.0;
        __syncthreads();
        for (int pass = 0; pass <= g.nbits; ++pass) {
            uint64_t f[DR_WPT];
            bool any = false;
#pragma unroll
            for (int q = 0; q < DR_WPT; ++q) {
                const int w = tid + 256 * q;
                f[q] = 0;
                if (w < nwords) {
                    const uint64_t v = __hip_atomic_load(&Vl[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & rem[q];
                    f[q] = v & ~prev[q];
                    prev[q] = v;
                    any |= f[q] != 0;
                }
            }
            if (!__syncthreads_or(any)) break;                           // every frontier is read; none anywhere: V is the fixed point
#pragma unroll
            for (int q = 0; q < DR_WPT; ++q) expand_droplet(f[q], tid + 256 * q, Dl, Rl, Vl, g, acc);
            __syncthreads();                                             // the ORs of this pass have landed
        }
        int sz = 0;
#pragma unroll
        for (int q = 0; q < DR_WPT; ++q) {
            uint64_t cl = prev[q];                                       // (the last look found nothing new: prev is V)
            rem[q] &= ~cl;
            sz += __popcll(cl);
            if (lab)
                while (cl) {
                    lab[(tid + 256 * q) * 64 + __ffsll((unsigned long long)cl) - 1] = k;
                    cl &= cl - 1;
                }
        }
        sz = wave_sum(sz);
        acc = wave_sum(acc);
        if (lane == 0) {
            reds[wave] = sz;
            redd[wave] = acc;
        }
        __syncthreads();
        const int size = reds[0] + reds[1] + reds[2] + reds[3];
        if (size < 256) small += tid == size;
        else if (tid == 0) atomicAdd(&o.size_hist[size], 1ull);
        if (tid == 0) tot.emit(o, m, root, size, 2.0 * ((redd[0] + redd[1]) + (redd[2] + redd[3])));
    }
    if (small) atomicAdd(&o.size_hist[tid], (unsigned long long)small);
    __syncthreads();
    if (tid == 0) {
        tot.finish(o, m, cnt);
        redi[0] = tot.count;
    }
    __syncthreads();
    for (int k = redi[0] + tid; k < o.K; k += 256) {
        o.root[m * o.K + k] = -1;
        o.size[m * o.K + k] = 0;
        o.de[m * o.K + k] = 0.0;
    }
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tn_droplets(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const uint64_t* ref, const int32_t* rowptr, const int32_t* cols,
                const double* vals, int64_t nnz, const double* field, int64_t K, int32_t* count_out, int32_t* diff_out, int32_t* largest_out,
                double* de_total_out, int32_t* root_out, int32_t* size_out, double* de_out, int64_t* size_hist, int32_t* labels, int64_t ldl,
                void* stream) {
    const int64_t two31 = (int64_t)1 << 31;
    TN_CHECK_ARG(M >= 0 && M < two31, "M negative or not below 2^31");
    if (nbits < 1 || nbits > cluster_exchange_max_nbits()) {
        set_error("tn_droplets: nbits = %lld outside 1 .. %lld", (long long)nbits, (long long)cluster_exchange_max_nbits());
        return -1;
    }
    TN_CHECK_ARG(nnz >= 0 && nnz < two31, "nnz negative or not below 2^31");
    TN_CHECK_ARG(K >= 0 && K < two31, "K negative or not below 2^31");
    TN_CHECK_ARG(mul_fits({M, K}), "M K does not fit an index");
    const int64_t nwords = cdiv(nbits, 64);
    TN_CHECK_ARG(ldr >= nwords, "ldr shorter than a row of ceil(nbits / 64) words");
    TN_CHECK_ARG(!labels || (ldl >= nbits && mul_fits({M, ldl})), "ldl shorter than the nbits labels of a row (or M ldl does not fit an index)");
    if (M == 0) return 0;
    TN_CHECK_ARG(rows && ref && rowptr && (nnz == 0 || (cols && vals)) && count_out && diff_out && largest_out && de_total_out && size_hist &&
                     (K == 0 || (root_out && size_out && de_out)),
                 "null operand");
    const int used = (int)(nbits - (nwords - 1) * 64);
    const uint64_t last_mask = used == 64 ? ~(uint64_t)0 : (((uint64_t)1 << used) - 1);
    const DropletGraph g{rowptr, cols, vals, field, (int)nnz, (int)nbits};
    const DropletOut o{count_out, diff_out, largest_out, de_total_out, root_out, size_out, de_out, (unsigned long long*)size_hist, labels, ldl, (int)K};
    hipStream_t st = (hipStream_t)stream;
    if (nbits <= DR_WAVE_BITS) {
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(droplets_wave_kernel, dim3((unsigned)cdiv(M, DR_WAVES)), dim3(64 * DR_WAVES), 0, st, rows, M,
                                                         (int)nwords, ldr, last_mask, ref, g, o));
        TN_CHECK_LAUNCH("droplets_wave_kernel");
    } else {
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(droplets_block_kernel, dim3((unsigned)M), dim3(256), 0, st, rows, M, (int)nwords, ldr, last_mask,
                                                         ref, g, o));
        TN_CHECK_LAUNCH("droplets_block_kernel");
    }
    return 0;
}

}  // extern "C"
