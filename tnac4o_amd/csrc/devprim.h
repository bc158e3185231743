// Device primitives shared by the kernels of libtnpeps (gfx950 only).  Internal header: everything here is
// static __device__ __forceinline__, nothing has external linkage.
#pragma once
#include "common.h"

namespace tn {

// ---- agent-scope accesses: what workgroups of one launch publish to each other ----------------------------------------------
static __device__ __forceinline__ double ld_agent(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static __device__ __forceinline__ int ldi_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// What the workgroups publish to each other (partial Gram matrices, block exponents) is written with agent-scope stores:
// they go through to memory, so the publisher only waits for their completion before it takes its ticket -- a release
// fence would also write back every dirty line of the XCD's L2 (the tile just stored: 3.6 us measured against ~1).
static __device__ __forceinline__ void st_agent(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static __device__ __forceinline__ void sti_agent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
static __device__ __forceinline__ void publish_wait() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_waitcnt(0); }

// In-kernel barrier of the workgroups of one launch (they must be co-resident, see fused.hip): a monotone arrival counter polled
// by one lane; `target` = arrivals expected so far.  Every wave first waits for its agent-scope stores.  SLEEP: argument of the
// s_sleep between two looks at the counter; naps: further pauses of ~0.4 us each for waits known to be long.  Bounded: false when
// the counter has not reached the target after spin_limit looks (the caller poisons its output and books a time-out).
template <int SLEEP>
static __device__ __forceinline__ bool grid_barrier(int* counter, int target, int* s_flag, int tid, unsigned spin_limit, int naps = 0) {
    publish_wait();                                        // every wave: its agent-scope stores have completed
    __syncthreads();
    if (tid == 0) {
        atomicAdd(counter, 1);
        int ok = 1;
        unsigned spins = 0;
        while (ldi_agent(counter) < target) {
            __builtin_amdgcn_s_sleep(SLEEP);
            for (int i = 0; i < naps; ++i) __builtin_amdgcn_s_sleep(15);
            if (++spins > spin_limit) { ok = 0; break; }
        }
        *s_flag = ok;
    }
    __syncthreads();
    return *s_flag != 0;
}

// ---- lanes and arithmetic ----------------------------------------------------------------------------------------------------
static __device__ __forceinline__ double readlane_f64(double v, int lane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, lane);
    hi = __builtin_amdgcn_readlane(hi, lane);
    return __hiloint2double(hi, lo);
}
static __device__ __forceinline__ double rsqrt2(double x) {      // hardware seed (~2^-26) + two Newton steps: full double accuracy
    double r = __builtin_amdgcn_rsq(x);
    r = r * (1.5 - 0.5 * x * r * r);
    r = r * (1.5 - 0.5 * x * r * r);
    return r;
}
// Fast reciprocal square root / reciprocal with three Newton steps (full double accuracy to ~1 ulp; the hardware
// seeds are single-precision accurate).  They sit on the per-column critical path of the panel factorisation.
static __device__ __forceinline__ double fast_rsqrt(double x) {
    double r = __builtin_amdgcn_rsq(x);
    r = r * (1.5 - 0.5 * x * r * r);
    r = r * (1.5 - 0.5 * x * r * r);
    r = r * (1.5 - 0.5 * x * r * r);
    return r;
}
static __device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = r * (2.0 - x * r);
    r = r * (2.0 - x * r);
    r = r * (2.0 - x * r);
    return r;
}
// acc -= a * b, pinned in program order: left to itself the compiler sinks the rank-1 updates of an unrolled factorisation
// into 31-long dependent chains at the point of use and spills the multipliers it keeps alive for them
static __device__ __forceinline__ void fnma(double& acc, double a, double b) {
    asm volatile("v_fma_f64 %0, -%1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
// acc -= s * v with the first factor wave-uniform (an SGPR pair), pinned in program order like fnma
static __device__ __forceinline__ void fnma_s(double& acc, double s_uniform, double v) {
    asm volatile("v_fma_f64 %0, -%1, %2, %0" : "+v"(acc) : "s"(s_uniform), "v"(v));
}
// deterministic noise in [-0.5, 0.5) for columns that are refilled
static __device__ __forceinline__ double hash_unit(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return ((double)(x >> 11) * (1.0 / 9007199254740992.0)) - 0.5;
}
// rows r0 .. r0 + nr - 1 of workgroup blk when nrows are dealt out evenly to nblk workgroups
static __device__ __forceinline__ void block_rows(int64_t nrows, int nblk, int blk, int64_t& r0, int& nr) {
    const int64_t base = nrows / nblk, rem = nrows % nblk;
    r0 = blk * base + (blk < rem ? blk : rem);
    nr = (int)(base + (blk < rem ? 1 : 0));
}

// ---- 256-thread reductions ---------------------------------------------------------------------------------------------------
// sum through wave shuffles and LDS (two barriers); red: >= 4 doubles
static __device__ __forceinline__ double block_sum(double v, double* red, int tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// binary trees in LDS (fixed order of additions whatever the wave size); red: 256 doubles, free again on return
static __device__ __forceinline__ double block_tree_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) red[tid] += red[tid + k];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}
static __device__ __forceinline__ double block_tree_min(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) red[tid] = fmin(red[tid], red[tid + k]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

}  // namespace tn
