// Rank-b update of a trailing matrix, C (m x n) -= W (m x b) X (b x n) with 1 <= b <= 32: the product behind every panel of the
// blocked QR (qr.hip), as a kernel of its own instead of a K = 32 launch of gemm_kernel (gemm_f64.hip).
//
// The generic kernel stages its operands through LDS (load, store, barrier, two K steps, barrier) and only then fetches the old
// values of C: three dependent memory round trips around 8 MFMA issues per 16 x 16 tile.  With K <= 32 the operands of a wave fit in
// registers in the MFMA lane layout (A[l&15][l>>4], B[l>>4][l&15]), so here a wave issues EVERY load it needs -- its 2 x 8 fragments
// of W, its 2 x 8 fragments of X and the 16 old values of its 32 x 32 piece of C -- back to back, then multiplies, subtracts and
// stores: one round trip, no LDS, no barrier.  The operands are issued first, so the multiplications start while C is still in
// flight.  All loads are unconditional: an index past an edge is clamped to the last valid one (k past b then selects zero; a row
// or column past the edge only feeds results that are never stored), so the loads of a path form one basic block, and a
// scheduling barrier keeps them in front of the first MFMA (without it the compiler interleaves them with the multiplications to
// save registers, and sinks the loads of C below the branch on the flag).  The skip flag (*active, device-side pivoting) is read
// in the same round trip and only guards the stores: a launch enqueued behind the exit reads its operands for nothing and writes
// nothing.
//
// Tiles and order are gemm_kernel<64,64>'s: 64 x 64 per 256-thread workgroup, four waves as 2 x 2, the XCD-aware tile order (the
// tiles of one row-panel share W through one L2).  The lanes of an access to C run along its columns; a column-major C is updated as
// the transposed product C^T -= X^T W^T (operand roles exchanged by the host function), as gemm_ex does.  The two 16 x 16 tiles a
// lane holds side by side take the columns 2 l and 2 l + 1 (not l and l + 16): with unit stride along the columns -- both layouts of
// the workload -- a lane moves its pair of X and of C in one 16-byte access, 256 consecutive bytes per row and instruction, half
// the memory instructions.  Which columns a tile holds changes no result: every element still sees its own row of W, its own
// column of X and the same sequence of MFMA issues.  Pieces that touch an edge, and other strides, take the 8-byte path with
// guarded stores.  The wave index is made uniform (readfirstlane) so that the choice between the two paths is a scalar branch:
// as a divergent one both paths run under exec masks, and the second waits for loads of the first that share its registers.
//
// Same bits as the launch it replaces: per element acc = 0, then acc = mfma_f64_16x16x4(a, b, acc) over the groups of four k in
// ascending order, K padded with zeros to a multiple of 16 (4 or 8 issues, as the generic K steps of 16), result c_old - acc
// (= alpha acc + beta c_old with alpha = -1, beta = 1: both products are exact).  The transposed form exchanges the factors of
// each scalar product only.  K = 32 < 2 TN_GEMM_MINCHUNK: the launch plan never splits K for these products at its defaults.
//
// Compiled for gfx950 (-Rpass-analysis=kernel-resource-usage): no scratch, no LDS, 147 VGPRs = 3 waves per SIMD for b > 16
// (111 = 4 for b <= 16); 32 loads (16-byte path) or 48 (8-byte path) in flight per wave.
#include "common.h"

namespace tn {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef d2 d2u __attribute__((aligned(8)));      // a pair of columns starts at any even column of any row

struct RankP {
    const double* A;      // M x K
    const double* B;      // K x N
    double* C;            // M x N, lanes along N
    int M, N, K;
    int64_t rsa, csa, rsb, csb, rsc, csc;
    int tiles_n;
    const int* active;
};

// One wave's 32 x 32 piece at (r0, c0).  WIDE: the piece lies inside the matrix and C and B have unit stride along the columns --
// tile j holds the columns c0 + 2 (lane & 15) + j, so a lane's two tiles are neighbours and B and C move in 16-byte accesses.
// Otherwise the same column assignment with 8-byte accesses, indices clamped at the edges and every store guarded.
template <int KG, bool WIDE>
__device__ __forceinline__ void rank_update_piece(const RankP& g, const int r0, const int c0, const int lr, const int lk, const int act) {
    double a[2][KG], b[2][KG], cv[2][2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const double* pa = g.A + (int64_t)min(r0 + i * 16 + lr, g.M - 1) * g.rsa;
#pragma unroll
        for (int kk = 0; kk < KG; ++kk) a[i][kk] = pa[(int64_t)min(kk * 4 + lk, g.K - 1) * g.csa];
    }
    if constexpr (WIDE) {
        const double* pb = g.B + (c0 + 2 * lr);
#pragma unroll
        for (int kk = 0; kk < KG; ++kk) {
            const d2 v = *(const d2u*)(pb + (int64_t)min(kk * 4 + lk, g.K - 1) * g.rsb);
            b[0][kk] = v.x; b[1][kk] = v.y;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const d2 v = *(const d2u*)(g.C + (int64_t)(r0 + i * 16 + lk + 4 * r) * g.rsc + (c0 + 2 * lr));
                cv[i][0][r] = v.x; cv[i][1][r] = v.y;
            }
    } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double* pb = g.B + (int64_t)min(c0 + 2 * lr + j, g.N - 1) * g.csb;
#pragma unroll
            for (int kk = 0; kk < KG; ++kk) b[j][kk] = pb[(int64_t)min(kk * 4 + lk, g.K - 1) * g.rsb];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    cv[i][j][r] = g.C[(int64_t)min(r0 + i * 16 + lk + 4 * r, g.M - 1) * g.rsc + (int64_t)min(c0 + 2 * lr + j, g.N - 1) * g.csc];
    }
    __builtin_amdgcn_sched_barrier(0);               // every load above is issued before the first multiplication below

    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < KG; ++kk) {
        const bool kin = kk * 4 + lk < g.K;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(kin ? a[i][kk] : 0.0, kin ? b[j][kk] : 0.0, acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) cv[i][j][r] -= acc[i][j][r];
    __builtin_amdgcn_sched_barrier(0);               // (the results exist before the flag decides about the stores)

    if (!act) return;
    if constexpr (WIDE) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *(d2u*)(g.C + (int64_t)(r0 + i * 16 + lk + 4 * r) * g.rsc + (c0 + 2 * lr)) = d2{cv[i][0][r], cv[i][1][r]};
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = r0 + i * 16 + lk + 4 * r, col = c0 + 2 * lr + j;
                    if (row < g.M && col < g.N) g.C[(int64_t)row * g.rsc + (int64_t)col * g.csc] = cv[i][j][r];
                }
    }
}

template <int KG, bool FLAG>         // KG groups of four k: 4 (K <= 16) or 8 (K <= 32); FLAG: *active is read
__global__ __launch_bounds__(256, 2) void rank_update_kernel(RankP g) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // (uniform: the branches below are scalar)
    const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lk = lane >> 4;
    int bid = blockIdx.x;
    {   // XCD-aware tile order, as gemm_kernel
        const int nwg = gridDim.x, q = nwg / 8, r = nwg % 8, xcd = bid % 8, loc = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int r0 = (bid / g.tiles_n) * 64 + wm * 32, c0 = (bid % g.tiles_n) * 64 + wn * 32;
    if (r0 >= g.M || c0 >= g.N) return;              // (a wave of its own: there is no barrier to miss)
    const int act = FLAG ? *g.active : 1;
    if (r0 + 32 <= g.M && c0 + 32 <= g.N && g.csc == 1 && g.csb == 1) rank_update_piece<KG, true>(g, r0, c0, lr, lk, act);
    else rank_update_piece<KG, false>(g, r0, c0, lr, lk, act);
}

}  // namespace

int rank_update(hipStream_t st, int64_t m, int64_t n, int b, const double* W, int64_t wrs, int64_t wcs, const double* X, int64_t xrs,
                int64_t xcs, double* C, int64_t rsc, int64_t csc, const int* active) {
    if (m <= 0 || n <= 0) return 0;
    TN_CHECK_ARG(b >= 1 && b <= 32, "the rank must be between 1 and 32");
    TN_CHECK_ARG(cdiv(m, 64) * cdiv(n, 64) < ((int64_t)1 << 31), "too many tiles");
    RankP g;
    g.C = C; g.K = b; g.active = active;
    if (rsc == 1 && csc != 1) {        // column-major C: C^T -= X^T W^T, the lanes along the unit stride
        g.A = X; g.rsa = xcs; g.csa = xrs; g.B = W; g.rsb = wcs; g.csb = wrs; g.M = (int)n; g.N = (int)m; g.rsc = csc; g.csc = rsc;
    } else {
        g.A = W; g.rsa = wrs; g.csa = wcs; g.B = X; g.rsb = xrs; g.csb = xcs; g.M = (int)m; g.N = (int)n; g.rsc = rsc; g.csc = csc;
    }
    g.tiles_n = (int)cdiv(g.N, 64);
    const dim3 grid((unsigned)(cdiv(g.M, 64) * g.tiles_n));
    // booked under the family gemm would have launched, with its flops; the bytes count C read and written
    const int fam = gemm_prof_family(m, n, b, rsc, csc);
    prof_begin(st, fam);
    if (b <= 16 && active) hipLaunchKernelGGL((rank_update_kernel<4, true>), grid, dim3(256), 0, st, g);
    else if (b <= 16) hipLaunchKernelGGL((rank_update_kernel<4, false>), grid, dim3(256), 0, st, g);
    else if (active) hipLaunchKernelGGL((rank_update_kernel<8, true>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((rank_update_kernel<8, false>), grid, dim3(256), 0, st, g);
    TN_CHECK_LAUNCH("rank_update_kernel");
    prof_end(st, fam, 2.0 * m * n * b, 8.0 * ((double)m * b + (double)b * n + 2.0 * m * n));
    return 0;
}

}  // namespace tn
