// The two products of a contraction that goes through the MPS (x) MPO factors, in one launch.
//
//     stage 1:  S_z[(i, j), n] = sum_{k < K1}  P[z, i, k] X[k, j, n]           i < I, j < J
//     stage 2:  Out_z[m, n]    = sum_{q < I J} W[m, q] S_z[q, n]               q = i J + j,  m = m_hi Mlo + m_lo
//
// Every operand is addressed by element strides.  The Gram step of the weighted first pass (T1 = Gp A, T2 = Wx T1) and the attach
// through the factors (T = A C, M = Wq T; chain.hip) are this pair: as two launches of gemm_kernel the first writes S for every z
// to memory (134 MB at a bulk site of the flagship workload) and the second, a batched product with a 64-wide side on 64 x 64
// tiles, reads it straight back.  Here a 512-thread workgroup owns one (z, chunk of 64 columns n), keeps its S tile (I J <= 256
// rows x 64 columns, 128 KiB) in LDS and never shares anything with another workgroup: no counters, no atomics.
//
// Stage 1.  A unit is one 16 x 16 MFMA tile of S: the rows i (I <= 16, one tile of rows) of one j, 16 columns of the chunk.  The
// units go round the eight waves.  With K1 <= 64 a wave keeps ITS fragments of P in registers for the whole stage (16 doubles per
// lane, MFMA lane layout A[l&15][l>>4]) and reads the fragments of X straight from memory (B[l>>4][l&15]: 16 consecutive n per k,
// full 128-byte segments with unit stride along n): every element of X's chunk enters exactly one MFMA of the workgroup, so a
// detour through LDS would save no traffic.  The loads of the next unit are in flight while this one is multiplied.
// Stage 2.  Wave w owns the rows 32 w .. 32 w + 31 of a 256-row slab of Out and all columns of the chunk: 2 x 4 tiles in
// registers over the whole depth I J.  The fragments of W come straight from memory as well (each is used for the four column
// tiles; the callers of chain.hip pass W q-major, so that the 16 rows of a fragment are one 128-byte segment), one 16-step ahead
// of the multiplications; the fragments of S come from LDS.  S is stored q-major with 64 doubles per row and bit 4 of the column
// flipped on odd q: the four rows q of a fragment read (16 consecutive doubles each) then fall into alternating halves of the 64
// banks, which is what the pitch of 16 extra doubles does for gemm_kernel's stages without spending the LDS.  No barrier inside
// a stage, one between them.
//
// Same bits as gemm + gemm (alpha = 1, beta = 0, no split of K): every element of S is acc = 0, then acc = mfma_f64_16x16x4(a, b,
// acc) over the groups of four k ascending, K1 padded with zeros to whole 16-steps, lane l >> 4 supplying k = 4 g + (l >> 4) of
// group g, exactly gemm_kernel's sequence for that element; every element of Out likewise over q.  Which wave or tile an element
// belongs to, and whether an operand came through LDS, does not enter its sum.  The host side (factor_products_fits, and the
// callers' check that the launch plan would not split the first product) decides where this holds; everything else keeps the
// two launches.
//
// All loads are unconditional with indices clamped to the last valid one (the value is replaced by zero where the index was
// out of range, see fp_keep), every store is guarded.
#include "common.h"

namespace tn {

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int FP_NC = 64;           // columns n of a workgroup's chunk
constexpr int FP_QMAX = 256;        // rows I J of the S tile
constexpr int FP_IMAX = 16;         // one MFMA tile of rows i
constexpr int FP_K1MAX = 64;        // depth of stage 1 (P's fragments stay in registers)
constexpr int FP_THREADS = 512, FP_WAVES = FP_THREADS / 64;
constexpr int FP_SLAB = 32 * FP_WAVES;      // rows of Out per round of stage 2

struct FacP {
    const double* P;
    const double* X;
    const double* W;
    double* Out;
    int Z, I, J, K1, N, M, Mlo, chunks;
    int64_t pz, pi, pk, xk, xj, xn, wm, wq, oz, ohi, olo, on;
};

__device__ __forceinline__ int fp_sidx(int q, int c) { return q * FP_NC + (c ^ ((q & 1) << 4)); }

// v where keep, else +0.0.  The loads are unconditional (clamped indices); written as a select, the compiler moves each load into a
// branch of its own on the condition and waits for it there -- one memory round trip per load.  So the value is masked bitwise, with
// a mask the optimiser cannot see through (an empty asm: no instruction, no wait -- the mask does not come from memory).
__device__ __forceinline__ double fp_keep(double v, bool keep) {
    long long m = keep ? -1ll : 0ll;
    asm volatile("" : "+v"(m));
    return __longlong_as_double(__double_as_longlong(v) & m);
}

template <int KS>       // 16-steps of K1
__device__ __forceinline__ void fp_stage1(const FacP& g, double* S, const int z, const int n0, const int nb, const int wave, const int lr, const int lk) {
    constexpr int KG = 4 * KS;
    double p[KG];
    {
        const double* Pz = g.P + (int64_t)z * g.pz + (int64_t)min(lr, g.I - 1) * g.pi;
#pragma unroll
        for (int kk = 0; kk < KG; ++kk) {
            const int k = kk * 4 + lk;
            const double v = Pz[(int64_t)min(k, g.K1 - 1) * g.pk];
            p[kk] = fp_keep(v, lr < g.I && k < g.K1);
        }
    }
    const int units = g.J * nb;
    auto load = [&](double (&b)[KG], const int u) {
        const int uc = min(u, units - 1), j = uc / nb, cb = uc - j * nb, n = n0 + cb * 16 + lr;
        const double* Xp = g.X + (int64_t)j * g.xj + (int64_t)min(n, g.N - 1) * g.xn;
#pragma unroll
        for (int kk = 0; kk < KG; ++kk) {
            const int k = kk * 4 + lk;
            const double v = Xp[(int64_t)min(k, g.K1 - 1) * g.xk];
            b[kk] = fp_keep(v, n < g.N && k < g.K1);
        }
    };
    auto multiply = [&](const double (&b)[KG], const int u) {
        if (u >= units) return;
        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < KG; ++kk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(p[kk], b[kk], acc, 0, 0, 0);
        const int j = u / nb, cb = u - j * nb;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = lk + 4 * r;
            if (i < g.I) S[fp_sidx(i * g.J + j, cb * 16 + lr)] = acc[r];
        }
    };
    double b0[KG], b1[KG];
    load(b0, wave);
    for (int u = wave; u < units; u += 2 * FP_WAVES) {
        load(b1, u + FP_WAVES);
        multiply(b0, u);
        load(b0, u + 2 * FP_WAVES);
        multiply(b1, u + FP_WAVES);
    }
}

template <int TN>       // 16-column tiles of the chunk
__device__ __forceinline__ void fp_stage2(const FacP& g, const double* S, const int z, const int n0, const int Q, const int m0, const int lr, const int lk) {
    const double* Wr[2];
    bool rv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + i * 16 + lr;
        rv[i] = m < g.M;
        Wr[i] = g.W + (int64_t)min(m, g.M - 1) * g.wm;
    }
    auto load = [&](double (&a)[4][2], const int qs) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int q = qs + kk * 4 + lk;
            const int64_t off = (int64_t)min(q, Q - 1) * g.wq;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const double v = Wr[i][off];
                a[kk][i] = fp_keep(v, rv[i] && q < Q);
            }
        }
    };
    d4 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
    double ac[4][2], an[4][2];
    load(ac, 0);
    for (int qs = 0; qs < Q; qs += 16) {
        load(an, qs + 16);                                  // (past the end: clamped addresses, zeros, never multiplied)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int q = qs + kk * 4 + lk;
            double b[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = S[fp_sidx(q, j * 16 + lr)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[kk][i], b[j], acc[i][j], 0, 0, 0);
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int i = 0; i < 2; ++i) ac[kk][i] = an[kk][i];
    }
    double* Oz = g.Out + (int64_t)z * g.oz;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + i * 16 + lk + 4 * r;
            if (m >= g.M) continue;
            const int mh = m / g.Mlo, ml = m - mh * g.Mlo;
            double* o = Oz + (int64_t)mh * g.ohi + (int64_t)ml * g.olo;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + j * 16 + lr;
                if (n < g.N) o[(int64_t)n * g.on] = acc[i][j][r];
            }
        }
}

template <int KS>
__global__ __launch_bounds__(FP_THREADS) void factor_products_kernel(FacP g) {
    __shared__ double S[FP_QMAX * FP_NC];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lk = lane >> 4;
    int bid = blockIdx.x;
    {   // XCD-aware order, as gemm_kernel: the chunks of one z (they share P) and neighbouring z land on the same XCD
        const int nwg = gridDim.x, q = nwg / 8, r = nwg % 8, xcd = bid % 8, loc = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int z = bid / g.chunks, n0 = (bid - z * g.chunks) * FP_NC;
    const int nb = (min(FP_NC, g.N - n0) + 15) >> 4;
    const int Q = g.I * g.J, Qpad = (Q + 15) & ~15;
    for (int e = Q * FP_NC + tid; e < Qpad * FP_NC; e += FP_THREADS) S[e] = 0.0;     // the rows stage 2 reads beyond Q (whole rows: the swizzle stays inside one)
    fp_stage1<KS>(g, S, z, n0, nb, wave, lr, lk);
    __syncthreads();
    for (int mt = 0; mt < g.M; mt += FP_SLAB) {
        const int m0 = mt + wave * 32;
        if (m0 >= g.M) break;                               // (uniform per wave; no barrier follows)
        if (nb == 4) fp_stage2<4>(g, S, z, n0, Q, m0, lr, lk);
        else if (nb == 3) fp_stage2<3>(g, S, z, n0, Q, m0, lr, lk);
        else if (nb == 2) fp_stage2<2>(g, S, z, n0, Q, m0, lr, lk);
        else fp_stage2<1>(g, S, z, n0, Q, m0, lr, lk);
    }
}

}  // namespace

bool factor_products_fits(int64_t Z, int64_t I, int64_t J, int64_t K1, int64_t N, int64_t M) {
    if (Z < 1 || I < 1 || J < 1 || K1 < 1 || N < 1 || M < 1) return false;
    if (I > FP_IMAX || I * J > FP_QMAX || K1 > FP_K1MAX) return false;
    return M < ((int64_t)1 << 30) && N < ((int64_t)1 << 30) && Z * cdiv(N, FP_NC) < ((int64_t)1 << 31);
}

int factor_products(hipStream_t st, const FactorProducts& f) {
    TN_CHECK_ARG(factor_products_fits(f.Z, f.I, f.J, f.K1, f.N, f.Mhi * f.Mlo) && f.Mhi >= 1 && f.Mlo >= 1, "shape outside the kernel's limits");
    FacP g;
    g.P = f.P; g.X = f.X; g.W = f.W; g.Out = f.Out;
    g.Z = (int)f.Z; g.I = (int)f.I; g.J = (int)f.J; g.K1 = (int)f.K1; g.N = (int)f.N; g.M = (int)(f.Mhi * f.Mlo); g.Mlo = (int)f.Mlo;
    g.chunks = (int)cdiv(f.N, FP_NC);
    g.pz = f.pz; g.pi = f.pi; g.pk = f.pk; g.xk = f.xk; g.xj = f.xj; g.xn = f.xn; g.wm = f.wm; g.wq = f.wq;
    g.oz = f.oz; g.ohi = f.ohi; g.olo = f.olo; g.on = f.on;
    const dim3 grid((unsigned)(f.Z * g.chunks));
    const double Q = (double)(f.I * f.J), M = (double)g.M;
    // booked with the 64 x 64 launches it replaces: the flops of both stages, the bytes of P, X and W in and Out out
    prof_begin(st, PROF_GEMM_64x64);
    switch (cdiv(f.K1, 16)) {
        case 1: hipLaunchKernelGGL((factor_products_kernel<1>), grid, dim3(FP_THREADS), 0, st, g); break;
        case 2: hipLaunchKernelGGL((factor_products_kernel<2>), grid, dim3(FP_THREADS), 0, st, g); break;
        case 3: hipLaunchKernelGGL((factor_products_kernel<3>), grid, dim3(FP_THREADS), 0, st, g); break;
        default: hipLaunchKernelGGL((factor_products_kernel<4>), grid, dim3(FP_THREADS), 0, st, g); break;
    }
    TN_CHECK_LAUNCH("factor_products_kernel");
    prof_end(st, PROF_GEMM_64x64, 2.0 * f.Z * f.N * Q * ((double)f.K1 + M),
             8.0 * ((double)f.Z * f.I * f.K1 + (double)f.K1 * f.J * f.N + M * Q + (double)f.Z * M * f.N));
    return 0;
}

}  // namespace tn
