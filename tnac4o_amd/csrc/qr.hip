// K3 — economic QR with non-negative diagonal of R (reference mps.py:43-59; call sites orth_left/right :532-548).
//
// Blocked Householder QR designed for launch-level parallelism instead of LAPACK's column-serial panel:
//   for each panel (nb columns of the trailing matrix):
//     1. orthonormalise the panel by 4 rounds of "scaled Gram -> Jacobi eigenvectors -> W <- W D^-1 J"
//        (one-sided block Jacobi on the panel; columns that are exactly zero or collapse to rounding noise are
//        refilled with hash noise so the basis is complete), then normalise;
//     2. Householder reconstruction (Ballard et al. 2014): sign-choosing LU of the top block gives Y (unit lower
//        trapezoidal) and T with  H = I - Y T Y^T,  H[:, :nb] = Q1 S;
//     3. trailing update  A <- H^T A  as three GEMMs on the MFMA kernel.
//   Q = H_1 ... H_P [Z; 0] accumulated backwards with GEMMs; the dense nb x nb diagonal blocks left by step 1 are
//   triangularised by small Householder QRs (Z), which also fixes diag(R) >= 0.
// Every transformation applied to A is orthogonal to rounding (the Gram matrices only steer the rotations), so the
// factorisation is column-wise backward stable like dgeqrf even for the numerically rank-deficient, strongly graded
// matrices this path produces (validated against LAPACK on matrices captured from the droplet sweeps).
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "common.h"
#include "devprim.h"

namespace tn {

// ------------------------------------------------------------------------------------------ helpers
__global__ __launch_bounds__(256) void copy_mat_kernel(const double* __restrict__ S, int64_t srs, int64_t scs,
                                                       double* __restrict__ D, int64_t drs, int64_t dcs, int64_t m,
                                                       int64_t n, int colfast) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m * n) return;
    const int64_t i = colfast ? e / n : e % m, j = colfast ? e % n : e / m;
    D[i * drs + j * dcs] = S[i * srs + j * scs];
}

int copy_mat(hipStream_t st, const double* S, int64_t srs, int64_t scs, double* D, int64_t drs, int64_t dcs, int64_t m,
             int64_t n) {
    if (m <= 0 || n <= 0) return 0;
    const int colfast = (dcs == 1 || scs == 1) ? 1 : 0;
    TN_PROF_LAUNCH(st, PROF_QR_AUX, hipLaunchKernelGGL(copy_mat_kernel, dim3((unsigned)cdiv(m * n, 256)), dim3(256), 0, st, S, srs, scs, D, drs, dcs, m,
                       n, colfast));
    TN_CHECK_LAUNCH("copy_mat_kernel");
    return 0;
}

__global__ __launch_bounds__(256) void fill_mat_kernel(double* __restrict__ D, int64_t drs, int64_t dcs, int64_t m, int64_t n, double v,
                                                       int colfast) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= m * n) return;
    const int64_t i = colfast ? e / n : e % m, j = colfast ? e % n : e / m;
    D[i * drs + j * dcs] = v;
}
static int fill_mat(hipStream_t st, double* D, int64_t drs, int64_t dcs, int64_t m, int64_t n, double v) {
    if (m <= 0 || n <= 0) return 0;
    TN_PROF_LAUNCH(st, PROF_QR_AUX, hipLaunchKernelGGL(fill_mat_kernel, dim3((unsigned)cdiv(m * n, 256)), dim3(256), 0, st, D, drs, dcs, m, n, v,
                       dcs == 1 ? 1 : 0));
    TN_CHECK_LAUNCH("fill_mat_kernel");
    return 0;
}

// column swaps of a panel-pivoting step, applied in order to every row: A(r, pairs[2t]) <-> A(r, pairs[2t+1]), t = 0 .. npairs-1
// The swaps of a pivoting step as ONE gather / scatter: the host composes the sequence of swaps into "column dst[i] receives the
// old column src[i]" over the (at most 64) columns they touch; a thread fetches its row's values of all those columns together and
// then stores them (the swaps applied one after the other cost two dependent round trips each: 12 us per panel).  The list travels
// by value in the kernel arguments: no host-to-device copy, no staging buffer to keep alive.
struct SwapList { int n; int dst[64]; int src[64]; };
__global__ __launch_bounds__(256) void swap_columns_kernel(double* __restrict__ A, int64_t rs, int64_t cs, int64_t m, SwapList sl) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    double* row = A + r * rs;
    double v[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) v[i] = (i < sl.n) ? row[(int64_t)sl.src[i] * cs] : 0.0;
#pragma unroll
    for (int i = 0; i < 64; ++i)
        if (i < sl.n) row[(int64_t)sl.dst[i] * cs] = v[i];
}
// pairs: npairs swaps (a, b) applied in order -> the moves they amount to
static void compose_swaps(const int* pairs, int npairs, SwapList& sl) {
    int cols[64], from[64], nc = 0;                  // touched columns and, for each, the ORIGINAL column whose data it holds now
    auto slot = [&](int c) { for (int i = 0; i < nc; ++i) if (cols[i] == c) return i; cols[nc] = c; from[nc] = c; return nc++; };
    for (int t = 0; t < npairs; ++t) {
        const int a = pairs[2 * t], b = pairs[2 * t + 1];
        if (a == b) continue;
        const int ia = slot(a), ib = slot(b);
        const int tmp = from[ia]; from[ia] = from[ib]; from[ib] = tmp;
    }
    sl.n = 0;
    for (int i = 0; i < nc; ++i)
        if (from[i] != cols[i]) { sl.dst[sl.n] = cols[i]; sl.src[sl.n] = from[i]; ++sl.n; }
}

// columns of the panel flagged dead (exactly zero) get deterministic pseudo-random content
__global__ __launch_bounds__(256) void refill_dead_kernel(double* __restrict__ W, int64_t rs, int64_t cs, int64_t m,
                                                          int b, const int* __restrict__ dead, uint64_t seed) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= m) return;
    for (int j = 0; j < b; ++j)
        if (dead[j]) W[r * rs + j * cs] = hash_unit(seed + (uint64_t)r * 64 + j);
}

// ------------------------------------------------------------------------------------------ reconstruction
// One workgroup.  In: top b x b block of the orthonormal panel (strided).  Out: Y1 (unit lower triangular, written
// back in place with explicit zeros/ones), Uinv (b x b), T (b x b upper), and the products that fold T into the tall
// factors so that a block reflector is applied with two GEMMs instead of three:
//   W = Y T^T (trailing update A -= W (Y^T A)),  Wq = Y T (Q accumulation Q -= Wq (Y^T Q)),  Y = [Y1; Q1_below Uinv]:
//   rows below the top block use UT = Uinv T^T and UTq = Uinv T, the top block (Wtop, Wqtop) is produced here.
// Steps: (1) sign-choosing LU of Q1_top - S = L U (Ballard et al.), one barrier per pivot: every thread derives the pivot
// and its multipliers itself, the multipliers go to a separate array; (2) U^-1 and L^-1 by substitution, one column per
// lane with the column in registers (wave 0: U^-1, wave 1: L^-1); (3) T = -U S L^-T and (4) the four 32^3 products on the
// matrix cores, one product per wave.
typedef double d4l __attribute__((ext_vector_type(4)));

template <int NB>
__device__ __forceinline__ void small_mm(const double* __restrict__ Am, bool at, const double* __restrict__ Bm_, bool bt, int P,
                                         int lane, d4l (&acc)[NB / 16][NB / 16]) {
    // acc = op(A) op(B) for NB x NB matrices in LDS (pitch P); at / bt: use the transpose.  One wave.
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < NB / 16; ++ti)
#pragma unroll
        for (int tj = 0; tj < NB / 16; ++tj) acc[ti][tj] = d4l{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < NB / 4; ++ks) {
        const int k = ks * 4 + lk;
        double fa[NB / 16], fb[NB / 16];
#pragma unroll
        for (int t = 0; t < NB / 16; ++t) {
            const int i = t * 16 + li;
            fa[t] = at ? Am[k * P + i] : Am[i * P + k];
            fb[t] = bt ? Bm_[i * P + k] : Bm_[k * P + i];
        }
#pragma unroll
        for (int ti = 0; ti < NB / 16; ++ti)
#pragma unroll
            for (int tj = 0; tj < NB / 16; ++tj)
                acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ti], fb[tj], acc[ti][tj], 0, 0, 0);
    }
}

template <int NB>
__global__ __launch_bounds__(256) void lu_reconstruct_kernel(double* __restrict__ Ytop, int64_t rs, int64_t cs, int b,
                                                             double* __restrict__ Uinv, double* __restrict__ T,
                                                             double* __restrict__ UT, double* __restrict__ UTq,
                                                             double* __restrict__ Wtop, int64_t wrs, int64_t wcs,
                                                             double* __restrict__ Wqtop) {
    constexpr int P = NB + 1;
    __shared__ double Um[NB * P];      // work matrix, then U (zeros below the diagonal), then U S, then T
    __shared__ double Lm[NB * P];      // L (unit lower, zeros above)
    __shared__ double Ui[NB * P];      // U^-1
    __shared__ double Li[NB * P];      // L^-1
    __shared__ double sg[NB];
    double* const Tm = Um;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {
        double yv[NB * NB / 256];
#pragma unroll
        for (int t = 0; t < NB * NB / 256; ++t) {            // one memory round trip
            const int e = tid + 256 * t, i = e / NB, j = e % NB;
            yv[t] = (i < b && j < b) ? Ytop[i * rs + j * cs] : ((i == j) ? 0.0 : 0.0);
        }
#pragma unroll
        for (int t = 0; t < NB * NB / 256; ++t) {
            const int e = tid + 256 * t, i = e / NB, j = e % NB;
            Um[i * P + j] = yv[t];
            Lm[i * P + j] = (i == j) ? 1.0 : 0.0;
            Ui[i * P + j] = 0.0;
            Li[i * P + j] = 0.0;
        }
    }
    __syncthreads();
    // (1) LU with the sign choice  s_i = -sign(u_ii):  u_ii <- u_ii - s_i  (|pivot| >= 1)
    for (int i = 0; i < b; ++i) {
        const double bii = Um[i * P + i];
        const double sgn = (bii >= 0.0) ? -1.0 : 1.0, piv = bii - sgn, rp = fast_rcp(piv);
        const int rem = b - i - 1;
        for (int e = tid; e < rem * rem; e += 256) {
            const int r = i + 1 + e / rem, c = i + 1 + e % rem;
            const double l = Um[r * P + i] * rp;
            Um[r * P + c] -= l * Um[i * P + c];
            if (c == i + 1) Lm[r * P + i] = l;
        }
        __syncthreads();
        if (tid == 0) { sg[i] = sgn; Um[i * P + i] = piv; }
        if (tid > i && tid < b) Um[tid * P + i] = 0.0;       // column i below the pivot is L's now
    }
    if (tid >= b && tid < NB) { sg[tid] = 1.0; Um[tid * P + tid] = 1.0; }      // padding: identity block
    __syncthreads();
    // (2) one column per lane, the column held in registers
    if (wave == 0 && lane < NB) {
        const int j = lane;
        double x[NB], rd[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) rd[i] = fast_rcp(Um[i * P + i]);
#pragma unroll
        for (int i = NB - 1; i >= 0; --i) {
            double sa[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = i + 1; k < NB; ++k) sa[k & 3] += Um[i * P + k] * x[k];
            const double t = (sa[0] + sa[1]) + (sa[2] + sa[3]);
            x[i] = (i > j) ? 0.0 : ((i == j) ? rd[i] : -t * rd[i]);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) Ui[i * P + j] = x[i];
    } else if (wave == 1 && lane < NB) {
        const int j = lane;
        double x[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            double sa[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < i; ++k) sa[k & 3] += Lm[i * P + k] * x[k];
            const double t = (sa[0] + sa[1]) + (sa[2] + sa[3]);
            x[i] = (i < j) ? 0.0 : ((i == j) ? 1.0 : -t);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) Li[i * P + j] = x[i];
    }
    __syncthreads();
    for (int e = tid; e < NB * NB; e += 256) Um[(e / NB) * P + e % NB] *= sg[e % NB];      // U S, in place (U is done)
    __syncthreads();
    // (3) T = -(U S) L^-T, upper triangle
    const int li = lane & 15, lk = lane >> 4;
    d4l acc[NB / 16][NB / 16];
    if (wave == 0) small_mm<NB>(Tm, false, Li, true, P, lane, acc);
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int ti = 0; ti < NB / 16; ++ti)
#pragma unroll
            for (int tj = 0; tj < NB / 16; ++tj)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = ti * 16 + lk + 4 * r, j = tj * 16 + li;
                    const double t = (i <= j && j < b) ? -acc[ti][tj][r] : 0.0;
                    Tm[i * P + j] = t;
                    if (i < b && j < b) T[i * b + j] = t;
                }
    }
    __syncthreads();
    // (4) wave 0: UT = Uinv T^T, wave 1: UTq = Uinv T, wave 2: W_top = L T^T, wave 3: Wq_top = L T
    const double* left = (wave < 2) ? Ui : Lm;
    small_mm<NB>(left, false, Tm, (wave & 1) == 0, P, lane, acc);
#pragma unroll
    for (int ti = 0; ti < NB / 16; ++ti)
#pragma unroll
        for (int tj = 0; tj < NB / 16; ++tj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti * 16 + lk + 4 * r, j = tj * 16 + li;
                if (i < b && j < b) {
                    const double v = acc[ti][tj][r];
                    if (wave == 0) UT[i * b + j] = v;
                    else if (wave == 1) UTq[i * b + j] = v;
                    else if (wave == 2) Wtop[i * wrs + j * wcs] = v;
                    else Wqtop[i * rs + j * cs] = v;
                }
            }
    for (int e = tid; e < b * b; e += 256) {
        const int i = e / b, j = e % b;
        Uinv[e] = Ui[i * P + j];
        Ytop[i * rs + j * cs] = Lm[i * P + j];
    }
}

// rows r < nrows:  x = X(r, :b);  X(r,:) <- x S0 (in place),  W1(r,:) <- x S1,  W2(r,:) <- x S2   (all b x b, row-major).
// One workgroup per 256 rows.  Row-major operands (cs == 1) go through an LDS tile so that global loads and stores are
// full 256-byte rows (a thread writing its own row element by element costs 5x the bytes in partial-line writes:
// WRITE_SIZE 65.7 MB vs 12.6 MB algorithmic on the 16384 x 32 panel, profiles/r01_pmc_*); column-major operands are
// already coalesced across the threads of a wave.
template <int NB>
__global__ __launch_bounds__(256) void rows_times_small3_kernel(double* __restrict__ X, int64_t rs, int64_t cs, int64_t nrows,
                                                                int b, const double* __restrict__ S0, const double* __restrict__ S1,
                                                                const double* __restrict__ S2, double* __restrict__ W1, int64_t w1rs,
                                                                int64_t w1cs, double* __restrict__ W2) {
    constexpr int P = NB + 1;
    constexpr bool STAGE = (NB == 32);                   // the 64-wide (first-generation) panels keep the direct form
    __shared__ double Ss[3][NB * NB];
    __shared__ double tile[STAGE ? 256 * P : 1];
    const int tid = threadIdx.x;
    for (int e = tid; e < NB * NB; e += 256) {
        const int i = e / NB, j = e % NB;
        const bool in = (i < b && j < b);
        Ss[0][e] = in ? S0[i * b + j] : 0.0;
        Ss[1][e] = in ? S1[i * b + j] : 0.0;
        Ss[2][e] = in ? S2[i * b + j] : 0.0;
    }
    const int64_t r0 = (int64_t)blockIdx.x * 256;
    const int nr = (int)((nrows - r0 < 256) ? nrows - r0 : 256);
    const int64_t r = r0 + tid;
    const bool live = tid < nr;
    const bool xrow = STAGE && (cs == 1), wrow = STAGE && (w1cs == 1);
    double x[NB];
    if (xrow) {
        for (int e = tid; e < nr * b; e += 256) tile[(e / b) * P + e % b] = X[(r0 + e / b) * rs + e % b];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NB; ++i) x[i] = (live && i < b) ? tile[tid * P + i] : 0.0;
    } else {
#pragma unroll
        for (int i = 0; i < NB; ++i) x[i] = (live && i < b) ? X[r * rs + i * cs] : 0.0;
    }
    __syncthreads();                                     // Ss complete; tile free again
#pragma unroll 1
    for (int o = 0; o < 3; ++o) {
        double* dst = (o == 0) ? X : (o == 1) ? W1 : W2;
        const int64_t drs = (o == 1) ? w1rs : rs, dcs = (o == 1) ? w1cs : cs;
        const bool drow = (o == 1) ? wrow : xrow;
        const double* Sm = Ss[o];
        if (drow) {
            for (int j = 0; j < b; ++j) {
                double y = 0.0;
#pragma unroll
                for (int i = 0; i < NB; ++i) y += x[i] * Sm[i * NB + j];
                tile[tid * P + j] = y;
            }
            __syncthreads();
            for (int e = tid; e < nr * b; e += 256) dst[(r0 + e / b) * drs + e % b] = tile[(e / b) * P + e % b];
            __syncthreads();
        } else if (live) {
            for (int j = 0; j < b; ++j) {
                double y = 0.0;
#pragma unroll
                for (int i = 0; i < NB; ++i) y += x[i] * Sm[i * NB + j];
                dst[r * drs + j * dcs] = y;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ diagonal blocks
// One workgroup per diagonal block: Householder QR  D = Z Tri  with diag(Tri) >= 0.
template <int NB>
__global__ __launch_bounds__(256) void diag_qr_kernel(const double* __restrict__ A, int64_t rs, int64_t cs, int nb,
                                                      int64_t k, double* __restrict__ Zbuf, double* __restrict__ Tri, int* clear64) {
    constexpr int P = NB + 1;
    // the first launch after the last panel of the factorisation: leaves the stream's panel state block (64 words) clean for the
    // next call (cholqr_begin)
    if (clear64 && blockIdx.x == 0 && threadIdx.x < 64) clear64[threadIdx.x] = 0;
    __shared__ double D[NB * P];
    __shared__ double Z[NB * P];
    __shared__ double tau[NB];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int64_t j0 = (int64_t)p * nb;
    const int b = (int)((k - j0 < nb) ? k - j0 : nb);
    for (int e = tid; e < b * b; e += 256) {
        const int i = e / b, j = e % b;
        D[i * P + j] = A[(j0 + i) * rs + (j0 + j) * cs];
        Z[i * P + j] = (i == j) ? 1.0 : 0.0;
    }
    __syncthreads();
    // Householder QR with all 256 threads: thread (c, g) = (tid % NB, tid / NB) owns rows g, g + NG, ... of column c.
    // Per column one pass gives sum_{r>j} a_rj a_rc for every c (partials meet in LDS), from which the reflector and
    // its action follow; entries are first scaled to [0.5,1) by a power of two.
    constexpr int NG = 256 / NB;
    __shared__ double part[256];
    __shared__ double dscale;
    {
        double m = 0.0;
        for (int e = tid; e < b * b; e += 256) m = fmax(m, fabs(D[(e / b) * P + e % b]));
        part[tid] = m;
        __syncthreads();
        for (int k = 128; k > 0; k >>= 1) {
            if (tid < k) part[tid] = fmax(part[tid], part[tid + k]);
            __syncthreads();
        }
        if (tid == 0) {
            int ex = 0;
            if (part[0] > 0.0 && part[0] < 1.7e308) frexp(part[0], &ex);
            dscale = ldexp(1.0, ex);
        }
        __syncthreads();
        const double scl = 1.0 / dscale;
        for (int e = tid; e < b * b; e += 256) D[(e / b) * P + e % b] *= scl;
        __syncthreads();
    }
    const int c = tid % NB, g = tid / NB;
    // Fast path: the panel step hands over an orthonormal basis Q1 with span(Q1[:, :j]) = span(panel[:, :j]) (Cholesky-QR is a
    // triangular orthogonalisation), so the block D = S Q1^T A_panel is upper triangular already, up to
    // rounding (|d_ij| <~ eps ||a_j|| below the diagonal).  Then Z = I: dropping entries below 4e-15 of their column's norm is a
    // column-wise backward error of the size every other step of the factorisation makes, and it saves the 2 x 32 serial
    // Householder steps (50 us of pure latency per tn_qr call).  Anything else (64-wide first-generation panels) takes the general path.
    __shared__ int notri;
    if (tid == 0) notri = 0;
    __syncthreads();
    if (tid < b) {
        double below = 0.0, all2 = 0.0;
        for (int r = 0; r < b; ++r) {
            const double x = D[r * P + tid];
            all2 += x * x;
            if (r > tid) below = fmax(below, fabs(x));
        }
        if (!(below * below <= 1.6e-29 * all2)) notri = 1;          // (4e-15)^2; NaN lands here too
    }
    __syncthreads();
    const bool tri = (notri == 0);
    for (int j = 0; j < b && !tri; ++j) {
        double s = 0.0;
        if (c < b)
            for (int r = j + 1 + g; r < b; r += NG) s += D[r * P + j] * D[r * P + c];
        part[tid] = s;
        const double alpha = D[j * P + j], ajc = (c < b) ? D[j * P + c] : 0.0;
        __syncthreads();
        double sc = 0.0, sj = 0.0;
#pragma unroll
        for (int k = 0; k < NG; ++k) { sc += part[k * NB + c]; sj += part[k * NB + j]; }
        const double wj = alpha * alpha + sj;
        double t = 0.0;
        if (sj > 0.0 && wj > 1e-290) {                    // nothing below the diagonal -> H = I (like dlarfg)
            const double rn = fast_rsqrt(wj), nrm = wj * rn;
            const double beta = -copysign(nrm, alpha), d = alpha - beta, invd = fast_rcp(d);
            t = 1.0 + fabs(alpha) * rn;
            if (c > j && c < b) {
                const double f = t * (ajc + sc * invd);
                for (int r = j + 1 + g; r < b; r += NG) D[r * P + c] -= D[r * P + j] * invd * f;
                if (g == 0) D[j * P + c] = ajc - f;
            }
            __syncthreads();                               // column j is still needed unscaled by the updates above
            if (c == j) {
                for (int r = j + 1 + g; r < b; r += NG) D[r * P + j] *= invd;
                if (g == 0) D[j * P + j] = beta;
            }
        }
        if (tid == 0) tau[j] = t;
        __syncthreads();
    }
    for (int j = b - 1; j >= 0 && !tri; --j) {    // Z = H_0 ... H_{b-1}
        const double t = tau[j];
        if (t != 0.0) {                            // uniform
            double s = 0.0;
            if (c < b)
                for (int r = j + g; r < b; r += NG) s += ((r == j) ? 1.0 : D[r * P + j]) * Z[r * P + c];
            part[tid] = s;
            __syncthreads();
            double w = 0.0;
#pragma unroll
            for (int k = 0; k < NG; ++k) w += part[k * NB + c];
            w *= t;
            if (c < b)
                for (int r = j + g; r < b; r += NG) Z[r * P + c] -= ((r == j) ? 1.0 : D[r * P + j]) * w;
            __syncthreads();
        }
    }
    double* zo = Zbuf + (int64_t)p * nb * nb;
    double* to = Tri + (int64_t)p * nb * nb;
    for (int e = tid; e < b * b; e += 256) {
        const int i = e / b, j = e % b;
        const double sj = (D[j * P + j] < 0.0) ? -1.0 : 1.0, si = (D[i * P + i] < 0.0) ? -1.0 : 1.0;
        zo[i * nb + j] = Z[i * P + j] * sj;                  // column j of Z scaled
        to[i * nb + j] = (i <= j) ? D[i * P + j] * si * dscale : 0.0; // row i of Tri scaled (and un-normalised)
    }
}

// R[i][j]: 0 left of the diagonal block, Tri inside it, Z^T A to the right;  Q starts as [Z; 0] (block diagonal Z).
// Both only wait for diag_qr_kernel, so they share one launch: the first nR workgroups write R, the rest Q.
// With fold_b > 0 the LAST panel's reflector is applied on the way (single-level path): its columns of Q are
//     H_p [Z_p; 0] = [Z_p; 0] - (Y_p T_p) (Ytop_p^T Z_p),
// a b x b product every workgroup forms for itself in LDS -- two GEMM launches less per factorisation, and for a one-panel
// factorisation no Q accumulation at all.  Y / Wq: the reflectors and Y T of all panels (strides yrs / ycs), j0f: first column of the
// last panel.
__global__ __launch_bounds__(256) void assemble_R_init_Q_kernel(const double* __restrict__ A, int64_t rs, int64_t cs, int nb, int64_t k, int64_t n,
                                                                const double* __restrict__ Zbuf, const double* __restrict__ Tri,
                                                                double* __restrict__ R, int64_t rrs, int64_t rcs, unsigned nR,
                                                                double* __restrict__ Q, int64_t qrs, int64_t qcs, int64_t m, int colfast,
                                                                const double* __restrict__ Y, const double* __restrict__ Wq, int64_t yrs,
                                                                int64_t ycs, int64_t j0f, int fold_b) {
    if (blockIdx.x < nR) {
        const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (e >= k * n) return;
        const int64_t i = e / n, j = e % n;
        const int64_t p = i / nb, j0 = p * nb;
        const int b = (int)((k - j0 < nb) ? k - j0 : nb);
        const int il = (int)(i - j0);
        double v = 0.0;
        if (j >= j0 + b) {
            const double* z = Zbuf + p * nb * nb;
            if (nb == 32) {                                  // fixed trip count: the 2 x 32 loads go out together (one round trip, not 32)
                double zv[32], av[32];
#pragma unroll
                for (int r = 0; r < 32; ++r) {
                    zv[r] = (r < b) ? z[r * 32 + il] : 0.0;
                    av[r] = (r < b) ? A[(j0 + r) * rs + j * cs] : 0.0;
                }
#pragma unroll
                for (int r = 0; r < 32; ++r) v += zv[r] * av[r];
            } else {
                for (int r = 0; r < b; ++r) v += z[r * nb + il] * A[(j0 + r) * rs + j * cs];
            }
        } else if (j >= j0) {
            v = Tri[p * nb * nb + il * nb + (j - j0)];
        }
        R[i * rrs + j * rcs] = v;
    } else {
        __shared__ double Ms[32 * 33];
        if (fold_b > 0) {                                   // M = Ytop^T Z of the last panel (uniform branch)
            const double* z = Zbuf + (j0f / nb) * nb * nb;
            for (int e = threadIdx.x; e < fold_b * fold_b; e += 256) {
                const int c = e / fold_b, jj = e % fold_b;
                double yv[32], zv[32];
#pragma unroll
                for (int r = 0; r < 32; ++r) {
                    yv[r] = (r < fold_b) ? Y[(j0f + r) * yrs + (j0f + c) * ycs] : 0.0;
                    zv[r] = (r < fold_b) ? z[r * nb + jj] : 0.0;
                }
                double acc = 0.0;
#pragma unroll
                for (int r = 0; r < 32; ++r) acc += yv[r] * zv[r];
                Ms[c * 33 + jj] = acc;
            }
            __syncthreads();
        }
        const int64_t e = (int64_t)(blockIdx.x - nR) * 256 + threadIdx.x;
        if (e >= m * k) return;
        const int64_t i = colfast ? e / k : e % m, j = colfast ? e % k : e / m;
        double v = 0.0;
        if (i < k && i / nb == j / nb) {
            const int64_t p = i / nb;
            v = Zbuf[p * nb * nb + (i - p * nb) * nb + (j - p * nb)];
        }
        if (fold_b > 0 && j >= j0f && i >= j0f) {
            const int jj = (int)(j - j0f);
            double wv[32];
#pragma unroll
            for (int c = 0; c < 32; ++c) wv[c] = (c < fold_b) ? Wq[i * yrs + (j0f + c) * ycs] : 0.0;      // together: one round trip
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < 32; ++c) acc += wv[c] * ((c < fold_b) ? Ms[c * 33 + jj] : 0.0);
            v -= acc;
        }
        Q[i * qrs + j * qcs] = v;
    }
}

// out[j] = sum_i A(i,j)^2 for the columns of an (m x n) block (the host takes the maximum: no atomics, nothing to pre-zero)
__global__ __launch_bounds__(256) void colnorm2_kernel(const double* __restrict__ A, int64_t rs, int64_t cs, int64_t m,
                                                       int64_t n, double* __restrict__ out) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t j = blockIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int64_t i = tid;
    for (; i + 768 < m; i += 1024) {                      // four independent loads in flight
        const double x0 = A[i * rs + j * cs], x1 = A[(i + 256) * rs + j * cs], x2 = A[(i + 512) * rs + j * cs],
                     x3 = A[(i + 768) * rs + j * cs];
        s0 += x0 * x0; s1 += x1 * x1; s2 += x2 * x2; s3 += x3 * x3;
    }
    for (; i < m; i += 256) { const double x = A[i * rs + j * cs]; s0 += x * x; }
    double s = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) out[j] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- tiny factorisations in ONE workgroup -----------------------------------------------------------------------------------
// A sweep makes ~450 factorisations of at most 4096 elements (1 x 1 edge sites, 16 x 16, 256 x 16 ...): through the blocked path
// each is a dozen launches, ~100 us of pure launch latency.  Here: the matrix in LDS, Householder QR column by column with all 256
// threads (thread (c, g) = column c, row group g; per column one pass gives sum_{r>j} a_rj a_rc for every c, from which the
// reflector and its action follow -- the scheme of diag_qr_kernel), backward accumulation of Q = H_0 ... H_{k-1} [I; 0], signs
// chosen so that diag(R) >= 0.  Entries are first scaled into [0.5, 1) by a power of two.  m n <= 4096, k = min(m, n) <= 32.
__global__ __launch_bounds__(256) void tiny_qr_kernel(const double* __restrict__ A, int64_t rs, int64_t cs, int m, int n, double* __restrict__ Q,
                                                      int64_t qrs, int64_t qcs, double* __restrict__ R, int64_t rrs, int64_t rcs) {
    __shared__ double As[4096];          // m x n, pitch n; below the diagonal: the reflectors (unit diagonal implied)
    __shared__ double Qs[4096];          // m x k, pitch k
    __shared__ double scol[4096];        // per column: sum over the rows below the pivot row
    __shared__ double part[256];
    __shared__ double taus[32];
    __shared__ double dscale_s;
    const int tid = threadIdx.x;
    const int k = m < n ? m : n;
    {
        double mx = 0.0;
        double xv[16];                                       // m n <= 4096 = 16 x 256: one memory round trip for the whole matrix
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = tid + 256 * u;
            xv[u] = (e < m * n) ? A[(int64_t)(e / n) * rs + (int64_t)(e % n) * cs] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int e = tid + 256 * u;
            if (e < m * n) {
                As[e] = xv[u];
                const double a = fabs(xv[u]);
                mx = (a == a) ? fmax(mx, a) : 1.7e308;
            }
        }
        part[tid] = mx;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (tid < h) part[tid] = fmax(part[tid], part[tid + h]);
            __syncthreads();
        }
        if (tid == 0) {
            int ex = 0;
            if (part[0] > 0.0 && part[0] < 1.7e308) frexp(part[0], &ex);
            dscale_s = ldexp(1.0, ex);
        }
        __syncthreads();
        const double scl = 1.0 / dscale_s;
        for (int e = tid; e < m * n; e += 256) As[e] *= scl;
        __syncthreads();
    }
    // columns over NC thread-columns (a power of two >= n, at most 256), rows over NG = 256 / NC groups
    int NC = 16;
    while (NC < n && NC < 256) NC <<= 1;
    const int NG = 256 / NC;
    const int cc = tid % NC, g = tid / NC;
    for (int j = 0; j < k; ++j) {
        for (int c = cc; c < n; c += NC) {
            double acc = 0.0;
            if (c >= j)
                for (int r = j + 1 + g; r < m; r += NG) acc += As[r * n + j] * As[r * n + c];
            if (NG > 1) part[g * NC + cc] = acc;             // (NG > 1 means n <= NC: one column per thread-column)
            else scol[c] = acc;
        }
        __syncthreads();
        if (NG > 1 && g == 0 && cc < n) {
            double acc = 0.0;
            for (int h = 0; h < NG; ++h) acc += part[h * NC + cc];
            scol[cc] = acc;
        }
        __syncthreads();
        const double alpha = As[j * n + j], sigma = scol[j];
        double tau = 0.0, beta = alpha, inv = 0.0;
        if (sigma > 0.0 && alpha * alpha + sigma > 1e-290) {     // nothing below the diagonal -> H = I (like dlarfg)
            const double nrm = sqrt(alpha * alpha + sigma);
            beta = -copysign(nrm, alpha);
            tau = (beta - alpha) / beta;
            inv = 1.0 / (alpha - beta);
        }
        double wreg[16];                                          // w_c of this thread's columns (n <= 4096 = 16 x 256)
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int c = cc + NC * u;
            wreg[u] = (c < n && c > j) ? tau * (As[j * n + c] + inv * scol[c]) : 0.0;
        }
        __syncthreads();                                          // row j is rewritten below
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int c = cc + NC * u;
            if (c < n && c > j && tau != 0.0) {
                const double w = wreg[u];
                for (int r = j + 1 + g; r < m; r += NG) As[r * n + c] -= As[r * n + j] * inv * w;
                if (g == 0) As[j * n + c] -= w;
            }
        }
        __syncthreads();                                          // column j was read unscaled by the updates above
        for (int r = j + 1 + tid; r < m; r += 256) As[r * n + j] *= inv;
        if (tid == 0) { As[j * n + j] = beta; taus[j] = tau; }
        __syncthreads();
    }
    // Q = H_0 ... H_{k-1} [I; 0]
    for (int e = tid; e < m * k; e += 256) Qs[e] = (e / k == e % k) ? 1.0 : 0.0;
    __syncthreads();
    int NQ = 16;
    while (NQ < k) NQ <<= 1;
    const int NGq = 256 / NQ, cq = tid % NQ, gq = tid / NQ;
    for (int j = k - 1; j >= 0; --j) {
        const double tau = taus[j];
        if (tau != 0.0) {                                         // uniform
            double acc = 0.0;
            if (cq >= j && cq < k)
                for (int r = j + 1 + gq; r < m; r += NGq) acc += As[r * n + j] * Qs[r * k + cq];
            part[gq * NQ + cq] = acc;
            __syncthreads();
            double w = 0.0;
            if (cq >= j && cq < k) {
                for (int h = 0; h < NGq; ++h) w += part[h * NQ + cq];
                w = tau * (Qs[j * k + cq] + w);
            }
            __syncthreads();
            if (cq >= j && cq < k) {
                for (int r = j + 1 + gq; r < m; r += NGq) Qs[r * k + cq] -= As[r * n + j] * w;
                if (gq == 0) Qs[j * k + cq] -= w;
            }
            __syncthreads();
        }
    }
    const double ds = dscale_s;
    for (int e = tid; e < k * n; e += 256) {
        const int i = e / n, c = e % n;
        const double sg = (As[i * n + i] < 0.0) ? -1.0 : 1.0;
        R[(int64_t)i * rrs + (int64_t)c * rcs] = (c >= i) ? sg * As[i * n + c] * ds : 0.0;
    }
    if (Q)
        for (int e = tid; e < m * k; e += 256) {
            const int r = e / k, j = e % k;
            const double sg = (As[j * n + j] < 0.0) ? -1.0 : 1.0;
            Q[(int64_t)r * qrs + (int64_t)j * qcs] = sg * Qs[e];
        }
}

// ------------------------------------------------------------------------------------------ driver
// TN_DEBUG=1: synchronise after each stage and report the first non-finite intermediate (diagnostics only)
static bool dbg_on() { static const bool on = env_flag_set("TN_DEBUG"); return on; }
static void dbg_check(hipStream_t st, const double* p, int64_t rs, int64_t cs, int64_t m, int64_t n, const char* what, int panel, int it) {
    if (!dbg_on()) return;
    std::vector<double> h((size_t)(m * n));
    (void)hipStreamSynchronize(st);
    for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < n; ++j) (void)hipMemcpy(&h[i * n + j], p + i * rs + j * cs, 8, hipMemcpyDeviceToHost);
    double mx = 0, mn = 1e300; int bad = 0;
    for (double v : h) { if (!(v == v) || v > 1e300 || v < -1e300) ++bad; else { double a = v < 0 ? -v : v; if (a > mx) mx = a; if (a < mn) mn = a; } }
    fprintf(stderr, "[tn_qr dbg] panel %d it %d %-10s %lldx%lld nonfinite=%d max=%.3e min|.|=%.3e\n", panel, it, what, (long long)m, (long long)n, bad, mx, mn);
}

constexpr int QR_NBO_MAX = 256;       // widest outer block of the two-level factorisation
struct QrWs {
    double *Y, *Wq, *W, *UT, *UTq;
    double *G, *Tblk, *Zo, *Zo2, *tmpT;
    double *T, *X, *part, *Js, *Uinv, *Z, *Tri, *gemm_ws, *cn;
    int* dead;
    int* pairs;          // swap list of the pivoted panel step (2 nb ints)
    char* piv;           // PivState + int permutation (device-side panel pivoting)
    int64_t gemm_ws_bytes;
    void* panel_ws;      // workspace of the Cholesky-QR panel step (cholqr.hip)
    int64_t panel_bytes;
    void* cq_state = nullptr;      // the stream's panel state block (cholqr_begin), or NULL = head of panel_ws
};

static int64_t qr_layout(int64_t m, int64_t n, int nb, char* base, QrWs* w) {
    const int64_t k = m < n ? m : n, P = cdiv(k, nb);
    WsCarve ws{base};
    double* Y = ws.take<double>(m * k * 8);
    double* Wq = ws.take<double>(m * k * 8);            // Y T of every panel (Q accumulation)
    double* Wp = ws.take<double>(m * nb * 8);           // Y T^T of the current panel (trailing update)
    double* UT = ws.take<double>((int64_t)nb * nb * 8);
    double* UTq = ws.take<double>((int64_t)nb * nb * 8);
    double* T = ws.take<double>(P * nb * nb * 8);
    double* X = ws.take<double>((int64_t)nb * (n > k ? n : k) * 8);
    double* part = ws.take<double>((int64_t)64 * nb * nb * 8);
    double* Js = ws.take<double>((int64_t)nb * nb * 8);
    double* Uinv = ws.take<double>((int64_t)nb * nb * 8);
    double* Z = ws.take<double>(P * nb * nb * 8);
    double* Tri = ws.take<double>(P * nb * nb * 8);
    int* dead = ws.take<int>(nb * 4);
    double* cn = ws.take<double>(2 * n * 8);            // column norms^2: [input | current trailing block]
    int* pairs = ws.take<int>((int64_t)2 * nb * 4);
    char* piv = ws.take<char>(1024 + n * 4);           // PivState | permutation (int) of the device-side panel pivoting
    // split-K scratch for the tall TN products (b x n, K = m)
    int64_t gw = (int64_t)64 * nb * (n > k ? n : k) * 8;      // upper bound of pick_splitk's partial buffers
    {   // ... and of the outer-block products (NBO x n', K = m) of the two-level path: pick_splitk asks for about 512 tiles of
        // 128 x 128 whatever n' is (s = ceil(512 / tiles)), i.e. <= (512 + tiles) 128^2 doubles; take that bound for the widest case
        const int64_t tiles = cdiv(QR_NBO_MAX, 128) * cdiv(n > k ? n : k, 128);
        const int64_t g2 = (512 + 2 * tiles) * 128 * 128 * 8;
        if (g2 > gw) gw = g2;
    }
    double* gws = ws.take<double>(gw + 256);
    // two-level blocking: Gram of an outer block, its merged T factors (one per block), the two (NBO x n) operands of the
    // outer update and a scratch for the T recurrence
    const int64_t nblk_o = cdiv(k, QR_NBO_MAX / 2);           // enough for the narrowest outer width used (128)
    double* Gm = ws.take<double>((int64_t)QR_NBO_MAX * QR_NBO_MAX * 8);
    double* Tblk = ws.take<double>(nblk_o * QR_NBO_MAX * QR_NBO_MAX * 8);
    double* Zb = ws.take<double>((int64_t)QR_NBO_MAX * (n > k ? n : k) * 8);
    double* Zb2 = ws.take<double>((int64_t)QR_NBO_MAX * (n > k ? n : k) * 8);
    double* tmpT = ws.take<double>((int64_t)QR_NBO_MAX * 64 * 8);
    if (w) { w->G = Gm; w->Tblk = Tblk; w->Zo = Zb; w->Zo2 = Zb2; w->tmpT = tmpT; }
    const int64_t pb = cholqr_ws_bytes(m, nb < 32 ? nb : 32);
    void* pw = ws.take(pb);
    if (w) { w->panel_ws = pw; w->panel_bytes = pb; }
    if (w) { w->Wq = Wq; w->W = Wp; w->UT = UT; w->UTq = UTq; }
    if (w) { w->Y = Y; w->T = T; w->X = X; w->part = part; w->Js = Js; w->Uinv = Uinv; w->Z = Z; w->Tri = Tri;
             w->dead = dead; w->gemm_ws = gws; w->gemm_ws_bytes = gw; w->cn = cn; w->pairs = pairs; w->piv = piv; }
    return ws.total();
}

int64_t qr_ws_bytes(int64_t m, int64_t n, int nb) { return qr_layout(m, n, nb, nullptr, nullptr); }
// ------------------------------------------------------------------------------------------ host driver: a call record, stages, qr_factor_impl
// One call of qr_factor: filled once, read by every stage below.
struct QrCall {
    hipStream_t st;
    double* A; int64_t rs, cs, m, n; double* Q; int64_t qrs, qcs; double* R; int64_t rrs, rcs;
    int nb; void* ws; int64_t ws_bytes; double rank_tol;
    int64_t* keff_host; double* dropped2_host; int frob_exit; int64_t* pivot_perm_host; double* nf_out2; int* nf_done; bool* input_intact;
};
// What the blocked paths derive from the call, once (the single-launch exits leave before it is filled).
struct QrState {
    QrWs w;
    bool pivot, reveal, rowmajor, ru_on, wform;      // pivot: panel pivoting; reveal: the rank-revealing check of every second panel
    int64_t yrs, ycs, wrs, wcs;          // strides of Y (and of the m x k array of W) / of the one-panel W of the 64-wide and two-level paths
    Mat Am, Ym, Wqm;
    int fbase = 0;                       // arrivals booked by the single-launch panel steps of this call (cholqr.hip)
    double scale2 = -1.0;                // measure of the input the exit tests compare with (lazily read back)
};
// The operands of one panel step
struct QrPanel {
    int p, b; int64_t j0, mp;            // number of the panel in the whole factorisation, its width; first row and column, rows from there on (m - j0)
    Mat Ap, Yp, Wp, Wqp;                 // A[j0:, j0:], Y[j0:, j0:], the W = Y T^T of the trailing update, the panel's place in the m x k array
    double* Tp;
};
static QrPanel panel_at(const QrCall& c, const QrState& s, int p, int64_t kend) {
    QrPanel pn;
    pn.p = p, pn.j0 = (int64_t)p * c.nb, pn.mp = c.m - pn.j0;
    pn.b = (int)((kend - pn.j0 < c.nb) ? kend - pn.j0 : c.nb);
    pn.Ap = sub(s.Am, pn.j0, pn.j0), pn.Yp = sub(s.Ym, pn.j0, pn.j0), pn.Wqp = sub(s.Wqm, pn.j0, pn.j0);
    // fused: W_p = Y_p T_p^T of EVERY panel is kept (in the m x k array that holds Y T for nb = 64): besides the trailing update it
    // serves the Q accumulation, H_p Q = Q - Y_p (W_p^T Q), so Y T is never formed (a third of the panel step's output)
    pn.Wp = s.wform ? pn.Wqp : mat(s.w.W, s.wrs, s.wcs);
    pn.Tp = s.w.T + (int64_t)p * c.nb * c.nb;
    return pn;
}
// one launch of 256-thread workgroups on the call's stream, booked under PROF_QR_AUX; a launch error ends the stage that made it
#define QR_LAUNCH(c, kernel, grid, ...) \
    do { TN_PROF_LAUNCH((c).st, PROF_QR_AUX, hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (c).st, __VA_ARGS__)); TN_CHECK_LAUNCH(#kernel); } while (0)
// ---- the ending: triangularise the diagonal blocks, assemble R, start Q (in front of the other stages: the file's kernels are emitted in order of first launch)
static int triangularise_diag(const QrCall& c, QrState& s, int64_t k, int P) {      // (32-wide panels; the 64-wide path launches its own form)
    QR_LAUNCH(c, (diag_qr_kernel<32>), dim3(P), c.A, c.rs, c.cs, c.nb, k, s.w.Z, s.w.Tri, (int*)s.w.cq_state);
    if (s.w.cq_state) cholqr_end_ok(c.st);
    return 0;
}
// The last panel's reflector applied by the launch that writes [Z; 0]:  Q[jf:, jf:] = [Z; 0] - second (first_top^T Z),  b columns (0: none)
struct QrFold { const double *first, *second; int64_t rs, cs, jf; int b; };
static int assemble_R_init_Q(const QrCall& c, QrState& s, int64_t k, const QrFold& f) {
    const int qcolfast = (c.qcs == 1) ? 1 : 0;
    const unsigned nR = (unsigned)cdiv(k * c.n, 256), nQ = (unsigned)cdiv(c.m * k, 256);
    QR_LAUNCH(c, assemble_R_init_Q_kernel, dim3(nR + nQ), c.A, c.rs, c.cs, c.nb, k, c.n, s.w.Z, s.w.Tri, c.R, c.rrs, c.rcs, nR, c.Q, c.qrs, c.qcs, c.m, qcolfast,
              f.first, f.second, f.rs, f.cs, f.jf, f.b);
    return 0;
}
// Selection of the b largest residuals among positions 0 .. ntr-1 by successive swaps (step t: the first maximum of positions
// t .. ntr-1 goes to position t), through a tournament tree over the positions instead of b linear scans (the scans cost 30 us of
// host time per panel with the device idle): leaf i = position i, a node keeps the position of the larger value, the left one on
// ties (= the first maximum of a scan); a placed position is retired with -infinity.  hcn is permuted along; perm (offset j0) too;
// pairs receives the b swaps (absolute column numbers) for swap_columns_kernel.
static void select_pivots(double* hcn, int64_t ntr, int b, int64_t j0, int64_t* perm, int* pairs) {
    int sz = 1;
    while (sz < ntr) sz <<= 1;
    thread_local std::vector<int> tree;
    thread_local std::vector<double> val;
    tree.assign((size_t)2 * sz, -1);
    val.assign((size_t)sz, -1.0);                   // squared norms are >= 0: -1 never wins
    for (int64_t j = 0; j < ntr; ++j) { val[j] = (hcn[j] == hcn[j]) ? hcn[j] : -1.0; tree[sz + j] = (int)j; }   // NaN never wins (as in a scan)
    auto better = [&](int a, int c) { return (a >= 0 && (c < 0 || val[a] >= val[c])) ? a : c; };
    for (int i = sz - 1; i >= 1; --i) tree[i] = better(tree[2 * i], tree[2 * i + 1]);
    auto update = [&](int pos) { for (int i = (sz + pos) >> 1; i >= 1; i >>= 1) tree[i] = better(tree[2 * i], tree[2 * i + 1]); };
    for (int t = 0; t < b; ++t) {
        int arg = tree[1];                            // leftmost maximum of the live positions t .. ntr-1
        if (arg < 0) arg = t;
        std::swap(hcn[t], hcn[arg]);
        std::swap(perm[j0 + t], perm[j0 + arg]);
        pairs[2 * t] = (int)(j0 + t);
        pairs[2 * t + 1] = (int)(j0 + arg);
        if (arg != t) { val[arg] = (hcn[arg] == hcn[arg]) ? hcn[arg] : -1.0; update(arg); }
        val[t] = -2.0;                                // position t is placed
        tree[sz + t] = -1;
        update(t);
    }
}

// ---- panel pivoting decided on the device ---------------------------------------------------------------------------------------
// The host-side selection above cost a read-back of the residual norms, a stream synchronisation and the host's tournament per panel --
// ~25 us of idle device in the one phase of a row where the host was still inside the chain (2 550 panels per sweep).  Here ONE workgroup
// takes the decisions: it adds the residual norms up (fixed order), applies the exit test, ranks the columns (rank counting in LDS), turns
// the b largest into the same "successive swaps" the host made (step t: the t-th largest goes to position t) and leaves the moves they
// amount to, the permutation and the verdict in device memory.  Every later launch of the factorisation -- column swap, panel step,
// trailing update -- looks at `active` and returns at once after the exit.  The host runs one panel ahead: it reads the verdict of panel
// p - 1 (32 bytes, copied behind the selection launch) before it enqueues panel p, so an exit costs one panel's worth of empty launches
// instead of a synchronisation per panel.  Ties between equal norms go to the lower ORIGINAL position (the host took the lower CURRENT
// one): only exact ties differ.  TN_PIVOT_DEVICE=0 keeps the host selection.
struct PivHead { int active, k_exit, stamp, swap_n; double scale2, dropped2; };      // what the host reads back (32 bytes)
struct PivState { PivHead h; int ticket; int pad[3]; int sel[32]; int dst[64]; int src[64]; };
constexpr int PIV_MAXN = 4096;
__device__ __forceinline__ void piv_sti(int* q, int v) { __hip_atomic_store((__attribute__((address_space(1))) int*)q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int piv_ldi(const int* q) { return __hip_atomic_load((const __attribute__((address_space(1))) int*)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__global__ __launch_bounds__(256) void pivot_init_kernel(PivState* S, int* __restrict__ perm, int n) {      // once per factorisation
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) perm[i] = i;
    if (i < (int)(sizeof(PivState) / 4)) ((int*)S)[i] = 0;
}
// grid = ceil(ntr / 16) workgroups.  Every workgroup adds up all norms (same order: same sum everywhere) and applies the exit test; then it
// ranks ITS 16 columns against all (16 threads per column, a sixteenth of the comparisons each -- fp64 compares: the loop is VALU-bound)
// and publishes the ones among the b largest; the last workgroup to finish (ticket) turns the selection into moves with one wave:
//   position t < b receives the t-th largest column; the front columns that are not selected go, in ascending order, to the positions
//   the selected columns from behind the front vacate, in ascending order; nothing else moves.
// The kernel is a chain of dependent memory round trips (~2 us each): state and norms are fetched together, the permutation is
// brought up to date by the column swap that follows (swap_columns_dev_kernel), not here.
// mail (page-locked HOST memory): the verdict for the host as ONE 8-byte word, (stamp << 32) | (active << 31) | columns accepted, written
// with a relaxed system-scope store -- no copy launch, no event, no release fence; the dropped norm is read at the end of the call
struct PivMail { unsigned long long word; };
__device__ __forceinline__ void piv_post(PivMail* mail, int active, int k_exit, unsigned stamp) {
    const unsigned long long w = ((unsigned long long)stamp << 32) | ((unsigned long long)(active ? 1u : 0u) << 31) | (unsigned long long)(unsigned)k_exit;
    __hip_atomic_store(&mail->word, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
constexpr int PIV_CPB = 16;         // columns per workgroup
__global__ __launch_bounds__(256) void pivot_select_kernel(const double* __restrict__ cn, int ntr, int b, int j0, int p, double tol2, PivState* S,
                                                           PivMail* mail, unsigned stamp) {
    __shared__ double v[PIV_MAXN];
    __shared__ double red[256];
    __shared__ int cnt[16][PIV_CPB];
    __shared__ int vpos[32];
    __shared__ int s_last;
    const int tid = threadIdx.x, blk = blockIdx.x, nblk = gridDim.x;
    // one round trip: the state words and this thread's norms
    const int act = (p > 0) ? S->h.active : 1;
    const double scale_prev = (p > 0) ? S->h.scale2 : 0.0;
    double part = 0.0;
    for (int j = tid; j < ntr; j += 256) {
        const double x = cn[j];
        part += x;                                            // (a NaN stays a NaN in the sum: the exit test then fails, as on the host)
        v[j] = (x == x) ? x : -1.0;                           // ... and never wins a selection
    }
    if (act == 0) {                                           // (written by an earlier launch: the same answer in every workgroup)
        if (blk == 0 && tid == 0) piv_post(mail, 0, S->h.k_exit, stamp);
        return;
    }
    red[tid] = part;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) { if (tid < k) red[tid] += red[tid + k]; __syncthreads(); }
    const double fro2 = red[0];
    const double scale2 = (p == 0) ? fro2 : scale_prev;
    if (p > 0 && fro2 <= tol2 * scale2) {                     // what is left is below the threshold: stop before this panel
        if (blk == 0 && tid == 0) {
            S->h.k_exit = j0; S->h.dropped2 = fro2; S->h.stamp = p + 1; S->h.swap_n = 0; S->h.active = 0;
            piv_post(mail, 0, j0, stamp);
        }
        return;
    }
    {
        const int c = tid & (PIV_CPB - 1), q = tid / PIV_CPB, j = blk * PIV_CPB + c;       // q: 0 .. 15
        const double mine = j < ntr ? v[j] : -2.0;
        const int chunk = (ntr + 15) >> 4, i0 = q * chunk, i1 = (i0 + chunk < ntr) ? i0 + chunk : ntr;
        int r = 0;
        int i = i0;
        for (; i + 8 <= i1; i += 8) {                         // eight LDS reads in flight
            double o[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) o[u] = v[i + u];
#pragma unroll
            for (int u = 0; u < 8; ++u) r += (o[u] > mine || (o[u] == mine && i + u < j)) ? 1 : 0;
        }
        for (; i < i1; ++i) { const double o = v[i]; r += (o > mine || (o == mine && i < j)) ? 1 : 0; }
        cnt[q][c] = r;
        __syncthreads();
        if (q == 0 && j < ntr) {
            int rank = 0;
#pragma unroll
            for (int u = 0; u < 16; ++u) rank += cnt[u][c];
            if (rank < b) piv_sti(&S->sel[rank], j);
        }
    }
    // (the selections are agent-scope stores: they go through to memory, the publisher only waits for their completion -- no release
    //  fence, which would write back the XCD's L2; the last workgroup reads them with agent-scope loads)
    publish_wait();
    __syncthreads();
    if (tid == 0) s_last = (atomicAdd(&S->ticket, 1) == nblk - 1) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    const int lane = tid;                                     // (the first wave decides; the barriers below are reached by all 256 threads)
    const int st = (lane < b) ? piv_ldi(&S->sel[lane]) : -1;  // original trailing position of the lane-th largest column
    bool selfront = false;
    int rankV = 0;
    const bool isV = lane < b && st >= b;
    if (lane < 64) {
        for (int t = 0; t < b; ++t) {
            const int x = __shfl(st, t, 64);
            selfront = selfront || x == lane;
            rankV += (isV && x >= b && x < st) ? 1 : 0;
        }
    }
    const bool isD = lane < b && !selfront;
    const bool mv1 = lane < b && st != lane;
    unsigned long long bD = 0ull, b1 = 0ull;
    if (lane < 64) {
        // safety net: the b selections must be b distinct trailing positions.  They feed the column moves of the next launch, where a
        // wrong index would be an out-of-range access; a selection that is not a valid set (never seen; it would mean a published
        // selection was not visible to this workgroup) stops the factorisation with an error mark instead (stamp < 0, read by the host)
        bool dup = false;
        for (int t = 0; t < b; ++t) { const int x = __shfl(st, t, 64); dup = dup || (t != lane && x == st); }
        const bool wrong = lane < b && (st < 0 || st >= ntr || dup);
        const unsigned long long bw = __ballot(wrong);
        if (lane == 0) s_last = (bw != 0ull) ? 2 : 1;
        bD = __ballot(isD); b1 = __ballot(mv1);
    }
    if (isV && rankV < 32) vpos[rankV] = st;
    __syncthreads();
    if (s_last == 2) {
        if (tid == 0) {
            S->ticket = 0;
            S->h.swap_n = 0; S->h.k_exit = j0; S->h.stamp = -(p + 1); S->h.dropped2 = 0.0; S->h.active = 0;
            piv_post(mail, 0, j0, stamp);
        }
        return;
    }
    const unsigned long long below = (lane < 64) ? ((1ull << lane) - 1ull) : 0ull;
    const int n1 = __popcll(b1), nD = __popcll(bD);
    if (mv1) { const int i = __popcll(b1 & below); S->dst[i] = j0 + lane; S->src[i] = j0 + st; }
    if (isD) { const int i = __popcll(bD & below); S->dst[n1 + i] = j0 + vpos[i]; S->src[n1 + i] = j0 + lane; }
    if (tid == 0) {
        S->ticket = 0;
        S->h.swap_n = n1 + nD;
        S->h.k_exit = j0 + b;
        S->h.stamp = p + 1;
        if (p == 0) { S->h.scale2 = fro2; S->h.dropped2 = 0.0; }
        S->h.active = 1;
        piv_post(mail, 1, j0 + b, stamp);
    }
}
// the moves of the selection applied to every row: 64 rows per workgroup, the (at most 64) moves dealt to 4 threads per row, all values
// of a workgroup's rows fetched before the first one is stored (the moves permute columns: sources and destinations overlap)
// (the workgroup after the last one applies the moves to the permutation: perm[dst] <- perm[src])
__global__ __launch_bounds__(256) void swap_columns_dev_kernel(double* __restrict__ A, int64_t rs, int64_t cs, int64_t m, const PivState* __restrict__ S,
                                                               int* __restrict__ perm) {
    // (header and move list are fetched together -- one memory round trip instead of two before the first row load; entries beyond swap_n
    //  are stale but in range of the array and never used)
    const int g = threadIdx.x >> 6;
    int src[16], dst[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { src[i] = S->src[g * 16 + i]; dst[i] = S->dst[g * 16 + i]; }
    const int active = S->h.active, ns = S->h.swap_n;
    if (active == 0 || ns <= 0 || ns > 64) return;
    if (blockIdx.x == gridDim.x - 1) {
        int old = 0;
        if ((int)threadIdx.x < ns) old = perm[S->src[threadIdx.x]];
        __syncthreads();
        if ((int)threadIdx.x < ns) perm[S->dst[threadIdx.x]] = old;
        return;
    }
    const int64_t r = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
    const bool in = r < m;
    double* row = A + (in ? r : 0) * rs;
    double v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { const int t = g * 16 + i; v[i] = (in && t < ns) ? row[(int64_t)src[i] * cs] : 0.0; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) { const int t = g * 16 + i; if (in && t < ns) row[(int64_t)dst[i] * cs] = v[i]; }
}

// ---- Q accumulation through merged reflectors (round 5) ---------------------------------------------------------------------
// The single-level paths used to apply every 32-wide reflector to Q on its own: per panel a split-K product Y_p^T Q, its reduction and a
// rank-32 update -- three launches and three passes over Q[j0:, j0:] per panel, ~35 us each in the pivoted factorisations of the first
// pass (2 550 panels per sweep).  Here QMB / 32 consecutive panels act at once,
//      H_1 ... H_q = I - Y_blk T_blk Y_blk^T,      T_blk^-1 = [[T_1^-1, Y_1^T Y_2, ...], [0, T_2^-1, ...], ...]
// (block upper triangular: the inverse of dlarft's merged factor has the panels' own T_p^-1 on the diagonal and the blocks of the Gram
// matrix G = Y_blk^T Y_blk above it), so X = T_blk (Y_blk^T Q) is a block back substitution,  X_q = T_q (Z_q - sum_{j > q} G_qj X_j),
// done by ONE small launch per outer block; T_blk itself is never formed.  Per outer block: G, Z = Y_blk^T Q, the substitution, and a
// rank-QMB update -- four products and three reductions less per four panels, a quarter of the passes over Q.
constexpr int QMB = 128;
// rows of an outer block above each panel's own top block must read as zero in the merged reflector (the workspace is reused)
__global__ __launch_bounds__(256) void zero_above_panels_kernel(double* __restrict__ Y, int64_t rs, int64_t cs, int64_t k, int nb) {
    const int64_t J0 = (int64_t)blockIdx.y * QMB;
    const int bw = (int)((k - J0 < QMB) ? k - J0 : QMB);
    for (int e = blockIdx.x * 256 + threadIdx.x; e < bw * bw; e += gridDim.x * 256) {
        const int i = e / bw, j = e % bw;
        if (i / nb < j / nb) Y[(J0 + i) * rs + (J0 + j) * cs] = 0.0;
    }
}
// X (bw x nq, row-major) = T_blk Z by block back substitution; G: bw x bw row-major (pitch bw); T: the block's first panel factor
// (b x b row-major each, pitch b, 32 x 32 doubles apart).  One workgroup = 32 columns of Z; the block rows of G and the T_q are staged in
// LDS and, panel by panel (last to first), the two small products run on the matrix cores: wave w owns the 16 x 16 tile (w / 2, w % 2)
// of the 32 x 32 result.  (A first version with one thread per 4 x 1 entries and G read from memory inside the dependent loop took 85 us.)
__global__ __launch_bounds__(256) void apply_merged_T_kernel(const double* __restrict__ Z, int64_t nq, const double* __restrict__ G, int bw,
                                                             const double* __restrict__ T, int npan, double* __restrict__ X) {
    constexpr int NP = QMB / 32;
    __shared__ double xs[QMB][33];                    // X so far (rows of the panels already substituted)
    __shared__ double vs[32][33];                     // Z_q - sum_j G_qj X_j
    __shared__ double gs[(NP - 1) * 32][QMB - 32 + 1];  // panel q's block row of G to the right of it: rows 32 q .. 32 q + 31, columns from 0
    __shared__ double ts[NP][32][33];                 // T_q
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4, ti = wave >> 1, tj = wave & 1;
    const int64_t c0 = (int64_t)blockIdx.x * 32;
    // everything the substitution reads goes to LDS / registers in ONE round of loads, issued back to back from fully unrolled loops with
    // masks instead of data-dependent trip counts (a loop whose body is "load, store to LDS" waits for every load before it issues the
    // next one: the per-panel staging spent 21 us of such round trips per launch in the sweep, a first "single round" version with
    // runtime loop bounds 25); the panels are then a chain of matrix-core steps and barriers only
    {
        double gv[12][3], tv[NP * 4];
#pragma unroll
        for (int u1 = 0; u1 < 12; ++u1)
#pragma unroll
            for (int u2 = 0; u2 < 3; ++u2) {
                const int i = (tid >> 5) + 8 * u1, j = (tid & 31) + 32 * u2;       // row i of the block, column 32 (q + 1) + j of G
                const int col = 32 * ((i >> 5) + 1) + j;
                gv[u1][u2] = (i < (npan - 1) * 32 && col < bw) ? G[(int64_t)i * bw + col] : 0.0;
            }
#pragma unroll
        for (int u = 0; u < NP * 4; ++u) {
            const int q = u >> 2, idx = (u & 3) * 256 + tid, i = idx >> 5, l = idx & 31;
            const int bq = (bw - 32 * q < 32) ? bw - 32 * q : 32;
            tv[u] = (q < npan && i < bq && l < bq) ? T[(int64_t)q * 1024 + i * bq + l] : 0.0;
        }
#pragma unroll
        for (int u1 = 0; u1 < 12; ++u1)
#pragma unroll
            for (int u2 = 0; u2 < 3; ++u2) gs[(tid >> 5) + 8 * u1][(tid & 31) + 32 * u2] = gv[u1][u2];
#pragma unroll
        for (int u = 0; u < NP * 4; ++u) { const int idx = (u & 3) * 256 + tid; ts[u >> 2][idx >> 5][idx & 31] = tv[u]; }
    }
    double zr[NP][4];
#pragma unroll
    for (int q = 0; q < NP; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 32 * q + 16 * ti + lk + 4 * r;
            const int64_t c = c0 + 16 * tj + lr;
            zr[q][r] = (q < npan && i < bw && c < nq) ? Z[(int64_t)i * nq + c] : 0.0;
        }
    __syncthreads();
#pragma unroll
    for (int qq = 0; qq < NP; ++qq) {
        const int q = NP - 1 - qq;
        if (q >= npan) continue;                                   // (uniform)
        const int r0 = q * 32, kr = bw - r0 - 32;                   // kr: columns of G right of the panel (<= 96; <= 0 for the last one)
        d4l acc = {zr[q][0], zr[q][1], zr[q][2], zr[q][3]};
        for (int kk = 0; kk < kr; kk += 4) {
            const int k = kk + lk;
            const double a = (k < kr) ? -gs[r0 + 16 * ti + lr][k] : 0.0;
            const double b = (k < kr) ? xs[r0 + 32 + k][16 * tj + lr] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) vs[16 * ti + lk + 4 * r][16 * tj + lr] = acc[r];
        __syncthreads();
        d4l x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 32; kk += 4) {
            const int k = kk + lk;
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(ts[q][16 * ti + lr][k], vs[k][16 * tj + lr], x, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) xs[r0 + 16 * ti + lk + 4 * r][16 * tj + lr] = x[r];
        __syncthreads();
    }
    for (int e = tid; e < bw * 32; e += 256) {
        const int i = e >> 5, cc = e & 31;
        if (c0 + cc < nq) X[(int64_t)i * nq + c0 + cc] = xs[i][cc];
    }
}

// TN_QR_TRACE=1 (diagnostics): every call is timed synchronously with a pair of events and booked under its shape and kind; the
// table is printed when the process exits.  Perturbs the run (one synchronisation per factorisation).
namespace {
struct QrTrace {
    bool on;
    std::mutex mu;
    std::map<std::tuple<int64_t, int64_t, int, int, int>, std::pair<double, long>> tab;
    std::map<std::tuple<int64_t, int64_t, int, int, int>, double> ranks;
    double cat_ms[8] = {0}, cat_rank[8] = {0}, cat_m[8] = {0};
    long cat_calls[8] = {0};
    QrTrace() : on(env_flag_set("TN_QR_TRACE")) {}
    ~QrTrace() {
        if (!on || tab.empty()) return;
        std::vector<std::pair<double, std::tuple<int64_t, int64_t, int, int, int>>> v;
        double tot = 0.0;
        long calls = 0;
        for (auto& kv : tab) { v.push_back({kv.second.first, kv.first}); tot += kv.second.first; calls += kv.second.second; }
        std::sort(v.begin(), v.end(), [](auto& a, auto& b) { return a.first > b.first; });
        fprintf(stderr, "[tn_qr trace] %zu shapes, %ld calls, %.1f ms in total; m n wantQ truncating pivoted : calls, ms, us/call, mean accepted rank\n", v.size(), calls, tot);
        const char* cn[8] = {"plain, n <= 32", "plain, n <= 64", "plain, n <= 128", "plain, n > 128", "truncating, unpivoted", "pivoted, m <= 8192", "pivoted, m > 8192", ""};
        for (int c = 0; c < 7; ++c)
            fprintf(stderr, "  [%s] %ld calls, %.1f ms, mean rows %.0f, mean accepted rank %.1f\n", cn[c], cat_calls[c], cat_ms[c],
                    cat_calls[c] ? cat_m[c] / cat_calls[c] : 0.0, cat_calls[c] ? cat_rank[c] / cat_calls[c] : 0.0);
        static const size_t rows = (size_t)env_i64("TN_QR_TRACE_ROWS", 60);
        for (size_t i = 0; i < v.size() && i < rows; ++i) {
            auto& k = v[i].second;
            auto& st = tab[k];
            fprintf(stderr, "  %6lld %6lld  %d %d %d : %6ld  %8.2f  %8.2f  %7.1f\n", (long long)std::get<0>(k), (long long)std::get<1>(k), std::get<2>(k),
                    std::get<3>(k), std::get<4>(k), st.second, st.first, 1e3 * st.first / st.second, ranks[k] / st.second);
        }
    }
};
QrTrace g_qr_trace;
}  // namespace
// ---- the single-launch exits: all k columns, the input untouched ----------------------------------------------------------------------
static int single_launch_done(const QrCall& c, int64_t k, bool* done) {
    if (c.keff_host) *c.keff_host = k;
    if (c.input_intact) *c.input_intact = true;
    *done = true;
    return 0;
}
// tiny matrices: the whole factorisation in one workgroup (TN_QR_TINY=0: the blocked path; read per call: the tests switch it)
static int tiny_exit(const QrCall& c, int64_t k, bool* done) {
    const bool tiny_on = env_flag_on("TN_QR_TINY");
    if (!(tiny_on && c.nb == 32 && c.pivot_perm_host == nullptr && c.m * c.n <= 4096 && k <= 32)) return 0;
    QR_LAUNCH(c, tiny_qr_kernel, dim3(1), (const double*)c.A, c.rs, c.cs, (int)c.m, (int)c.n, c.Q, c.qrs, c.qcs, c.R, c.rrs, c.rcs);
    return single_launch_done(c, k, done);
}
// up to 64 columns (no pivoting; the rank-revealing exit only exists from three panels on): the whole factorisation in ONE launch,
// explicit-Q iterated Cholesky-QR (smallqr.hip); it leaves the input untouched
static int smallqr_exit(const QrCall& c, QrWs& w, int64_t k, bool* done) {
    if (!(c.nb == 32 && c.pivot_perm_host == nullptr && c.Q != nullptr && smallqr_fits(c.m, c.n))) return 0;
    const int rc = smallqr_factor(c.st, c.A, c.rs, c.cs, c.m, c.n, c.Q, c.qrs, c.qcs, c.R, c.rrs, c.rcs, c.nf_out2, w.gemm_ws, w.gemm_ws_bytes);
    if (rc) return rc == 1 ? 0 : rc;     // 1: shape / stream not taken, the blocked path follows
    if (c.nf_done) *c.nf_done = c.nf_out2 ? 1 : 0;
    return single_launch_done(c, k, done);
}
// ---- device-side panel pivoting (see pivot_select_kernel): the host runs one panel ahead of the verdicts it reads back -----------------
struct PivDev {
    PivState* pst = nullptr; int* pperm = nullptr;      // state block and permutation in the workspace
    const int* active = nullptr;         // DEVICE: 0 once the exit test has fired, what the later launches of the call look at (null: not in use)
    PivMail* ring = nullptr; unsigned seq0 = 0;          // the host thread's mailbox ring and the stamp before the first one of this call
    int begin(const QrCall& c, QrWs& w, int P) {
        pst = (PivState*)w.piv, pperm = (int*)(w.piv + 1024), active = &pst->h.active;
        ring = (PivMail*)pinned_host(4 * sizeof(PivMail), PIN_SHARED);
        if (!ring) { set_error("tn_qr: no page-locked memory for the pivoting verdicts"); return 1; }
        for (int i = 0; i < 4; ++i) __atomic_store_n(&ring[i].word, 0ull, __ATOMIC_RELAXED);       // (the slot is shared with other read-backs of this thread: no stale word may look like a stamp)
        thread_local unsigned piv_seq = 0;                        // stamps are unique per host thread (the ring is the thread's own; wrap-around after 2^32 panels is harmless: four entries)
        seq0 = piv_seq, piv_seq += (unsigned)P + 1u;
        QR_LAUNCH(c, pivot_init_kernel, dim3((unsigned)cdiv(std::max<int64_t>(c.n, 256), 256)), pst, pperm, (int)c.n);
        return 0;
    }
    // residual norms, selection and column moves in front of panel pn
    int select(const QrCall& c, QrWs& w, const QrPanel& pn) {
        const int64_t ntr = c.n - pn.j0;
        QR_LAUNCH(c, colnorm2_kernel, dim3((unsigned)ntr), pn.Ap.p, c.rs, c.cs, pn.mp, ntr, w.cn);
        QR_LAUNCH(c, pivot_select_kernel, dim3((unsigned)cdiv(ntr, PIV_CPB)), (const double*)w.cn, (int)ntr, pn.b, (int)pn.j0, pn.p, c.rank_tol * c.rank_tol, pst,
                  &ring[pn.p & 3], seq0 + (unsigned)pn.p + 1u);
        QR_LAUNCH(c, swap_columns_dev_kernel, dim3((unsigned)cdiv(c.m, 64) + 1), c.A, c.rs, c.cs, c.m, (const PivState*)pst, pperm);
        return 0;
    }
    // verdict of panel q (the selection launch in front of it): *stop = the exit test fired there, with *k_exit columns accepted
    int verdict(const QrCall& c, int q, bool* stop, int64_t* k_exit) {
        const PivMail* h = &ring[q & 3];
        const unsigned want = seq0 + (unsigned)q + 1u;
        unsigned long long wd = __atomic_load_n(&h->word, __ATOMIC_ACQUIRE);
        for (long spins = 0; (unsigned)(wd >> 32) != want; ++spins) {
            if ((spins & 0xfffff) == 0xfffff && hipStreamQuery(c.st) != hipErrorNotReady) {          // the stream has drained (or failed): look once more, then give up
                wd = __atomic_load_n(&h->word, __ATOMIC_ACQUIRE);
                if ((unsigned)(wd >> 32) == want) break;
                set_error("tn_qr: the pivoting verdict of panel %d never arrived", q);
                return 1;
            }
            wd = __atomic_load_n(&h->word, __ATOMIC_ACQUIRE);
        }
        *stop = ((wd >> 31) & 1ull) == 0ull;
        if (*stop) *k_exit = (int64_t)(wd & 0x7fffffffull);
        return 0;
    }
    // the last panel's own verdict (it may have stopped the factorisation in front of itself) unless an earlier one has stopped it, then
    // the permutation and the dropped norm (with device-side pivoting only a verdict stops the factorisation)
    int finish(const QrCall& c, QrWs& w, int P, bool* stop, int64_t* k_exit) {
        int rc;
        if (P >= 1 && !*stop && (rc = verdict(c, P - 1, stop, k_exit))) return rc;
        // state block (1024 bytes, for the dropped norm) and permutation are neighbours in the workspace: one copy
        int* hp = nullptr;
        if ((rc = read_back_staged(c.st, (void**)&hp, w.piv, 1024 + (size_t)c.n * 4, PIN_QR, "permutation"))) return rc;
        for (int64_t j = 0; j < c.n; ++j) c.pivot_perm_host[j] = hp[256 + j];
        if (((const PivState*)hp)->h.stamp < 0) {
            set_error("tn_qr: the device-side pivot selection of panel %d was not a valid set of columns (TN_PIVOT_DEVICE=0 selects on the host)", -((const PivState*)hp)->h.stamp - 1);
            return 1;
        }
        if (*stop && c.dropped2_host) *c.dropped2_host = ((const PivState*)hp)->h.dropped2;
        return 0;
    }
};
// ---- host-side pivoting of one panel (TN_PIVOT_DEVICE=0, or more than PIV_MAXN columns): *stop with j0 columns accepted when what is
// left is below the threshold, otherwise the b columns with the largest residuals are swapped to the front
static int pivot_on_host(const QrCall& c, QrState& s, const QrPanel& pn, bool* stop, int64_t* k_exit) {
    const int64_t ntr = c.n - pn.j0;
    int rc;
    QR_LAUNCH(c, colnorm2_kernel, dim3((unsigned)ntr), pn.Ap.p, c.rs, c.cs, pn.mp, ntr, s.w.cn);
    double* hcn = nullptr;
    if ((rc = read_back_staged(c.st, (void**)&hcn, s.w.cn, (size_t)ntr * 8, PIN_QR, "norms"))) return rc;
    double fro2 = 0.0;
    for (int64_t j = 0; j < ntr; ++j) fro2 += hcn[j];
    if (pn.p == 0) s.scale2 = fro2;
    if (pn.p > 0 && fro2 <= c.rank_tol * c.rank_tol * s.scale2) {     // what is left is below the threshold: stop before this panel
        if (c.dropped2_host) *c.dropped2_host = fro2;
        *stop = true, *k_exit = pn.j0;
        return 0;
    }
    int pairs[64];
    select_pivots(hcn, ntr, pn.b, pn.j0, c.pivot_perm_host, pairs);
    SwapList sl = {};
    compose_swaps(pairs, pn.b, sl);
    if (sl.n > 0)
        TN_PROF_LAUNCH(c.st, PROF_QR_AUX, hipLaunchKernelGGL(swap_columns_kernel, dim3((unsigned)cdiv(c.m, 256)), dim3(256), 0, c.st, c.A, c.rs, c.cs, c.m, sl));
    TN_CHECK_LAUNCH("swap_columns_kernel");
    return 0;
}
// ---- panel step, 32-wide: orthonormalisation + reconstruction + the tall products in one chain of launches (cholqr.hip); W goes to pn.Wp
static int panel_fused(const QrCall& c, QrState& s, const QrPanel& pn, const int* active) {
    return cholqr_panel(c.st, pn.Ap.p, c.rs, c.cs, pn.Yp.p, s.yrs, s.ycs, pn.mp, pn.b, s.w.panel_ws, s.w.panel_bytes, (uint64_t)pn.p + 1, 1, pn.Tp, pn.Wp.p,
                        pn.Wp.rs, pn.Wp.cs, nullptr, &s.fbase, s.w.cq_state, active);
}
static void dbg_check_factors(const QrCall& c, QrState& s, const QrPanel& pn) {
    dbg_check(c.st, pn.Tp, pn.b, 1, pn.b, pn.b, "T", pn.p, 9), dbg_check(c.st, s.w.Uinv, pn.b, 1, pn.b, pn.b, "Uinv", pn.p, 9);
}
// 64-wide: five rounds of Jacobi orthonormalisation through the Gram matrix, then the reconstruction by lu_reconstruct_kernel
static int panel_jacobi64(const QrCall& c, QrState& s, const QrPanel& pn) {
    hipStream_t st = c.st;
    QrWs& w = s.w;
    const Mat Yp = pn.Yp, Wp = pn.Wp, Wqp = pn.Wqp;
    const int64_t yrs = s.yrs, ycs = s.ycs, mp = pn.mp;
    int rc, b = pn.b, p = pn.p;
    if ((rc = copy_mat(st, pn.Ap.p, c.rs, c.cs, Yp.p, yrs, ycs, mp, b))) return rc;
    const int nchunk = gram_nchunk(mp);
    for (int it = 0; it < 5; ++it) {
        if ((rc = gram_partial(st, Yp.p, ycs, yrs, mp, b, b, nullptr, 1, nchunk, w.part))) return rc;
        const int mode = (it < 4) ? 0 : 1;
        // after the first round the columns are images of unit columns under an orthogonal J: a squared norm below
        // 1e-26 there is rounding noise (possibly structured, e.g. all parallel), so the column is refilled
        if ((rc = eig_small(st, w.part, nchunk, b, 1, mode, 12, it == 0 ? 0.0 : 1e-26, w.Js, mode == 0 ? w.dead : nullptr, nullptr, nullptr))) return rc;
        dbg_check(st, w.Js, b, 1, b, b, "Js", p, it);
        if ((rc = rows_times_small(st, Yp.p, yrs, ycs, mp, b, w.Js))) return rc;
        dbg_check(st, Yp.p, yrs, ycs, mp < 64 ? mp : 64, b, "W", p, it);
        if (mode == 0)
            QR_LAUNCH(c, refill_dead_kernel, dim3((unsigned)cdiv(mp, 256)), Yp.p, yrs, ycs, mp, b, w.dead, (uint64_t)(0x9E3779B97F4A7C15ULL * (uint64_t)(p * 4 + it + 1)));
    }
    TN_PROF_LAUNCH(st, PROF_LU, hipLaunchKernelGGL((lu_reconstruct_kernel<64>), dim3(1), dim3(256), 0, st, Yp.p, yrs, ycs, b, w.Uinv, pn.Tp, w.UT, w.UTq,
                       Wp.p, s.wrs, s.wcs, Wqp.p));
    TN_CHECK_LAUNCH("lu_reconstruct_kernel");
    dbg_check_factors(c, s, pn);
    if (mp > b) {            // rows below the top block: Y <- Q1 Uinv,  W <- Q1 (Uinv T^T),  Wq <- Q1 (Uinv T)
        dim3 grid((unsigned)cdiv(mp - b, 256));
        prof_begin(st, PROF_ROWS_SMALL);
        hipLaunchKernelGGL((rows_times_small3_kernel<64>), grid, dim3(256), 0, st, sub(Yp, b, 0).p, yrs, ycs, mp - b, b,
                           w.Uinv, w.UT, w.UTq, sub(Wp, b, 0).p, s.wrs, s.wcs, sub(Wqp, b, 0).p);
        TN_CHECK_LAUNCH("rows_times_small3_kernel");
        prof_end(st, PROF_ROWS_SMALL, 6.0 * (mp - b) * b * b, 32.0 * (mp - b) * b);
    }
    return 0;
}
// ---- trailing update  A[j0:, j0:j0+nc] -= (Y T^T) (Y^T A[j0:, j0:j0+nc]) -----------------------------------------------------------------
// The rank-32 updates of the panels (trailing matrix and Q) go through rank_update (rank_update.hip) instead of a K = 32 launch of gemm: the
// same bits (TN_QR_RANK_UPDATE=0 restores gemm).  The 64-wide panels keep gemm.  active (DEVICE, may be null): the same two products,
// skipped on the device once the exit test of the device-side pivoting has fired.
static int trailing_update(const QrCall& c, QrState& s, const QrPanel& pn, int64_t nc, const int* active) {
    QrWs& w = s.w;
    const Mat Ap = pn.Ap, Wp = pn.Wp, Xm = mat(w.X, nc, 1), Yt = tr(pn.Yp);
    int rc;
    if (!active) {
        if ((rc = gemm(c.st, pn.b, nc, pn.mp, 1.0, Yt, Ap, 0.0, Xm, w.gemm_ws, w.gemm_ws_bytes))) return rc;
        return s.ru_on ? rank_update(c.st, pn.mp, nc, pn.b, Wp, Xm, Ap) : gemm(c.st, pn.mp, nc, pn.b, -1.0, Wp, Xm, 1.0, Ap);
    }
    GemmExtra gx_active;                 // (the same two products, skipped on the device once the exit test has fired)
    gx_active.skip = active;
    if ((rc = gemm_ex(c.st, pn.b, nc, pn.mp, 1.0, Yt.p, Yt.rs, Yt.cs, Ap.p, Ap.rs, Ap.cs, 0.0, Xm.p, Xm.rs, Xm.cs, 1, 0, 0, 0, w.gemm_ws, w.gemm_ws_bytes, &gx_active)))
        return rc;
    return s.ru_on ? rank_update(c.st, pn.mp, nc, pn.b, Wp, Xm, Ap, active)
                   : gemm_ex(c.st, pn.mp, nc, pn.b, -1.0, Wp.p, Wp.rs, Wp.cs, Xm.p, Xm.rs, Xm.cs, 1.0, Ap.p, Ap.rs, Ap.cs, 1, 0, 0, 0, nullptr, 0, &gx_active);
}
// ---- the rank-revealing exit (rank_tol > 0, no pivoting, from three panels on) -----------------------------------------------------------
// Every second panel the largest column norm of the not-yet-factored trailing block is compared with the largest column norm of the
// input; once it is below rank_tol times that, the remaining rows of R would be negligible on the scale of the leading singular value
// and the factorisation stops with k_eff columns (A = Q[:, :k_eff] R[:k_eff, :] to rank_tol * max column norm).  Used by the truncating
// canonisation passes, whose centre matrix is SVD-truncated at eps * S0 right afterwards (the Jacobi SVD deflates rows below 2^-56
// anyway); it needs one 16-byte read-back per check.  After panel pn: *stop with the columns up to the end of pn accepted.
static int reveal_check(const QrCall& c, QrState& s, const QrPanel& pn, bool* stop, int64_t* k_exit) {
    double* cn = s.w.cn;
    const int64_t n = c.n, j1 = pn.j0 + pn.b, nt = n - j1;
    int rc;
    QR_LAUNCH(c, colnorm2_kernel, dim3((unsigned)nt), sub(s.Am, j1, j1).p, c.rs, c.cs, c.m - j1, nt, cn + n);
    // one read-back: the trailing norms, and (first check only) the input norms stored in front of them
    const size_t nread = (size_t)(s.scale2 < 0.0 ? n + nt : nt);
    double* hcn = nullptr;
    if ((rc = read_back_staged(c.st, (void**)&hcn, s.scale2 < 0.0 ? cn : cn + n, nread * 8, PIN_QR, "norms"))) return rc;
    const double* tr2 = hcn;
    // measure of "what is left" against the input: largest column norm (default) or, frob_exit, the Frobenius norm
    if (s.scale2 < 0.0) {
        s.scale2 = 0.0;
        for (int64_t j = 0; j < n; ++j) s.scale2 = c.frob_exit ? s.scale2 + hcn[j] : std::max(s.scale2, hcn[j]);
        tr2 = hcn + n;
    }
    double left = 0.0;
    for (int64_t j = 0; j < nt; ++j) left = c.frob_exit ? left + tr2[j] : std::max(left, tr2[j]);
    if (!(left <= c.rank_tol * c.rank_tol * s.scale2)) return 0;      // (a NaN never stops the factorisation)
    double fro2 = 0.0;                                       // nothing left above the threshold: the squared Frobenius norm of the block that is dropped
    for (int64_t j = 0; c.dropped2_host && j < nt; ++j) fro2 += tr2[j];
    if (c.dropped2_host) *c.dropped2_host = fro2;
    *stop = true, *k_exit = j1;
    return 0;
}
// ---- Q accumulation through merged reflectors, last outer block (bwo columns) to first:  Q[J0:, J0:] -= Y_blk (T_blk (Y_blk^T Q[J0:, J0:])).  T_blk is applied
// either as the matrix the two-level factorisation has built (w.Tblk) or, merged_T, by the block back substitution of
// apply_merged_T_kernel from the panels' own T_p and the Gram matrix of the block, which is formed first.
static int accumulate_Q_blocks(const QrCall& c, QrState& s, int64_t k, int bwo, bool merged_T) {
    hipStream_t st = c.st;
    QrWs& w = s.w;
    const int nb = c.nb, nblk = (int)cdiv(k, bwo);
    const Mat Qm = mat(c.Q, c.qrs, c.qcs);
    int rc;
    if (merged_T) QR_LAUNCH(c, zero_above_panels_kernel, dim3(16, (unsigned)nblk), w.Y, s.yrs, s.ycs, k, nb);
    for (int bi = nblk - 1; bi >= 0; --bi) {
        const int64_t J0 = (int64_t)bi * bwo;
        const int bw = (int)((k - J0 < bwo) ? k - J0 : bwo);
        const int64_t mb = c.m - J0, nq = k - J0;
        const int npan = (int)cdiv(bw, nb);
        Mat Yb = sub(s.Ym, J0, J0), Qb = sub(Qm, J0, J0), Z = mat(w.Zo, nq, 1), X = mat(w.Zo2, nq, 1), Gm = mat(w.G, bw, 1);
        if (merged_T && npan > 1 && (rc = gemm(st, bw, bw, mb, 1.0, tr(Yb), Yb, 0.0, Gm, w.gemm_ws, w.gemm_ws_bytes))) return rc;
        // (the last block meets [Z; 0]: only its top bw rows are non-zero, the product over the rest adds zeros)
        if ((rc = gemm(st, bw, nq, bi == nblk - 1 ? (int64_t)bw : mb, 1.0, tr(Yb), Qb, 0.0, Z, w.gemm_ws, w.gemm_ws_bytes))) return rc;
        if (merged_T)
            QR_LAUNCH(c, apply_merged_T_kernel, dim3((unsigned)cdiv(nq, 32)), (const double*)Z.p, nq, (const double*)Gm.p, bw, (const double*)(w.T + (J0 / nb) * nb * nb), npan, X.p);
        else if ((rc = gemm(st, bw, nq, bw, 1.0, mat(w.Tblk + (int64_t)bi * QR_NBO_MAX * QR_NBO_MAX, bw, 1), Z, 0.0, X))) return rc;
        if ((rc = gemm(st, mb, nq, bw, -1.0, Yb, X, 1.0, Qb))) return rc;
    }
    return 0;
}
// Panel by panel, last to first; the last one is skipped when the launch that wrote [Z; 0] has applied it (what the m x k array holds: see panel_at)
static int accumulate_Q_panels(const QrCall& c, QrState& s, int64_t k, int P, int fold_b) {
    const Mat Qm = mat(c.Q, c.qrs, c.qcs);
    int rc;
    for (int p = P - 1 - (fold_b > 0 ? 1 : 0); p >= 0; --p) {
        const QrPanel pn = panel_at(c, s, p, k);
        const int64_t nq = k - pn.j0;
        const Mat Qp = sub(Qm, pn.j0, pn.j0), Xm = mat(s.w.X, nq, 1), Lp = s.wform ? pn.Yp : pn.Wqp;
        // Y^T Q (the last panel meets [Z; 0]: only its top b rows are non-zero, the product over the rest adds zeros)
        if ((rc = gemm(c.st, pn.b, nq, p == P - 1 ? (int64_t)pn.b : pn.mp, 1.0, tr(s.wform ? pn.Wqp : pn.Yp), Qp, 0.0, Xm, s.w.gemm_ws, s.w.gemm_ws_bytes))) return rc;
        // Q -= (Y T) (Y^T Q) = Y (W^T Q)
        if ((rc = s.ru_on ? rank_update(c.st, pn.mp, nq, pn.b, Lp, Xm, Qp) : gemm(c.st, pn.mp, nq, pn.b, -1.0, Lp, Xm, 1.0, Qp))) return rc;
    }
    return 0;
}
// ---- two-level blocked factorisation (nb = 32 inside outer blocks of `nbo` columns) ---------------------------------------
// Single-level blocking applies every 32-wide reflector to the whole trailing matrix and again to Q: three passes over up to
// 134 MB per panel at K = 32, i.e. HBM-bound work that fills the device (12.9 GB for one 16384 x 1024 call against 0.28 GB
// compulsory) and, with several chains on the GPU, serialises them.  Here the panels of an outer block only update the
// columns of that block; the columns to its right (and, afterwards, Q) see the block once, through the merged reflector
//      H_1 ... H_q = I - Y_blk T_blk Y_blk^T,   T_blk = [[T_1, -T_1 (Y_1^T Y_2) T_2, ...], [0, T_2, ...], ...]   (dlarft by blocks)
// built from the panels' own (Y_p, T_p) and one Gram matrix G = Y_blk^T Y_blk: rank-nbo GEMMs (K = 128 or 256) instead of
// rank-32 ones, 4-8x fewer bytes.  Used for the plain factorisation only (rank_tol = 0): the rank-revealing early exit of the
// truncating passes checks the trailing block after every second panel, which needs it up to date.
static int qr_two_level(const QrCall& c, QrState& s, int nbo) {
    hipStream_t st = c.st;
    QrWs& w = s.w;
    const int64_t m = c.m, n = c.n, k = m < n ? m : n;
    const int nb = 32, nblk = (int)cdiv(k, nbo);
    int rc;
    for (int bi = 0; bi < nblk; ++bi) {
        const int64_t J0 = (int64_t)bi * nbo;
        const int bw = (int)((k - J0 < nbo) ? k - J0 : nbo);
        const int64_t Jend = J0 + bw, mb = m - J0;
        Mat Yb = sub(s.Ym, J0, J0);
        // rows of the block above each panel's own top block must read as zero in the merged reflector
        if ((rc = fill_mat(st, Yb.p, s.yrs, s.ycs, bw, bw, 0.0))) return rc;
        double* Tb = w.Tblk + (int64_t)bi * QR_NBO_MAX * QR_NBO_MAX;            // bw x bw, row-major, pitch bw
        if ((rc = fill_mat(st, Tb, bw, 1, bw, bw, 0.0))) return rc;
        const int npan = (int)cdiv(bw, nb);
        for (int q = 0; q < npan; ++q) {
            QrPanel pn = panel_at(c, s, (int)(J0 / nb) + q, Jend);
            pn.Wp = mat(w.W, s.wrs, s.wcs);                                      // W of the current panel only: Q goes through T_blk
            if ((rc = panel_fused(c, s, pn, nullptr))) return rc;
            if ((rc = trailing_update(c, s, pn, Jend - pn.j0, nullptr))) return rc;   // the panel's update stays inside the block
            // T_blk: diagonal block = T_p (its pitch is b); column block from the recurrence once the Gram matrix exists (below)
            if ((rc = copy_mat(st, pn.Tp, pn.b, 1, Tb + (int64_t)(pn.j0 - J0) * bw + (pn.j0 - J0), bw, 1, pn.b, pn.b))) return rc;
        }
        // G = Y_blk^T Y_blk, then T_blk[0:c0, c0:c0+b] = -T_blk[0:c0, 0:c0] (G[0:c0, c0:c0+b] T_q)
        Mat Gm = mat(w.G, bw, 1);
        if (npan > 1) {
            if ((rc = gemm(st, bw, bw, mb, 1.0, tr(Yb), Yb, 0.0, Gm, w.gemm_ws, w.gemm_ws_bytes))) return rc;
            for (int q = 1; q < npan; ++q) {
                const int64_t c0 = (int64_t)q * nb;
                const int b = (int)((bw - c0 < nb) ? bw - c0 : nb);
                Mat Tq = mat(Tb + c0 * bw + c0, bw, 1), tmp = mat(w.tmpT, b, 1);
                if ((rc = gemm(st, c0, b, b, 1.0, sub(Gm, 0, c0), Tq, 0.0, tmp))) return rc;
                if ((rc = gemm(st, c0, b, c0, -1.0, mat(Tb, bw, 1), tmp, 0.0, mat(Tb + c0, bw, 1)))) return rc;
            }
        }
        // outer update of everything to the right of the block:  A_r -= Y_blk (T_blk^T (Y_blk^T A_r))
        const int64_t nr = n - Jend;
        if (nr > 0) {
            Mat Ar = sub(s.Am, J0, Jend), Z = mat(w.Zo, nr, 1), Z2 = mat(w.Zo2, nr, 1);
            if ((rc = gemm(st, bw, nr, mb, 1.0, tr(Yb), Ar, 0.0, Z, w.gemm_ws, w.gemm_ws_bytes))) return rc;
            if ((rc = gemm(st, bw, nr, bw, 1.0, tr(mat(Tb, bw, 1)), Z, 0.0, Z2))) return rc;
            if ((rc = gemm(st, mb, nr, bw, -1.0, Yb, Z2, 1.0, Ar))) return rc;
        }
    }
    // R, then Q = H_blk1 ... H_blkB [Z; 0] (no fold: every block goes through its T_blk)
    if ((rc = triangularise_diag(c, s, k, (int)cdiv(k, nb)))) return rc;
    if ((rc = assemble_R_init_Q(c, s, k, QrFold{}))) return rc;
    return accumulate_Q_blocks(c, s, k, nbo, false);
}
// ---- dispatch, the loop over the panels, the ending
static int qr_factor_impl(const QrCall& c) {
    const int64_t m = c.m, n = c.n;
    const int nb = c.nb;
    TN_CHECK_ARG(m >= 1 && n >= 1, "empty matrix");
    if (c.dropped2_host) *c.dropped2_host = 0.0;
    TN_CHECK_ARG(nb == 32 || nb == 64, "nb must be 32 or 64");
    TN_CHECK_ARG(c.ws_bytes >= qr_ws_bytes(m, n, nb), "workspace too small");
    int64_t k = m < n ? m : n;           // columns of Q, rows of R: k and P only change where the loop below stops early
    int rc;
    bool done = false, stop = false;     // a single-launch exit has done the work / an exit test has ended the panel loop
    if ((rc = tiny_exit(c, k, &done)) || done) return rc;
    QrState s;
    QrWs& w = s.w;
    qr_layout(m, n, nb, (char*)c.ws, &w);
    if ((rc = smallqr_exit(c, w, k, &done)) || done) return rc;
    int P = (int)cdiv(k, nb);
    const bool truncating = c.rank_tol > 0.0 && c.keff_host != nullptr;
    // Panel pivoting (pivot_perm_host != NULL; nb = 32, rank_tol > 0): before every panel the residual norms of all remaining
    // columns are read back, the factorisation stops when their Frobenius norm is below rank_tol x the input's, otherwise the
    // 32 columns with the largest residuals are swapped to the front and form the next panel (column-pivoted QR at panel
    // granularity: a strong rank revealer at one extra read-back per panel).  pivot_perm_host[j] = input column now at j.
    s.pivot = c.pivot_perm_host != nullptr && truncating && nb == 32;
    for (int64_t j = 0; c.pivot_perm_host && j < n; ++j) c.pivot_perm_host[j] = j;
    s.reveal = !s.pivot && truncating && P > 2 && nb == 32;
    if (s.reveal) QR_LAUNCH(c, colnorm2_kernel, dim3((unsigned)n), c.A, c.rs, c.cs, m, n, w.cn);      // the input's column norms (see reveal_check)
    // Y shares A's fast direction so panel kernels coalesce the same way
    s.rowmajor = (c.cs == 1 && c.rs != 1);
    s.yrs = s.rowmajor ? k : 1, s.ycs = s.rowmajor ? 1 : m, s.wrs = s.rowmajor ? nb : 1, s.wcs = s.rowmajor ? 1 : m;
    s.Am = mat(c.A, c.rs, c.cs), s.Ym = mat(w.Y, s.yrs, s.ycs), s.Wqm = mat(w.Wq, s.yrs, s.ycs);
    s.wform = (nb == 32);                // the fused panel step, whose W = Y T^T serves the Q accumulation too (see panel_at)
    if (nb == 32 && (rc = cholqr_begin(c.st, w.panel_ws, &w.cq_state))) return rc;
    s.ru_on = nb == 32 && env_flag_on("TN_QR_RANK_UPDATE");          // (see trailing_update; read per call: the tests switch it)
    {   // two-level blocking for the plain factorisation of matrices with several outer blocks (TN_QR_NBO = 0 disables it)
        const int v_nbo = env_int("TN_QR_NBO", 256), nbo = (v_nbo == 128 || v_nbo == 256) ? v_nbo : 0;      // read per call: the tests switch it
        if (nbo > 0 && nb == 32 && !truncating && k >= 2 * nbo && m >= 4 * nbo) {
            if (c.keff_host) *c.keff_host = k;
            return qr_two_level(c, s, nbo);
        }
    }
    const bool piv_dev = s.pivot && env_flag_on("TN_PIVOT_DEVICE") && n <= PIV_MAXN;      // (read per call: the tests switch it)
    PivDev piv;
    if (piv_dev && (rc = piv.begin(c, w, P))) return rc;
    int64_t k_exit = k;
    for (int p = 0; p < P && !stop; ++p) {
        const QrPanel pn = panel_at(c, s, p, k);
        if (piv_dev) {
            if (p >= 1 && (rc = piv.verdict(c, p - 1, &stop, &k_exit))) return rc;
            if (!stop && (rc = piv.select(c, w, pn))) return rc;
        } else if (s.pivot && (rc = pivot_on_host(c, s, pn, &stop, &k_exit))) return rc;
        if (stop) break;
        if ((rc = s.wform ? panel_fused(c, s, pn, piv.active) : panel_jacobi64(c, s, pn))) return rc;
        if (s.wform) dbg_check_factors(c, s, pn);
        if ((rc = trailing_update(c, s, pn, n - pn.j0, piv.active))) return rc;
        if (s.reveal && (p & 1) == 1 && p + 1 < P && (rc = reveal_check(c, s, pn, &stop, &k_exit))) return rc;
    }
    if (piv_dev && (rc = piv.finish(c, w, P, &stop, &k_exit))) return rc;
    if (stop) k = k_exit, P = (int)(k / nb);      // the one place where k and P change (every exit leaves whole panels)
    if (c.keff_host) *c.keff_host = k;
    // --- triangularise the diagonal blocks, assemble R
    if (nb == 64) QR_LAUNCH(c, (diag_qr_kernel<64>), dim3(P), c.A, c.rs, c.cs, nb, k, w.Z, w.Tri, (int*)nullptr);
    else if ((rc = triangularise_diag(c, s, k, P))) return rc;
    dbg_check(c.st, w.Z, nb, 1, (int64_t)P * nb, nb, "Z", -1, 0);
    dbg_check(c.st, w.Tri, nb, 1, (int64_t)P * nb, nb, "Tri", -1, 0);
    // --- Q = H_1 ... H_P [Z; 0]; the last panel's reflector is applied by the launch that writes [Z; 0] (nb = 32)
    const int64_t jf = (int64_t)(P - 1) * nb;
    // (every workgroup of the Q part recomputes the b x b product: worth it while there are few of them, i.e. for the small
    //  factorisations whose time is launches; the large ones keep the two GEMMs)
    const int fold_b = (nb == 32 && P >= 1 && m * k <= 256 * 512) ? (int)(k - jf) : 0;
    // fused panel step: the m x k array holds W = Y T^T of every panel and  H_p Q = Q - Y_p (W_p^T Q);  otherwise it holds Y T and
    // H_p Q = Q - (Y_p T_p) (Y_p^T Q).  The kernel forms  second (first_top^T Z)  either way.
    if ((rc = assemble_R_init_Q(c, s, k, QrFold{s.wform ? w.Wq : w.Y, s.wform ? w.Y : w.Wq, s.yrs, s.ycs, jf, fold_b}))) return rc;
    // merged reflectors (see apply_merged_T_kernel): from two panels on, unless the small-matrix fold above already took the last one
    // (TN_QR_MERGED_Q=0 keeps the panel-by-panel accumulation; read per call: the tests switch it)
    const bool merged_q = s.wform && c.Q != nullptr && P >= 2 && fold_b == 0 && env_flag_on("TN_QR_MERGED_Q");
    return merged_q ? accumulate_Q_blocks(c, s, k, QMB, true) : accumulate_Q_panels(c, s, k, P, fold_b);
}
static int qr_factor_traced(const QrCall& c) {
    if (c.nf_done) *c.nf_done = 0;
    if (!g_qr_trace.on) return qr_factor_impl(c);
    thread_local hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!e0) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); }
    (void)hipEventRecord(e0, c.st);
    const int rc = qr_factor_impl(c);
    (void)hipEventRecord(e1, c.st);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, e0, e1);
    std::lock_guard<std::mutex> lk(g_qr_trace.mu);
    const bool truncating = c.rank_tol > 0.0 && c.keff_host;
    const auto key = std::make_tuple(c.m, c.n, c.Q ? 1 : 0, truncating ? 1 : 0, c.pivot_perm_host ? 1 : 0);
    auto& ss = g_qr_trace.tab[key];
    ss.first += ms, ss.second += 1;
    const double kr = c.keff_host ? (double)*c.keff_host : (double)(c.m < c.n ? c.m : c.n);
    g_qr_trace.ranks[key] += kr;
    const int cat = c.pivot_perm_host ? (c.m > 8192 ? 6 : 5) : truncating ? 4 : (c.n <= 32 ? 0 : c.n <= 64 ? 1 : c.n <= 128 ? 2 : 3);
    g_qr_trace.cat_ms[cat] += ms; g_qr_trace.cat_rank[cat] += kr; g_qr_trace.cat_calls[cat] += 1; g_qr_trace.cat_m[cat] += (double)c.m;
    return rc;
}
// rank_tol > 0 enables the early exits (reveal_check; with pivot_perm_host, the panel pivoting): *keff_host receives the number of
// columns/rows produced.
// nf_out2 != NULL (device, 2 doubles): a path that can divide R by its power-of-two norm factor in the launch that produces it does
// so and sets *nf_done (the one-launch factorisation of smallqr.hip); otherwise *nf_done = 0 and the caller normalises.
// Launches with in-kernel barriers (single-launch panel steps, smallqr.hip) may give up when the co-residency they rely on does not
// hold; unless the caller has deferred the check (FusedDeferCheck: tn_compress_mps asks once per row) the call ends by asking
// fused_timeouts: a factorisation whose input is still intact is redone through the blocked path at once, otherwise the call fails
// with -7 (the input was overwritten: the caller must rerun from a copy; the stream no longer takes the single-launch forms).
int qr_factor(hipStream_t st, double* A, int64_t rs, int64_t cs, int64_t m, int64_t n, double* Q, int64_t qrs,
              int64_t qcs, double* R, int64_t rrs, int64_t rcs, int nb, void* ws, int64_t ws_bytes, double rank_tol,
              int64_t* keff_host, double* dropped2_host, int frob_exit, int64_t* pivot_perm_host, double* nf_out2, int* nf_done) {
    bool intact = false;
    const QrCall c = {st, A, rs, cs, m, n, Q, qrs, qcs, R, rrs, rcs, nb, ws, ws_bytes, rank_tol,
                      keff_host, dropped2_host, frob_exit, pivot_perm_host, nf_out2, nf_done, &intact};
    int rc = qr_factor_traced(c);
    if (fused_check_deferred() || !fused_check_needed()) return rc;
    int gave_up = 0;
    const int rc2 = fused_timeouts(st, &gave_up);
    if (rc2) return rc2;
    if (gave_up == 0) return rc;
    if (!intact) {
        set_error("tn_qr: %d launch(es) with in-kernel barriers gave up (co-residency budget exceeded: another tenant on the device?); the "
                  "results are invalid and the input was overwritten -- rerun from a copy (this stream now takes the six-launch panel chain)", gave_up);
        return -7;
    }
    return qr_factor_traced(c);
}

}  // namespace tn
