// tn_uniforms: the library's counter-based generator of uniform numbers (K14 of include/tnpeps.h).
//
// out[r ld + c] = U(seed, stream0 + r, first + c) with U a pure function of three unsigned 64-bit numbers: Philox4x32-10 (Salmon,
// Moraes, Dror, Shaw 2011) on counter (b lo, b hi, stream lo, stream hi), b = i >> 1, and key (seed lo, seed hi) gives four 32-bit
// words; number i takes the words 2h, 2h + 1 with h = i & 1 as a 64-bit value v, and U = (v >> 11) 2^-53.  One block is two numbers,
// 16 bytes.
//
// One lane per (row, block of that row).  A row covers the blocks b0 = first >> 1 .. (first + cols - 1) >> 1; the lane of block b0 + j
// holds the numbers of the columns c0 = 2 (b0 + j) - first and c0 + 1, of which the first is outside the row for j = 0 and an odd
// `first`, and the second is for the last block when first + cols is odd.  A lane whose two numbers are both inside the row and
// whose address is a multiple of 16 stores them with one 16-byte store, every other number goes out with an 8-byte store; which
// store is used changes no bit.  The 256 threads of a workgroup are laid out as TY rows by TX blocks, TX the power of two that
// covers a row's blocks, at most 256: a few rows of millions of columns run as 256 consecutive blocks of one row per workgroup, a
// million rows of three columns as 128 rows of two blocks, and in both the lanes of a wave store consecutive addresses of a row.  Both
// directions of the grid are capped and looped over, so every shape the entry point admits is one launch.
#include "common.h"

namespace tn {

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;     // multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;     // key increments
constexpr int RNG_THREADS = 256;
constexpr int64_t RNG_MAX_GRID_X = 4096;         // workgroups along a row; the rest is looped over
constexpr int64_t RNG_MAX_BLOCKS = 16384;        // workgroups of a launch

struct Philox4 { uint32_t x0, x1, x2, x3; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return Philox4{c0, c1, c2, c3};
}

// (v >> 11) 2^-53 of v = lo + 2^32 hi: the conversion of a 53-bit integer and the scaling by a power of two are both exact
__device__ __forceinline__ double unit_double(uint32_t lo, uint32_t hi) {
    const uint64_t v = ((uint64_t)hi << 32) | (uint64_t)lo;
    return (double)(v >> 11) * 0x1.0p-53;
}

__global__ __launch_bounds__(RNG_THREADS) void uniforms_kernel(uint64_t seed, uint64_t stream0, uint64_t first, int64_t rows, int64_t cols,
                                                               double* __restrict__ out, int64_t ld, int log2tx) {
    const int64_t tx = threadIdx.x & ((1 << log2tx) - 1), ty = threadIdx.x >> log2tx;
    const int64_t TX = (int64_t)1 << log2tx, TY = RNG_THREADS >> log2tx;
    const uint64_t b0 = first >> 1;
    const int64_t odd = (int64_t)(first & 1);
    const int64_t nb = (cols + odd + 1) >> 1;                            // blocks a row touches (cols >= 1)
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int64_t r = (int64_t)blockIdx.y * TY + ty; r < rows; r += (int64_t)gridDim.y * TY) {
        const uint64_t s = stream0 + (uint64_t)r;
        double* __restrict__ row = out + r * ld;
        for (int64_t j = (int64_t)blockIdx.x * TX + tx; j < nb; j += (int64_t)gridDim.x * TX) {
            const uint64_t b = b0 + (uint64_t)j;
            const Philox4 x = philox4x32_10((uint32_t)b, (uint32_t)(b >> 32), (uint32_t)s, (uint32_t)(s >> 32), k0, k1);
            const double u0 = unit_double(x.x0, x.x1), u1 = unit_double(x.x2, x.x3);
            const int64_t c0 = 2 * j - odd;                              // the column of u0; u1 is the next one
            const bool in0 = c0 >= 0, in1 = c0 + 1 < cols;               // (c0 < cols and c0 + 1 >= 0 hold for every j < nb)
            if (in0 && in1 && (((uintptr_t)(row + c0)) & 15) == 0) {
                *reinterpret_cast<double2*>(row + c0) = make_double2(u0, u1);
            } else {
                if (in0) row[c0] = u0;
                if (in1) row[c0 + 1] = u1;
            }
        }
    }
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tn_uniforms(uint64_t seed, uint64_t stream0, uint64_t first, int64_t rows, int64_t cols, double* out, int64_t ld, void* stream) {
    TN_CHECK_ARG(rows >= 0 && cols >= 0, "rows or cols negative");
    TN_CHECK_ARG(ld >= cols, "ld < cols");
    TN_CHECK_ARG(rows == 0 || ld < ((int64_t)1 << 62) / rows + (((int64_t)1 << 62) % rows != 0), "rows * ld not below 2^62");
    // first + cols and stream0 + rows must not pass 2^64: the last index is first + cols - 1, the last stream stream0 + rows - 1
    // (0 - n is 2^64 - n in unsigned arithmetic)
    TN_CHECK_ARG(cols == 0 || first <= (uint64_t)0 - (uint64_t)cols, "first + cols above 2^64");
    TN_CHECK_ARG(rows == 0 || stream0 <= (uint64_t)0 - (uint64_t)rows, "stream0 + rows above 2^64");
    if (rows == 0 || cols == 0) return 0;
    TN_CHECK_ARG(out != nullptr, "null out");
    TN_CHECK_ARG((((uintptr_t)out) & 7) == 0, "out not aligned to 8 bytes");
    const int64_t nb = (cols + (int64_t)(first & 1) + 1) >> 1;
    int log2tx = 0;
    while (log2tx < 8 && ((int64_t)1 << log2tx) < nb) ++log2tx;
    const int64_t TX = (int64_t)1 << log2tx, TY = RNG_THREADS >> log2tx;
    int64_t gx = cdiv(nb, TX);
    if (gx > RNG_MAX_GRID_X) gx = RNG_MAX_GRID_X;
    int64_t gy = cdiv(rows, TY);
    const int64_t gy_max = RNG_MAX_BLOCKS / gx;                          // >= 4
    if (gy > gy_max) gy = gy_max;
    TN_PROF_LAUNCH((hipStream_t)stream, PROF_MISC, hipLaunchKernelGGL(uniforms_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(RNG_THREADS), 0,
                                                                    (hipStream_t)stream, seed, stream0, first, rows, cols, out, ld, log2tx));
    TN_CHECK_LAUNCH("uniforms_kernel");
    return 0;
}

}  // extern "C"
