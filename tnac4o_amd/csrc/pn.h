// The conditional table of one cell for one boundary row (reference tnac4o.py:1786-1807), shared by calc_pn_kernel (beam.hip), which
// writes the table out, and sample_pn_kernel (sampler.hip), which draws from it in LDS: one copy of the arithmetic, so both see the
// same bits.  Internal header.
#pragma once
#include "devprim.h"

namespace tn {

// doubles of LDS in front of the table: T1 slice [p][Dr], RR [Dr][br], T2 [p][br]
static __host__ __device__ inline int64_t pn_front_doubles(int64_t p, int64_t Dr, int64_t br) { return p * Dr + Dr * br + p * br; }

// 256 threads.  t1: the prefix's slice of T1 (p x Dr), rr: the suffix's right environment (Dr x br), l / u: left and up index of
// the row.  front: pn_front_doubles(p, Dr, br) doubles of LDS, sP: q doubles of LDS, red: 256 doubles of LDS.  On return sP[s]
// holds the normalised table after the negative-probability rule (entry s written by thread s % 256: a barrier is the caller's
// when other threads read it); the value returned (the same in every thread) is the table's flag minP.
static __device__ __forceinline__ double pn_table(const double* __restrict__ t1, const double* __restrict__ rr, const double* __restrict__ F,
                                                  const int32_t* __restrict__ dmap, const int32_t* __restrict__ rmap, int l, int u, int q, int nl,
                                                  int nu, int p, int Dr, int br, double* front, double* sP, double* red) {
    double* sT1 = front;                // [p][Dr]
    double* sRR = sT1 + p * Dr;         // [Dr][br]
    double* sT2 = sRR + Dr * br;        // [p][br]
    const int tid = threadIdx.x;
    for (int e = tid; e < p * Dr; e += 256) sT1[e] = t1[e];
    for (int e = tid; e < Dr * br; e += 256) sRR[e] = rr[e];
    __syncthreads();
    for (int e = tid; e < p * br; e += 256) {
        const int d = e / br, r = e % br;
        double s = 0.0;
        for (int c = 0; c < Dr; ++c) s += sT1[d * Dr + c] * sRR[c * br + r];
        sT2[e] = s;
    }
    __syncthreads();
    double mn = 1.7e308;
    for (int s = tid; s < q; s += 256) {
        const double v = F[((int64_t)s * nl + l) * nu + u] * sT2[dmap[s] * br + rmap[s]];
        sP[s] = v;
        mn = fmin(mn, v);
    }
    double mPn = block_tree_min(mn, red);
    if (mPn < 0.0) {                                   // tnac4o.py:1796-1799
        const double a = fabs(mPn);
        double cnt = 0.0;
        for (int s = tid; s < q; s += 256)
            if (sP[s] < a) { sP[s] = a; cnt += 1.0; }
        mPn *= block_tree_sum(cnt, red);
    }
    double part = 0.0;
    for (int s = tid; s < q; s += 256) part += sP[s];
    const double no = block_tree_sum(part, red);
    if (no > 0.0) {                                    // tnac4o.py:1800-1803
        const double inv = 1.0 / no;
        for (int s = tid; s < q; s += 256) sP[s] = sP[s] * inv;
        mPn *= inv;
    } else {                                           // all zeros -> uniform, flag -1 (tnac4o.py:1804-1806)
        for (int s = tid; s < q; s += 256) sP[s] = sP[s] + 1.0 / (double)q;
        mPn = -1.0;
    }
    return mPn;
}

}  // namespace tn
