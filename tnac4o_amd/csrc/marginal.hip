// Thermal cluster marginals: the three-layer contraction  rhoB[ny] . row ny . rhoT[ny+1]  with one cell left open
// (tnac4o.calculate_marginals).  No counterpart in the reference, which only samples (gibbs_sampling).
//
// Operands of one cell (all contiguous, C order):
//   At (Dt, pd, Dt2)   site of rhoT[ny+1]: top bond, the row's down leg, top bond
//   W  (bl, pd, br, pu) row MPO site W[l,d,r,u] = sum_s T[s,l,d,r,u]  (tn_mpo_from_factor)
//   Ab (Db, pu, Db2)   site of rhoB[ny]:   bottom bond, the row's up leg, bottom bond
// Environments keep the MPO bond outermost: EL (bl, Dt, Db) left of the cell, ER (br, Dt2, Db2) right of it.
//
// env3, side 0 (left step, EL -> EL' (br, Dt2, Db2)), three strided GEMMs and no permutation of any operand:
//   HL[l][d][t'][b] = sum_t  At[t,(d,t')] EL[l][t][b]                  batch l:  M = pd Dt2,  N = Db,  K = Dt
//   Y [r][t'][b][u] = sum_{l,d} HL[(l,d),(t',b)] W[(l,d),r,u]          batch r:  M = Dt2 Db,  N = pu,  K = bl pd
//   EL'[(r,t'),b']  = sum_{b,u} Y[(r,t'),(b,u)] Ab[(b,u),b']                      M = br Dt2, N = Db2, K = Db pu
// env3, side 1 (right step, ER -> ER (bl, Dt, Db)); W is first permuted to W'[l][d][u][r] (bl pd pu br doubles, the only copy):
//   HR[u][r][t'][b] = sum_b' ER[(r,t'),b'] Ab[b,u,b']                  batch u:  M = br Dt2,  N = Db,  K = Db2
//   Y [(l,d),(t',b)] = sum_{u,r} W'[(l,d),(u,r)] HR[(u,r),(t',b)]                 M = bl pd,  N = Dt2 Db, K = pu br
//   ER[l][t][b]     = sum_{d,t'} At[t,(d,t')] Y[l][(d,t')][b]          batch l:  M = Dt,  N = Db,  K = pd Dt2
// Both end with the power-of-two normalisation of the result (exact); the log2 of the factor is added to a running total.
//
// cluster_marginal: the half-products HL (left step at the cell) and HR (right step at the cell) give
//   X[(l,d),(u,r)] = sum_{t',b} HL[(l,d),(t',b)] HR[(u,r),(t',b)]                 M = bl pd,  N = pu br,  K = Dt2 Db
// and one workgroup gathers P[s] = sum_{l,u} F[s,l,u] X[l,dmap[s],u,rmap[s]], applies the negative-probability rule of
// tn_calc_pn and normalises.  log2 of the raw sum plus the two environments' running totals is the row contraction.
//
// cluster_bond_marginal (tnac4o.calculate_correlations): the same X, and the same products left unsummed over one bond:
//   Pl[s,l] = sum_u F[s,l,u] X[l,dmap[s],u,rmap[s]],   Pu[s,u] = sum_l F[s,l,u] X[l,dmap[s],u,rmap[s]]
// one workgroup per state, then one workgroup divides both tables by T = sum Pl (no negativity rule: the sums stay exact).
#include "../../include/tnpeps.h"
#include "common.h"
#include "devprim.h"

#include <algorithm>
#include <initializer_list>

namespace tn {

static bool dims_ok(std::initializer_list<int64_t> dims) {
    for (int64_t d : dims)
        if (d < 1) return false;
    return true;
}

// workspace of env3: first product (unused with half_out) | second product | permuted W (side 1) | split-K scratch of the three
// GEMMs | [nf, 1/nf] | scratch of normalize_pow2
struct Env3Ws {
    double *H, *Y, *Wp, *g, *nf2;
    void* scratch;
    int64_t g1, g2, g3;                   // bytes of g each of the three GEMMs asks for
};
static int64_t env3_layout(int side, int64_t Dt, int64_t pd, int64_t Dt2, int64_t bl, int64_t br, int64_t pu, int64_t Db, int64_t Db2,
                           char* base, Env3Ws* out) {
    Env3Ws w;
    int64_t half, y, wp;                  // doubles of H, Y, Wp
    if (side == 0) {
        half = bl * pd * Dt2 * Db;
        y = br * Dt2 * Db * pu;
        wp = 0;
        w.g1 = gemm_ws_bytes(pd * Dt2, Db, Dt, bl);
        w.g2 = gemm_ws_bytes(Dt2 * Db, pu, bl * pd, br);
        w.g3 = gemm_ws_bytes(br * Dt2, Db2, Db * pu, 1);
    } else {
        half = pu * br * Dt2 * Db;
        y = bl * pd * Dt2 * Db;
        wp = bl * pd * pu * br;
        w.g1 = gemm_ws_bytes(br * Dt2, Db, Db2, pu);
        w.g2 = gemm_ws_bytes(bl * pd, Dt2 * Db, pu * br, 1);
        w.g3 = gemm_ws_bytes(Dt, Db, pd * Dt2, bl);
    }
    WsCarve ws{base};
    w.H = ws.take<double>(half * 8);
    w.Y = ws.take<double>(y * 8);
    w.Wp = ws.take<double>(wp * 8);
    w.g = ws.take<double>(std::max({w.g1, w.g2, w.g3}));
    w.nf2 = ws.take<double>(256);
    w.scratch = ws.take(NORMALIZE_SCRATCH_BYTES);
    if (out) *out = w;
    return ws.total();
}

// W[l][d][r][u] -> Wp[l][d][u][r]
__global__ __launch_bounds__(256) void mpo_swap_ru_kernel(const double* __restrict__ W, int64_t nld, int br, int pu, double* __restrict__ Wp) {
    const int64_t n = nld * br * pu;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t ld = e / (br * pu);
        const int rem = (int)(e - ld * br * pu), r = rem / pu, u = rem - r * pu;
        Wp[(ld * pu + u) * br + r] = W[e];
    }
}

// acc_out = acc_in + log2(nf): nf is an exact power of two (2^-1023 stands for an all-zero input, as in tn_nfactor)
__global__ void log2_acc_kernel(const double* __restrict__ nf2, const double* __restrict__ acc_in, double* __restrict__ acc_out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) acc_out[0] = (acc_in ? acc_in[0] : 0.0) + (double)ilogb(nf2[0]);
}

// ---- cell marginal -----------------------------------------------------------------------------------------------------
constexpr int64_t CM_QMAX = 16384;       // LDS holds the q entries of the table

// workspace of a cell closing: X (rows x ncols) | split-K scratch of its product
struct CellWs {
    double *X, *g;
    int64_t gb;                           // bytes of g the product asks for
};
static int64_t cell_layout(int64_t rows, int64_t ncols, int64_t K, char* base, CellWs* out) {
    const int64_t gb = gemm_ws_bytes(rows, ncols, K, 1);
    WsCarve ws{base};
    double* X = ws.take<double>(rows * ncols * 8);
    double* g = ws.take<double>(gb);
    if (out) *out = CellWs{X, g, gb};
    return ws.total();
}
// X[rows, (u,r)] = HL[rows, K] . HR[(u,r), K]^T
static int cell_product(hipStream_t st, const double* HL, const double* HR, int64_t rows, int64_t ncols, int64_t K, const CellWs& w) {
    return gemm(st, rows, ncols, K, 1.0, HL, K, 1, HR, 1, K, 0.0, w.X, ncols, 1, 1, 0, 0, 0, w.gb > 0 ? w.g : nullptr, w.gb);
}

// sum_{l,u} f[l,u] x[l,d,u,r] by one wave (every lane returns it; 0 for d or r outside the cell).  Lane i adds the products
// i, i + 64, ... of the (l,u) plane in that order, then the lanes are added in a butterfly: the order depends on nl nu alone.
__device__ __forceinline__ double cell_gather(const double* __restrict__ x, const double* __restrict__ f, int d, int r, int nl, int pd,
                                              int br, int nu, int lane) {
    const int nlu = nl * nu;
    double acc = 0.0;
    if (d >= 0 && d < pd && r >= 0 && r < br) {
        for (int i = lane; i < nlu; i += 64) {
            const int l = i / nu, u = i - l * nu;
            acc += f[i] * x[(((int64_t)l * pd + d) * nu + u) * br + r];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    return acc;
}

// one workgroup: wave w gathers the states s = w, w+4, ..., its lanes split the (l,u) sum
__global__ __launch_bounds__(256) void cluster_marginal_kernel(const double* __restrict__ X, const double* __restrict__ F,
                                                               const int32_t* __restrict__ dmap, const int32_t* __restrict__ rmap, int q,
                                                               int nl, int pd, int br, int nu, const double* __restrict__ log2L,
                                                               const double* __restrict__ log2R, double* __restrict__ P,
                                                               double* __restrict__ minP, double* __restrict__ log2z) {
    extern __shared__ double sP[];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int s = wv; s < q; s += 4) {
        const double acc = cell_gather(X, F + (int64_t)s * nl * nu, dmap[s], rmap[s], nl, pd, br, nu, lane);
        if (lane == 0) sP[s] = acc;
    }
    __syncthreads();
    double mn = 1.7e308, part = 0.0;
    for (int s = tid; s < q; s += 256) { mn = fmin(mn, sP[s]); part += sP[s]; }
    const double raw = block_tree_sum(part, red);
    double mPn = block_tree_min(mn, red);
    if (mPn < 0.0) {                                   // the rule of tn_calc_pn (reference tnac4o.py:1796-1799)
        const double a = fabs(mPn);
        double cnt = 0.0;
        for (int s = tid; s < q; s += 256)
            if (sP[s] < a) { sP[s] = a; cnt += 1.0; }
        mPn *= block_tree_sum(cnt, red);
    }
    part = 0.0;
    for (int s = tid; s < q; s += 256) part += sP[s];
    const double no = block_tree_sum(part, red);
    if (no > 0.0) {
        const double inv = 1.0 / no;
        for (int s = tid; s < q; s += 256) P[s] = sP[s] * inv;
        mPn *= inv;
    } else {                                           // all zeros -> uniform, flag -1 (as tn_calc_pn)
        for (int s = tid; s < q; s += 256) P[s] = sP[s] + 1.0 / (double)q;
        mPn = -1.0;
    }
    if (tid == 0) {
        minP[0] = mPn;
        log2z[0] = log2(raw) + (log2L ? log2L[0] : 0.0) + (log2R ? log2R[0] : 0.0);
    }
}

// ---- nearest-neighbour bond marginals ----------------------------------------------------------------------------------
// Pl[s,l] = sum_u F[s,l,u] X[l,dmap[s],u,rmap[s]] and Pu[s,u] = sum_l (the same products): the joint law of the cell's state
// with its left and with its upper bond index.  Launch 1 spreads the states over the device (one workgroup per state); launch 2
// is one workgroup that normalises both tables by the same total.

// one workgroup per state s.  The (l,u) plane is walked in tiles of TL rows x TU columns, TU = min(pu, 256), one product per
// lane; a tile goes through LDS, lanes t < TL add up its rows (the u sums of Pl) and lanes t < TU its columns (the l sums of
// Pu).  Every table entry has one owning lane and a fixed summation order.
__global__ __launch_bounds__(256) void bond_gather_kernel(const double* __restrict__ X, const double* __restrict__ F,
                                                          const int32_t* __restrict__ dmap, const int32_t* __restrict__ rmap, int nl,
                                                          int pd, int br, int nu, double* __restrict__ Pl, double* __restrict__ Pu) {
    __shared__ double tile[256];
    const int s = blockIdx.x, t = threadIdx.x;
    const int d = dmap[s], r = rmap[s];
    const bool ok = d >= 0 && d < pd && r >= 0 && r < br;
    const int TU = nu < 256 ? nu : 256, TL = 256 / TU;
    const int i = t / TU, j = t - i * TU;
    const double* f = F + (int64_t)s * nl * nu;
    double* pl = Pl + (int64_t)s * nl;
    double* pu = Pu + (int64_t)s * nu;
    for (int u0 = 0; u0 < nu; u0 += TU) {
        const int u = u0 + j;
        double cacc = 0.0;
        for (int l0 = 0; l0 < nl; l0 += TL) {
            const int l = l0 + i;
            double v = 0.0;
            if (ok && i < TL && l < nl && u < nu) v = f[(int64_t)l * nu + u] * X[(((int64_t)l * pd + d) * nu + u) * br + r];
            tile[t] = v;
            __syncthreads();
            if (t < TL && l0 + t < nl) {
                double racc = 0.0;
                for (int c = 0; c < TU; ++c) racc += tile[t * TU + c];
                pl[l0 + t] = u0 == 0 ? racc : pl[l0 + t] + racc;
            }
            if (t < TU)
                for (int c = 0; c < TL; ++c) cacc += tile[c * TU + t];
            __syncthreads();
        }
        if (t < TU && u < nu) pu[u] = cacc;
    }
}

// one workgroup: T = sum of the raw Pl, both tables divided by it, the smallest entry, log2 of the row contraction
__global__ __launch_bounds__(256) void bond_finish_kernel(const double* __restrict__ Rl, const double* __restrict__ Ru, int64_t nlq,
                                                          int64_t nuq, const double* __restrict__ log2L, const double* __restrict__ log2R,
                                                          double* __restrict__ Pl, double* __restrict__ Pu, double* __restrict__ minB,
                                                          double* __restrict__ log2z) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double part = 0.0;
    for (int64_t e = tid; e < nlq; e += 256) part += Rl[e];
    const double raw = block_tree_sum(part, red);
    double mn = 0.0;
    if (raw > 0.0) {
        const double inv = 1.0 / raw;
        for (int64_t e = tid; e < nlq; e += 256) { const double v = Rl[e] * inv; Pl[e] = v; mn = fmin(mn, v); }
        for (int64_t e = tid; e < nuq; e += 256) { const double v = Ru[e] * inv; Pu[e] = v; mn = fmin(mn, v); }
        mn = block_tree_min(mn, red);
    } else {                                           // all zeros -> uniform, flag -1 (as cluster_marginal_kernel)
        for (int64_t e = tid; e < nlq; e += 256) Pl[e] = 1.0 / (double)nlq;
        for (int64_t e = tid; e < nuq; e += 256) Pu[e] = 1.0 / (double)nuq;
        mn = -1.0;
    }
    if (tid == 0) {
        minB[0] = mn;
        log2z[0] = log2(raw) + (log2L ? log2L[0] : 0.0) + (log2R ? log2R[0] : 0.0);
    }
}

// workspace of the bond marginal: the cell's | raw Pl (q x bl) | raw Pu (q x pu)
struct BondWs {
    CellWs cell;
    double *Rl, *Ru;
};
static int64_t bond_layout(int64_t q, int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K, char* base, BondWs* out) {
    WsCarve ws{base};
    ws.take(cell_layout(bl * pd, pu * br, K, base, out ? &out->cell : nullptr));
    double* Rl = ws.take<double>(q * bl * 8);
    double* Ru = ws.take<double>(q * pu * 8);
    if (out) { out->Rl = Rl; out->Ru = Ru; }
    return ws.total();
}

// ---- in-line two-point functions: a stack of left environments (tnac4o.calculate_correlation_function) -----------------
// A stack E (nE, bl, Dt, Db) holds the plain left environment in slot 0 and, in the others, left environments with an operator
// inserted at an earlier cell.  One step carries all of them through the plain site Wops[0] and opens nop new slots, slot 0
// through the operator-weighted sites Wops[1 .. nop] (tn_mpo_from_factor_ops).  The three products of the left step of env3:
//   HL[(e,l)][(d,t'), b] = At^T . E[(e,l)]                          ONE launch, batch (e,l):  M = pd Dt2, N = Db, K = Dt
//   Y [e][r][(t',b), u]  = HL[e]^T[(t',b),(l,d)] . W0[(l,d), r, u]
//        r and u lie on both sides of (t',b) in Y (the last product needs (b,u) together) and the batch index is taken by e, so
//        one of them is walked on the host: min(br, pu) launches, batch e, M = Dt2 Db, N = pu (or br), K = bl pd
//   Y [nE+a][r]          = HL[0]^T . Wq[a][r]                       ONE launch, batch (a,r), after the op planes are permuted to
//        Wq[a][r][(l,d)][u] (nop bl pd br pu doubles, the only copy): there the batch index is free, HL[0] is shared
//   out[(e,r,t'), b']    = Y[(e,r,t'), (b,u)] . Ab[(b,u), b']        ONE launch:  M = (nE + nop) br Dt2, N = Db2, K = Db pu
// Every slot is divided by the power-of-two nfactor of slot 0 (exact), whose log2 is added to the running total: ratios between
// slots carry no factor.  No step depends on the number of slots through anything but the batch counts.
struct Env3StackWs {
    double *H, *Y, *Wq, *g, *nf2;         // first products (own_half), second products, permuted operator planes, split-K scratch, [nf, 1/nf]
    void* scratch;                        // of normalize_pow2
    int64_t wq;                           // doubles of Wq
    int64_t g1, g2, g2o, g3;              // bytes of g each GEMM asks for
    bool walk_u;                          // the middle product walks u (pu < br) instead of r
};
static int64_t env3_stack_layout(int64_t nE, int64_t nop, int64_t Dt, int64_t pd, int64_t Dt2, int64_t bl, int64_t br, int64_t pu, int64_t Db,
                                 int64_t Db2, bool own_half, char* base, Env3StackWs* out) {
    Env3StackWs w;
    w.wq = nop * br * bl * pd * pu;
    w.walk_u = pu < br;
    w.g1 = gemm_ws_bytes(pd * Dt2, Db, Dt, nE * bl);
    w.g2 = gemm_ws_bytes(Dt2 * Db, w.walk_u ? br : pu, bl * pd, nE);
    w.g2o = nop > 0 ? gemm_ws_bytes(Dt2 * Db, pu, bl * pd, nop * br) : 0;
    w.g3 = gemm_ws_bytes((nE + nop) * br * Dt2, Db2, Db * pu, 1);
    WsCarve ws{base};
    w.H = own_half ? ws.take<double>(nE * bl * pd * Dt2 * Db * 8) : nullptr;
    w.Y = ws.take<double>((nE + nop) * br * Dt2 * Db * pu * 8);
    w.Wq = ws.take<double>(w.wq * 8);
    w.g = ws.take<double>(std::max({w.g1, w.g2, w.g2o, w.g3}));
    w.nf2 = ws.take<double>(256);
    w.scratch = ws.take(NORMALIZE_SCRATCH_BYTES);
    if (out) *out = w;
    return ws.total();
}

// Wops[1 + a][l][d][r][u] -> Wq[a][r][(l,d)][u]
__global__ __launch_bounds__(256) void mpo_ops_by_r_kernel(const double* __restrict__ Wops, int64_t nop, int64_t nld, int br, int pu,
                                                           double* __restrict__ Wq) {
    const int64_t plane = nld * br * pu, n = nop * plane;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t a = e / plane, rem = e - a * plane, ld = rem / (br * pu);
        const int ru = (int)(rem - ld * br * pu), r = ru / pu, u = ru - r * pu;
        Wq[((a * br + r) * nld + ld) * pu + u] = Wops[plane + e];
    }
}

static bool stack_dims_ok(int64_t nE, int64_t nop) { return nE >= 1 && nop >= 0; }

// ---- closing every slot of a stack at one cell -------------------------------------------------------------------------
//   X[e][l,d,u,r] = sum_K HL[e][(l,d),K] HR[(u,r),K]                 ONE launch:  M = nE bl pd, N = pu br, K = Dt2 Db
//   D[e][s] = sum_{l,u} F[s,l,u] X[e][l,dmap[s],u,rmap[s]]           raw: no negativity rule, no division
// One wave per (slot, state) runs cell_gather, the four waves of a workgroup take four slots of one state (they share the row of F).
// X is read once in all (a chimera cell sends every (d,r) to one state), at the stride of its r index.
__global__ __launch_bounds__(256) void stack_gather_kernel(const double* __restrict__ X, const double* __restrict__ F,
                                                           const int32_t* __restrict__ dmap, const int32_t* __restrict__ rmap, int q, int nE,
                                                           int nl, int pd, int br, int nu, double* __restrict__ D) {
    const int s = blockIdx.x, lane = threadIdx.x & 63;
    const int e = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (e >= nE) return;                                   // whole wave leaves together
    const double acc = cell_gather(X + (int64_t)e * nl * pd * nu * br, F + (int64_t)s * nl * nu, dmap[s], rmap[s], nl, pd, br, nu, lane);
    if (lane == 0) D[(int64_t)e * q + s] = acc;
}

}  // namespace tn

using namespace tn;

extern "C" {

int64_t tn_env3_ws_bytes(int side, int64_t Dt, int64_t pd, int64_t Dt2, int64_t bl, int64_t br, int64_t pu, int64_t Db, int64_t Db2) {
    if ((side != 0 && side != 1) || !dims_ok({Dt, pd, Dt2, bl, br, pu, Db, Db2})) return 0;
    return env3_layout(side, Dt, pd, Dt2, bl, br, pu, Db, Db2, nullptr, nullptr);
}

int tn_env3(int side, const double* E, const double* At, const double* W, const double* Ab, int64_t Dt, int64_t pd, int64_t Dt2, int64_t bl,
            int64_t br, int64_t pu, int64_t Db, int64_t Db2, const double* log2nf_in, double* out, double* log2nf_out, double* half_out,
            void* ws, int64_t ws_bytes, void* stream) {
    TN_CHECK_ARG(side == 0 || side == 1, "side must be 0 (left step) or 1 (right step)");
    TN_CHECK_ARG(E && At && W && Ab && out && log2nf_out && ws, "null operand");
    TN_CHECK_ARG(dims_ok({Dt, pd, Dt2, bl, br, pu, Db, Db2}), "non-positive dimension");
    Env3Ws w;
    TN_CHECK_ARG(ws_bytes >= env3_layout(side, Dt, pd, Dt2, bl, br, pu, Db, Db2, (char*)ws, &w), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double* H = half_out ? half_out : w.H;
    double* g1 = w.g1 > 0 ? w.g : nullptr;
    double* g2 = w.g2 > 0 ? w.g : nullptr;
    double* g3 = w.g3 > 0 ? w.g : nullptr;
    int rc;
    if (side == 0) {
        // HL_l[(d,t'), b] = At^T[(d,t'), t] . EL_l[t, b]
        if ((rc = gemm(st, pd * Dt2, Db, Dt, 1.0, At, 1, pd * Dt2, E, Db, 1, 0.0, H, Db, 1, bl, 0, Dt * Db, pd * Dt2 * Db, g1, w.g1))) return rc;
        // Y_r[(t',b), u] = HL^T[(t',b), (l,d)] . W_r[(l,d), u]
        if ((rc = gemm(st, Dt2 * Db, pu, bl * pd, 1.0, H, 1, Dt2 * Db, W, br * pu, 1, 0.0, w.Y, pu, 1, br, 0, pu, Dt2 * Db * pu, g2, w.g2)))
            return rc;
        // EL'[(r,t'), b'] = Y[(r,t'), (b,u)] . Ab[(b,u), b']
        if ((rc = gemm(st, br * Dt2, Db2, Db * pu, 1.0, w.Y, Db * pu, 1, Ab, Db2, 1, 0.0, out, Db2, 1, 1, 0, 0, 0, g3, w.g3))) return rc;
        if ((rc = normalize_pow2(st, out, br * Dt2 * Db2, w.nf2, w.scratch, NORMALIZE_SCRATCH_BYTES))) return rc;
    } else {
        // HR_u[(r,t'), b] = ER[(r,t'), b'] . Ab_u[b', b]     (Ab_u[b', b] = Ab[b, u, b'])
        if ((rc = gemm(st, br * Dt2, Db, Db2, 1.0, E, Db2, 1, Ab, 1, pu * Db2, 0.0, H, Db, 1, pu, 0, Db2, br * Dt2 * Db, g1, w.g1))) return rc;
        const int64_t nw = bl * pd * pu * br;
        int64_t nbk = cdiv(nw, 256);
        if (nbk > 1024) nbk = 1024;
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(mpo_swap_ru_kernel, dim3((unsigned)nbk), dim3(256), 0, st, W, bl * pd, (int)br, (int)pu, w.Wp));
        TN_CHECK_LAUNCH("mpo_swap_ru_kernel");
        // Y[(l,d), (t',b)] = W'[(l,d), (u,r)] . HR[(u,r), (t',b)]
        if ((rc = gemm(st, bl * pd, Dt2 * Db, pu * br, 1.0, w.Wp, pu * br, 1, H, Dt2 * Db, 1, 0.0, w.Y, Dt2 * Db, 1, 1, 0, 0, 0, g2, w.g2))) return rc;
        // ER_l[t, b] = At[t, (d,t')] . Y_l[(d,t'), b]
        if ((rc = gemm(st, Dt, Db, pd * Dt2, 1.0, At, pd * Dt2, 1, w.Y, Db, 1, 0.0, out, Db, 1, bl, 0, pd * Dt2 * Db, Dt * Db, g3, w.g3))) return rc;
        if ((rc = normalize_pow2(st, out, bl * Dt * Db, w.nf2, w.scratch, NORMALIZE_SCRATCH_BYTES))) return rc;
    }
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(log2_acc_kernel, dim3(1), dim3(64), 0, st, w.nf2, log2nf_in, log2nf_out));
    TN_CHECK_LAUNCH("log2_acc_kernel");
    return 0;
}

int64_t tn_cluster_marginal_ws_bytes(int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K) {
    if (!dims_ok({bl, pd, br, pu, K})) return 0;
    return cell_layout(bl * pd, pu * br, K, nullptr, nullptr);
}

int tn_cluster_marginal(const double* HL, const double* HR, const double* F, const int32_t* dmap, const int32_t* rmap, int64_t q, int64_t bl,
                        int64_t pd, int64_t br, int64_t pu, int64_t K, const double* log2L, const double* log2R, double* P, double* minP,
                        double* log2z, void* ws, int64_t ws_bytes, void* stream) {
    TN_CHECK_ARG(HL && HR && F && dmap && rmap && P && minP && log2z && ws, "null operand");
    TN_CHECK_ARG(dims_ok({q, bl, pd, br, pu, K}), "non-positive dimension");
    TN_CHECK_ARG(q <= CM_QMAX, "more than 16384 cell states");
    CellWs w;
    TN_CHECK_ARG(ws_bytes >= cell_layout(bl * pd, pu * br, K, (char*)ws, &w), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = cell_product(st, HL, HR, bl * pd, pu * br, K, w))) return rc;
    const size_t lds = (size_t)q * 8;
    if (lds > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)cluster_marginal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(cluster_marginal_kernel, dim3(1), dim3(256), lds, st, w.X, F, dmap, rmap, (int)q, (int)bl,
                                                     (int)pd, (int)br, (int)pu, log2L, log2R, P, minP, log2z));
    TN_CHECK_LAUNCH("cluster_marginal_kernel");
    return 0;
}

int64_t tn_cluster_bond_marginal_ws_bytes(int64_t q, int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K) {
    if (!dims_ok({q, bl, pd, br, pu, K})) return 0;
    return bond_layout(q, bl, pd, br, pu, K, nullptr, nullptr);
}

int tn_cluster_bond_marginal(const double* HL, const double* HR, const double* F, const int32_t* dmap, const int32_t* rmap, int64_t q,
                             int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K, const double* log2L, const double* log2R, double* Pl,
                             double* Pu, double* minB, double* log2z, void* ws, int64_t ws_bytes, void* stream) {
    TN_CHECK_ARG(HL && HR && F && dmap && rmap && Pl && Pu && minB && log2z && ws, "null operand");
    TN_CHECK_ARG(dims_ok({q, bl, pd, br, pu, K}), "non-positive dimension");
    TN_CHECK_ARG(q <= CM_QMAX, "more than 16384 cell states");
    BondWs w;
    TN_CHECK_ARG(ws_bytes >= bond_layout(q, bl, pd, br, pu, K, (char*)ws, &w), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = cell_product(st, HL, HR, bl * pd, pu * br, K, w.cell))) return rc;
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(bond_gather_kernel, dim3((unsigned)q), dim3(256), 0, st, w.cell.X, F, dmap, rmap, (int)bl,
                                                     (int)pd, (int)br, (int)pu, w.Rl, w.Ru));
    TN_CHECK_LAUNCH("bond_gather_kernel");
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(bond_finish_kernel, dim3(1), dim3(256), 0, st, w.Rl, w.Ru, q * bl, q * pu, log2L, log2R,
                                                     Pl, Pu, minB, log2z));
    TN_CHECK_LAUNCH("bond_finish_kernel");
    return 0;
}

int64_t tn_env3_stack_ws_bytes(int64_t nE, int64_t nop, int64_t Dt, int64_t pd, int64_t Dt2, int64_t bl, int64_t br, int64_t pu, int64_t Db,
                               int64_t Db2, int own_half) {
    if (!stack_dims_ok(nE, nop) || !dims_ok({Dt, pd, Dt2, bl, br, pu, Db, Db2})) return 0;
    return env3_stack_layout(nE, nop, Dt, pd, Dt2, bl, br, pu, Db, Db2, own_half != 0, nullptr, nullptr);
}

int tn_env3_stack(const double* E, const double* At, const double* Wops, const double* Ab, int64_t nE, int64_t nop, int64_t Dt, int64_t pd,
                  int64_t Dt2, int64_t bl, int64_t br, int64_t pu, int64_t Db, int64_t Db2, const double* log2nf_in, double* out,
                  double* log2nf_out, double* half_out, void* ws, int64_t ws_bytes, void* stream) {
    TN_CHECK_ARG(E && At && Wops && Ab && out && log2nf_out && ws, "null operand");
    TN_CHECK_ARG(stack_dims_ok(nE, nop), "the stack needs at least the plain slot and a non-negative operator count");
    TN_CHECK_ARG(dims_ok({Dt, pd, Dt2, bl, br, pu, Db, Db2}), "non-positive dimension");
    Env3StackWs w;
    TN_CHECK_ARG(ws_bytes >= env3_stack_layout(nE, nop, Dt, pd, Dt2, bl, br, pu, Db, Db2, half_out == nullptr, (char*)ws, &w),
                 "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    double* H = half_out ? half_out : w.H;
    double* g1 = w.g1 > 0 ? w.g : nullptr;
    double* g2 = w.g2 > 0 ? w.g : nullptr;
    double* g2o = w.g2o > 0 ? w.g : nullptr;
    double* g3 = w.g3 > 0 ? w.g : nullptr;
    double* Y = w.Y;
    const int64_t KD = Dt2 * Db, LD = bl * pd, slotY = br * KD * pu, slotO = br * Dt2 * Db2;
    int rc;
    // HL[(e,l)][(d,t'), b] = At^T[(d,t'), t] . E[(e,l)][t, b]
    if ((rc = gemm(st, pd * Dt2, Db, Dt, 1.0, At, 1, pd * Dt2, E, Db, 1, 0.0, H, Db, 1, nE * bl, 0, Dt * Db, pd * KD, g1, w.g1))) return rc;
    // Y[e][r][(t',b), u] = HL[e]^T[(t',b), (l,d)] . W0[(l,d), r, u]
    if (w.walk_u) {
        for (int64_t u = 0; u < pu; ++u)
            if ((rc = gemm(st, KD, br, LD, 1.0, H, 1, KD, Wops + u, br * pu, pu, 0.0, Y + u, pu, KD * pu, nE, LD * KD, 0, slotY, g2, w.g2)))
                return rc;
    } else {
        for (int64_t r = 0; r < br; ++r)
            if ((rc = gemm(st, KD, pu, LD, 1.0, H, 1, KD, Wops + r * pu, br * pu, 1, 0.0, Y + r * KD * pu, pu, 1, nE, LD * KD, 0, slotY, g2, w.g2)))
                return rc;
    }
    if (nop > 0) {
        int64_t nbk = cdiv(w.wq, 256);
        if (nbk > 1024) nbk = 1024;
        TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(mpo_ops_by_r_kernel, dim3((unsigned)nbk), dim3(256), 0, st, Wops, nop, LD, (int)br, (int)pu, w.Wq));
        TN_CHECK_LAUNCH("mpo_ops_by_r_kernel");
        // Y[nE + a][r][(t',b), u] = HL[0]^T[(t',b), (l,d)] . Wq[a][r][(l,d), u]
        if ((rc = gemm(st, KD, pu, LD, 1.0, H, 1, KD, w.Wq, pu, 1, 0.0, Y + nE * slotY, pu, 1, nop * br, 0, LD * pu, KD * pu, g2o, w.g2o)))
            return rc;
    }
    // out[(e,r,t'), b'] = Y[(e,r,t'), (b,u)] . Ab[(b,u), b']
    if ((rc = gemm(st, (nE + nop) * br * Dt2, Db2, Db * pu, 1.0, Y, Db * pu, 1, Ab, Db2, 1, 0.0, out, Db2, 1, 1, 0, 0, 0, g3, w.g3))) return rc;
    if ((rc = normalize_pow2(st, out, slotO, w.nf2, w.scratch, NORMALIZE_SCRATCH_BYTES))) return rc;
    if ((rc = scale_by(st, out + slotO, (nE + nop - 1) * slotO, w.nf2 + 1))) return rc;
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(log2_acc_kernel, dim3(1), dim3(64), 0, st, w.nf2, log2nf_in, log2nf_out));
    TN_CHECK_LAUNCH("log2_acc_kernel");
    return 0;
}

int64_t tn_stack_cell_law_ws_bytes(int64_t nE, int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K) {
    if (!dims_ok({nE, bl, pd, br, pu, K})) return 0;
    return cell_layout(nE * bl * pd, pu * br, K, nullptr, nullptr);
}

int tn_stack_cell_law(const double* HL, const double* HR, const double* F, const int32_t* dmap, const int32_t* rmap, int64_t q, int64_t nE,
                      int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K, double* D, void* ws, int64_t ws_bytes, void* stream) {
    TN_CHECK_ARG(HL && HR && F && dmap && rmap && D && ws, "null operand");
    TN_CHECK_ARG(dims_ok({q, nE, bl, pd, br, pu, K}), "non-positive dimension");
    TN_CHECK_ARG(q < (int64_t)1 << 31 && cdiv(nE, 4) <= 65535 && bl * pu < (int64_t)1 << 31, "too many states or slots for one launch");
    CellWs w;
    TN_CHECK_ARG(ws_bytes >= cell_layout(nE * bl * pd, pu * br, K, (char*)ws, &w), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = cell_product(st, HL, HR, nE * bl * pd, pu * br, K, w))) return rc;
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(stack_gather_kernel, dim3((unsigned)q, (unsigned)cdiv(nE, 4)), dim3(256), 0, st, w.X, F, dmap,
                                                     rmap, (int)q, (int)nE, (int)bl, (int)pd, (int)br, (int)pu, D));
    TN_CHECK_LAUNCH("stack_gather_kernel");
    return 0;
}

}  // extern "C"
