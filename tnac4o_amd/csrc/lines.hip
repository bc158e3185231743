// Line sweeps over given configurations (no counterpart in the reference): tn_line_sweep resamples (heat bath) or minimises (quench)
// WHOLE lattice rows and columns exactly, under the energy of the cell sweeps (relax.hip).  With the lines next to it given, a line is a
// chain of cells: for a row (a column exchanges E1 / left_map / nx with E4 / up_map / ny)
//     side energy   a_x(s) = ((1.0 Es[s] + E4_x[s, U]) + B.E4[sb, B.up_map(s)])       (a term is absent at a lattice edge)
//     coupling      E1_x[s_x, r_{x-1}(s_{x-1})],   r_{x-1}(s') = left_map_x ? left_map_x[s'] : s'
// heat bath at beta (forward filtering, backward sampling; linear domain):
//     lambda_0(s) = w_0(s),  lambda_x(s) = w_x(s) sum_r F_x[r] T_x[s, r],  w_x(s) = exp(-beta (a_x(s) - min a_x)),
//     T_x[s, r] = exp(-beta (E1_x[s, r] - min E1_x)),  F_x[r] = (sum over s' with r_{x-1}(s') = r of lambda_{x-1}(s')) / max lambda_{x-1};
//     cell n-1 is drawn from lambda_{n-1}, cell x < n-1 from lambda_x(s) T_{x+1}[s_{x+1}, r_x(s)], each by tn_cell_sweep's rule
// quench: the same recursion in (min, +): Lambda_x(s) = a_x(s) + min_r (mu_x[r] + E1_x[s, r]), mu_x[r] = min over s' with r_{x-1}(s') = r of
//     Lambda_{x-1}(s'); the line moves when E* = min Lambda_{n-1} lies strictly below its energy c (c_0 = a_0(s_0), c_x = a_x(s_x) +
//     (c_{x-1} + E1_x[s_x, r]); +inf with a state outside its cell), to the minimiser that is smallest in the order (s_{n-1}, ..., s_0).
// A pass updates the lines of even index, then those of odd index: lines of one parity share no coupling, so one launch serves a parity in
// place.  A workgroup walks (line, tile of samples) units; a GROUP of W lanes (8, 32 or 64 by the largest q of the lattice) serves one
// sample, state s on lane s % W.  Per group only the messages F_x (mu_x) of the line and one vector of q numbers are kept -- in LDS when
// the workgroup's share fits 48 KiB, else in a scratch of the workspace sized by the grid -- and lambda_x (Lambda_x) is evaluated again
// on the way back.  T_x is computed once per call into the workspace, transposed, for as many tables as fit TN_LINE_SWEEP_TABLES bytes
// (default and at most 32 MiB, 0: none); the others evaluate the same expression where they need it: the same bits.
// A state outside [0, q) of its cell is never used as an index: as a neighbour it is read as 0.
#include "walk.h"
#include "sweep.h"

#pragma clang fp contract(off)

namespace tn {

namespace {

constexpr int64_t LINE_TABLE_BYTES = (int64_t)32 << 20;   // the arena of the transfer tables T_x (TN_LINE_SWEEP_TABLES caps its use)
constexpr int64_t LINE_SCRATCH_BYTES = (int64_t)16 << 20; // the per-group vectors of the workgroups that do not keep them in LDS
constexpr int64_t LINE_LDS_BYTES = 48 * 1024;              // ... and the most a workgroup keeps in LDS
constexpr int64_t LINE_MAX_BLOCKS = 8192;
constexpr int LINE_BUILD_BLOCKS = 8;                       // workgroups per table of line_tables_kernel
constexpr double LINE_BETA_RANGE = 300.0;                  // the range guard: beta (max - min) of every chain table

// a cell as a link of the chain of direction dir (0: rows, 1: columns): chain table Ec / cmap / ccols, side table Sd / smap / scols
struct ChainCell {
    const double *Es, *Ec, *Sd;
    const int64_t *cmap, *smap;
    int q, ccols, scols;
};
__device__ __forceinline__ ChainCell chain_cell(const SweepCell& c, int dir) {
    ChainCell o;
    o.Es = c.Es; o.q = c.q;
    if (dir == 0) { o.Ec = c.E1; o.cmap = c.left_map; o.ccols = c.e1cols; o.Sd = c.E4; o.smap = c.up_map; o.scols = c.e4cols; }
    else { o.Ec = c.E4; o.cmap = c.up_map; o.ccols = c.e4cols; o.Sd = c.E1; o.smap = c.left_map; o.scols = c.e1cols; }
    return o;
}

__device__ __forceinline__ int line_in_cell(int s, int q) { return (s >= 0 && s < q) ? s : 0; }

// the one expression of a transfer-table entry, in the table and where it is evaluated in place
__device__ __forceinline__ double transfer_entry(double beta, double e, double emin) { return exp(-beta * (e - emin)); }

struct LineArgs {
    const SweepCell* cells;
    int16_t* states;
    const double* uniforms;            // row 0 = cell 0 of this pass
    uint8_t* chg;                      // [cell][sample]
    const double* ranges;              // [dir][cell][min, max] of the chain tables (heat bath)
    const int64_t* toff;               // [dir][cell]: offset (doubles) of the transposed T in tables, -1: evaluated in place
    const double* tables;
    double* scratch;
    int64_t Nx, Ny, M, ldu, per, maxq, nunits, ntiles;
    int dir, parity, use_lds;
    double beta;
};

// side energy of one cell for one sample
struct Side {
    const double *Es, *Sd, *Arow;
    const int64_t* amap;
    int64_t scols, U;
    bool hb, ha;
};
__device__ __forceinline__ double side_energy(const Side& sd, int s) {
    double e = 1.0 * sd.Es[s];
    if (sd.hb) e = e + sd.Sd[(int64_t)s * sd.scols + sd.U];
    if (sd.ha) e = e + sd.Arow[sd.amap ? sd.amap[s] : (int64_t)s];
    return e;
}
__device__ __forceinline__ Side make_side(const LineArgs& a, const ChainCell& c, const int16_t* row, int64_t k, int64_t so, bool hb, bool ha) {
    Side sd;
    sd.Es = c.Es; sd.Sd = c.Sd; sd.scols = c.scols; sd.hb = hb; sd.ha = ha; sd.U = 0; sd.Arow = nullptr; sd.amap = nullptr;
    if (hb) {
        const int sb = line_in_cell(row[k - so], a.cells[k - so].q);
        sd.U = c.smap ? c.smap[sb] : (int64_t)sb;
    }
    if (ha) {
        const ChainCell A = chain_cell(a.cells[k + so], a.dir);
        const int sa = line_in_cell(row[k + so], A.q);
        sd.Arow = A.Sd + (int64_t)sa * A.scols;
        sd.amap = A.smap;
    }
    return sd;
}

// The chain table of a cell as the recursion reads it -- MODE 0: T = exp(-beta (Ec - min Ec)), MODE 1: Ec itself --: the transposed
// copy in the workspace when it was built, else the expression on the cell's own table
struct Transfer {
    const double *tp, *Ec;
    double emin, beta;
    int64_t q, ccols;
    template <int MODE>
    __device__ __forceinline__ double at(int64_t s, int64_t r) const {
        if (tp) return tp[r * q + s];
        return MODE == 0 ? transfer_entry(beta, Ec[s * ccols + r], emin) : Ec[s * ccols + r];
    }
};
template <int MODE>
__device__ __forceinline__ Transfer make_transfer(const LineArgs& a, const ChainCell& c, int64_t k) {
    const int64_t t = (int64_t)a.dir * a.Nx * a.Ny + k;
    Transfer T;
    T.tp = a.toff[t] >= 0 ? a.tables + a.toff[t] : nullptr;
    T.Ec = c.Ec; T.emin = MODE == 0 ? a.ranges[2 * t] : 0.0; T.beta = a.beta; T.q = c.q; T.ccols = c.ccols;
    return T;
}

// what the messages F of the left neighbour give state s: MODE 0 sum_r F[r] T[s, r], MODE 1 min_r (F[r] + Ec[s, r]), r ascending.  An
// empty column (F = 0, resp. +inf) leaves the result as it is, bit for bit, whether it is skipped or not: with a map and a built table
// every column is taken, so that the loads do not wait for a branch; otherwise (one column per state of the neighbour, most of them
// empty in the spare columns, or the expression evaluated in place) the empty ones are skipped.
template <int MODE>
__device__ __forceinline__ double line_message(const double* F, const Transfer& T, int64_t s, bool dense) {
    const double none = MODE == 0 ? 0.0 : std::numeric_limits<double>::infinity();
    double acc = none;
    if (dense && T.tp) {
        const double* tp = T.tp + s;
#pragma unroll 8
        for (int64_t r = 0; r < T.ccols; ++r) {
            const double t = tp[r * T.q];
            acc = MODE == 0 ? acc + F[r] * t : fmin(acc, F[r] + t);
        }
    } else {
        for (int64_t r = 0; r < T.ccols; ++r) {
            const double f = F[r];
            if (f != none) {
                const double t = T.at<MODE>(s, r);
                acc = MODE == 0 ? acc + f * t : fmin(acc, f + t);
            }
        }
    }
    return acc;
}

template <int W>
__device__ __forceinline__ double group_min(double v) {
#pragma unroll
    for (int o = W / 2; o >= 1; o >>= 1) v = fmin(v, __shfl_xor(v, o, W));
    return v;
}
template <int W>
__device__ __forceinline__ double group_max(double v) {
#pragma unroll
    for (int o = W / 2; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, W));
    return v;
}
template <int W>
__device__ __forceinline__ double group_scan(double v, int l) {       // inclusive over the group, lane order
#pragma unroll
    for (int o = 1; o < W; o <<= 1) {
        const double t = __shfl_up(v, o, W);
        if (l >= o) v += t;
    }
    return v;
}
// the smallest state attaining the minimum over the group: (value, state); a lane without a state holds state 0x7fffffff
template <int W>
__device__ __forceinline__ void group_argmin(double& be, int& bs) {
#pragma unroll
    for (int o = W / 2; o >= 1; o >>= 1) {
        const double oe = __shfl_xor(be, o, W);
        const int os = __shfl_xor(bs, o, W);
        if (os != 0x7fffffff && (bs == 0x7fffffff || oe < be || (oe == be && os < bs))) { be = oe; bs = os; }
    }
}

// vec[s] = a(s) for the states of this lane, and min_s a(s) over the group.  The loop is short and unrolled so that the loads of
// several chunks are in flight together (a lane past the last state evaluates state q - 1 again and keeps nothing).
template <int W>
__device__ __forceinline__ double side_to_vec(const Side& sd, int q, int l, double* vec) {
    double amin = std::numeric_limits<double>::infinity();
    const int nchunk = (q + W - 1) / W;
#pragma unroll 4
    for (int j = 0; j < nchunk; ++j) {
        const int s = j * W + l;
        const double e = side_energy(sd, s < q ? s : q - 1);
        if (s < q) vec[s] = e;
        amin = fmin(amin, e);
    }
    return group_min<W>(amin);
}

// MODE 0: heat bath, 1: quench.  Control flow is uniform over the workgroup (every group of a workgroup works on the same line; a group
// without a sample repeats the last one and writes nothing), so the barriers between a cell's vector and the next cell's messages hold.
template <int W, int MODE>
__global__ __launch_bounds__(256) void line_sweep_kernel(LineArgs a) {
    extern __shared__ double lds[];
    constexpr int G = 256 / W;
    const int tid = threadIdx.x, l = tid % W, g = tid / W;
    const int64_t ncell = a.Nx * a.Ny;
    const int64_t n = a.dir ? a.Ny : a.Nx, nl = a.dir ? a.Nx : a.Ny;          // cells of a line, lines
    const int64_t co = a.dir ? a.Nx : 1, so = a.dir ? 1 : a.Nx;               // index steps along / across the line
    double* vec = a.use_lds ? lds + (int64_t)g * a.per : a.scratch + ((int64_t)blockIdx.x * G + g) * a.per;
    double* msg = vec + a.maxq;
    const double inf = std::numeric_limits<double>::infinity();
    for (int64_t unit = blockIdx.x; unit < a.nunits; unit += gridDim.x) {
        const int64_t line = 2 * (unit / a.ntiles) + a.parity, tile = unit % a.ntiles;
        const int64_t k0 = a.dir ? line : line * a.Nx;
        const bool hb = line > 0, ha = line + 1 < nl;
        const int64_t mm = tile * G + g;
        const bool active = mm < a.M;
        const int64_t m = active ? mm : a.M - 1;
        int16_t* row = a.states + m * ncell;
        int64_t moff = 0;                                                       // where the messages of cell x start
        double ccur = 0.0;                                                      // quench: the energy of the line as it stands
        bool bad = false;
        // ---- forward
        for (int64_t x = 0; x < n; ++x) {
            const int64_t k = k0 + x * co;
            const ChainCell c = chain_cell(a.cells[k], a.dir);
            const Side sd = make_side(a, c, row, k, so, hb, ha);
            const int q = c.q, nchunk = (q + W - 1) / W;
            const double* F = msg + moff;
            double top = 0.0;
            // (a lane past the last state evaluates state q - 1 again and keeps nothing: the loads then wait for no branch)
            const bool dense = c.cmap != nullptr;
            const Transfer T = make_transfer<MODE>(a, c, k);
            const double amin = side_to_vec<W>(sd, q, l, vec);               // vec[s] = a(s): a lane reads back what it wrote
            if constexpr (MODE == 0) {
                for (int j = 0; j < nchunk; ++j) {
                    const int s = j * W + l, sc = s < q ? s : q - 1;
                    double w = exp(-a.beta * ((s < q ? vec[s] : amin) - amin));
                    if (x > 0) w = w * line_message<0>(F, T, sc, dense);
                    if (s < q) {
                        vec[s] = w;
                        top = fmax(top, w);
                    }
                }
                top = group_max<W>(top);
            } else {
                if (x > 0)
                    for (int j = 0; j < nchunk; ++j) {
                        const int s = j * W + l, sc = s < q ? s : q - 1;
                        const double v = (s < q ? vec[s] : amin) + line_message<1>(F, T, sc, dense);
                        if (s < q) vec[s] = v;
                    }
                const int cur = row[k];
                const int cc = line_in_cell(cur, q);
                bad = bad || cur != cc;
                const double acur = side_energy(sd, cc);
                if (x == 0) ccur = acur;
                else {
                    const int pq = a.cells[k - co].q;
                    const int ps = line_in_cell(row[k - co], pq);
                    const int64_t r = c.cmap ? c.cmap[ps] : (int64_t)ps;
                    ccur = acur + (ccur + c.Ec[(int64_t)cc * c.ccols + r]);
                }
            }
            if (x + 1 < n) {                                                    // the messages of the next cell
                const ChainCell nc = chain_cell(a.cells[k + co], a.dir);
                double* Fn = msg + (x > 0 ? moff + c.ccols : 0);
                __syncthreads();
                if (nc.cmap && nc.ccols <= W) {
                    // few columns: cp = the power of two that holds them; the W / cp parts of the group each gather an equal share of
                    // the states, and a butterfly over the parts adds the shares up (an order fixed by W, q and the columns alone)
                    int cp = 1;
                    while (cp < nc.ccols) cp <<= 1;
                    const int parts = W / cp, r = l % cp, part = l / cp;
                    const int len = (q + parts - 1) / parts, s0 = part * len, s1 = min(q, s0 + len);
                    double v = MODE == 0 ? 0.0 : inf;
#pragma unroll 16
                    for (int s = s0; s < s1; ++s) {                             // (both loads unconditional: they go out together)
                        const int64_t col = nc.cmap[s];
                        const double y = vec[s];
                        if (col == r) v = MODE == 0 ? v + y : fmin(v, y);
                    }
                    for (int o = cp; o < W; o <<= 1) {
                        const double t = __shfl_xor(v, o, W);
                        v = MODE == 0 ? v + t : fmin(v, t);
                    }
                    if (part == 0 && r < nc.ccols) Fn[r] = MODE == 0 ? v / top : v;
                } else
                for (int r = l; r < nc.ccols; r += W) {
                    double v;
                    if (nc.cmap) {
                        v = MODE == 0 ? 0.0 : inf;
                        for (int s = 0; s < q; ++s)
                            if (nc.cmap[s] == r) v = MODE == 0 ? v + vec[s] : fmin(v, vec[s]);
                    } else {
                        v = r < q ? vec[r] : (MODE == 0 ? 0.0 : inf);
                    }
                    Fn[r] = MODE == 0 ? v / top : v;
                }
                __syncthreads();
            }
            if (x > 0) moff += c.ccols;
        }
        // ---- backward
        int snext = 0;
        bool move = true;
        if constexpr (MODE == 1) {
            const int q = a.cells[k0 + (n - 1) * co].q, nchunk = (q + W - 1) / W;
            double be = inf;
            int bs = 0x7fffffff;
            for (int j = 0; j < nchunk; ++j) {
                const int s = j * W + l;
                if (s < q) { const double v = vec[s]; if (v < be || bs == 0x7fffffff) { be = v; bs = s; } }
            }
            group_argmin<W>(be, bs);
            move = be < (bad ? inf : ccur);
            snext = bs;
        }
        for (int64_t x = n - 1; x >= 0; --x) {
            const int64_t k = k0 + x * co;
            const ChainCell c = chain_cell(a.cells[k], a.dir);
            const int q = c.q, nchunk = (q + W - 1) / W;
            if (x > 0) moff -= c.ccols;
            const double* F = msg + moff;
            int news = snext;
            if (MODE == 0 || x < n - 1) {
                const Side sd = make_side(a, c, row, k, so, hb, ha);
                ChainCell nc = c;
                if (x + 1 < n) nc = chain_cell(a.cells[k + co], a.dir);
                const bool dense = c.cmap != nullptr;
                const Transfer T = make_transfer<MODE>(a, c, k);
                Transfer Tn = T;
                if (x + 1 < n) Tn = make_transfer<MODE>(a, nc, k + co);
                const double amin = side_to_vec<W>(sd, q, l, vec);
                if constexpr (MODE == 0) {
                    double carry = 0.0;
                    for (int j = 0; j < nchunk; ++j) {                          // weights into vec, their total
                        const int s = j * W + l, sc = s < q ? s : q - 1;
                        double w = exp(-a.beta * ((s < q ? vec[s] : amin) - amin));
                        if (x > 0) w = w * line_message<0>(F, T, sc, dense);
                        if (x + 1 < n) w = w * Tn.template at<0>(snext, nc.cmap ? nc.cmap[sc] : (int64_t)sc);
                        if (s < q) vec[s] = w;
                        else w = 0.0;
                        const double v = group_scan<W>(w, l);
                        carry = carry + __shfl(v, W - 1, W);
                    }
                    const double t = a.uniforms[k * a.ldu + m] * carry;
                    int first = 0x7fffffff, last = -1;
                    double carry2 = 0.0;
                    for (int j = 0; j < nchunk; ++j) {
                        const int s = j * W + l;
                        const double w = s < q ? vec[s] : 0.0;
                        const double v = group_scan<W>(w, l);
                        if (s < q && w > 0.0) {
                            last = s;
                            if (carry2 + v >= t && first == 0x7fffffff) first = s;
                        }
                        carry2 = carry2 + __shfl(v, W - 1, W);
                    }
#pragma unroll
                    for (int o = W / 2; o >= 1; o >>= 1) {
                        first = min(first, __shfl_xor(first, o, W));
                        last = max(last, __shfl_xor(last, o, W));
                    }
                    news = first != 0x7fffffff ? first : (last >= 0 ? last : line_in_cell(row[k], q));
                } else {
                    double be = inf;
                    int bs = 0x7fffffff;
                    for (int j = 0; j < nchunk; ++j) {
                        const int s = j * W + l, sc = s < q ? s : q - 1;
                        double v = s < q ? vec[s] : amin;
                        if (x > 0) v = v + line_message<1>(F, T, sc, dense);
                        v = v + Tn.template at<1>(snext, nc.cmap ? nc.cmap[sc] : (int64_t)sc);
                        if (s < q && (v < be || bs == 0x7fffffff)) { be = v; bs = s; }
                    }
                    group_argmin<W>(be, bs);
                    news = bs;
                }
            }
            snext = news;
            if (active && l == 0) {
                const int cur = row[k];
                const int put = move ? news : cur;
                if (put != cur) row[k] = (int16_t)put;
                a.chg[k * a.M + m] = put != cur ? 1 : 0;
            }
        }
        __syncthreads();                                                        // the next unit writes vec and msg again
    }
}

// [dir][cell]: min and max of the chain table (E1 for dir 0, E4 for dir 1); a cell without one gets 0, 0.  One workgroup per table.
__global__ __launch_bounds__(256) void line_ranges_kernel(const SweepCell* cells, int64_t ncell, double* ranges) {
    __shared__ double smin[256], smax[256];
    const int64_t t = blockIdx.x, k = t % ncell;
    const int dir = (int)(t / ncell);
    const ChainCell c = chain_cell(cells[k], dir);
    double mn = std::numeric_limits<double>::infinity(), mx = -mn;
    if (c.Ec) {
        const int64_t cnt = (int64_t)c.q * c.ccols;
        for (int64_t i = threadIdx.x; i < cnt; i += 256) { const double v = c.Ec[i]; mn = fmin(mn, v); mx = fmax(mx, v); }
    }
    smin[threadIdx.x] = mn; smax[threadIdx.x] = mx;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) {
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + o]);
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ranges[2 * t] = c.Ec ? smin[0] : 0.0;
        ranges[2 * t + 1] = c.Ec ? smax[0] : 0.0;
    }
}

// where the transposed T of every chain table of the directions in use goes: in table order while it fits `limit` bytes, else -1
__global__ void line_offsets_kernel(const SweepCell* cells, int64_t ncell, int dirs, int64_t limit, int64_t* toff) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t off = 0;
    for (int64_t t = 0; t < 2 * ncell; ++t) {
        const int dir = (int)(t / ncell);
        const ChainCell c = chain_cell(cells[t % ncell], dir);
        const int64_t cnt = (int64_t)c.q * c.ccols;
        const bool used = c.Ec && (dirs == 2 || dirs == dir);
        if (used && (off + cnt) * 8 <= limit) { toff[t] = off; off += cnt; }
        else toff[t] = -1;
    }
}

// the transposed tables: mode 0 T = exp(-beta (Ec - min Ec)) (the minimum from ranges), mode 1 Ec itself
__global__ __launch_bounds__(256) void line_tables_kernel(const SweepCell* cells, int64_t ncell, const double* ranges, const int64_t* toff, int mode,
                                                          double beta, double* tables) {
    const int64_t t = blockIdx.x / LINE_BUILD_BLOCKS, part = blockIdx.x % LINE_BUILD_BLOCKS;
    if (toff[t] < 0) return;
    const ChainCell c = chain_cell(cells[t % ncell], (int)(t / ncell));
    const int64_t cnt = (int64_t)c.q * c.ccols;
    const double emin = mode == 0 ? ranges[2 * t] : 0.0;
    double* T = tables + toff[t];
    for (int64_t i = part * 256 + threadIdx.x; i < cnt; i += (int64_t)LINE_BUILD_BLOCKS * 256)
        T[(i % c.ccols) * c.q + i / c.ccols] = mode == 0 ? transfer_entry(beta, c.Ec[i], emin) : c.Ec[i];
}

// moves of one pass from its flags: moves[m] = (first pass of the call ? 0 : moves[m]) + n, last[m] = (first pass of the sweep ? 0 : last[m]) + n
__global__ __launch_bounds__(256) void line_moves_kernel(const uint8_t* chg, int64_t ncell, int64_t M, int first_call, int first_pass, int32_t* moves,
                                                         int32_t* last) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    int32_t n = 0;
    for (int64_t k = 0; k < ncell; ++k) n += chg[k * M + m];
    if (moves) moves[m] = (first_call ? 0 : moves[m]) + n;
    if (last) last[m] = (first_pass ? 0 : last[m]) + n;
}

// the workspace of tn_line_sweep: the table of the cells, the flags of a pass, ranges and offsets of the chain tables, the arena of the
// transfer tables, the scratch of the groups.  Only the flags depend on M.
struct LineWs {
    SweepCell* cells;
    uint8_t* chg;
    double* ranges;
    int64_t* toff;
    double* tables;
    double* scratch;
    int64_t bytes;
};
LineWs line_layout(void* ws, int64_t Nx, int64_t Ny, int64_t M) {
    WsCarve w{(char*)ws};
    LineWs s;
    s.cells = w.take<SweepCell>(Nx * Ny * (int64_t)sizeof(SweepCell));
    s.chg = w.take<uint8_t>(Nx * Ny * M);
    s.ranges = w.take<double>(Nx * Ny * 4 * 8);
    s.toff = w.take<int64_t>(Nx * Ny * 2 * 8);
    s.tables = w.take<double>(LINE_TABLE_BYTES);
    s.scratch = w.take<double>(LINE_SCRATCH_BYTES);
    s.bytes = w.total();
    return s;
}

int64_t line_table_limit() { return std::min(std::max<int64_t>(env_i64("TN_LINE_SWEEP_TABLES", LINE_TABLE_BYTES), 0), LINE_TABLE_BYTES); }

template <int W>
int launch_lines(hipStream_t st, const LineArgs& a, int mode, int64_t nblocks, int64_t lds) {
    if (mode == 0) TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL((line_sweep_kernel<W, 0>), dim3((unsigned)nblocks), dim3(256), (size_t)lds, st, a));
    else TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL((line_sweep_kernel<W, 1>), dim3((unsigned)nblocks), dim3(256), (size_t)lds, st, a));
    TN_CHECK_LAUNCH("line_sweep_kernel");
    return 0;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int64_t tn_line_sweep_ws_bytes(int64_t Nx, int64_t Ny, int64_t M) {
    if (Nx < 1 || Ny < 1 || M < 1 || M >= ((int64_t)1 << 31)) return 0;             // 0: a shape the call refuses
    int64_t n = 0, b = 0;
    if (__builtin_mul_overflow(Nx, Ny, &n) || n >= ((int64_t)1 << 26) || __builtin_mul_overflow(n, M, &b) || b >= ((int64_t)1 << 60)) return 0;
    return line_layout(nullptr, Nx, Ny, M).bytes;
}

int tn_line_sweep(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int16_t* states, int mode, int lines, double beta, int64_t sweeps,
                  const double* uniforms, int64_t ldu, double* energy_out, int32_t* moves_out, int32_t* last_moves_out, void* ws, int64_t ws_bytes,
                  void* stream) {
    TN_CHECK_ARG(Nx >= 1 && Ny >= 1 && cells, "Nx, Ny: non-positive, or cells: null");
    TN_CHECK_ARG(M >= 1 && M < ((int64_t)1 << 31), "M: outside 1 .. 2^31 - 1");
    TN_CHECK_ARG(mode == 0 || mode == 1, "mode: 0 (heat bath) or 1 (quench)");
    TN_CHECK_ARG(lines >= 0 && lines <= 2, "lines: 0 (rows), 1 (columns) or 2 (both)");
    TN_CHECK_ARG(sweeps >= 0, "sweeps: negative");
    TN_CHECK_ARG(states && energy_out, "states / energy_out: null");
    if (mode == 0) {
        TN_CHECK_ARG(beta > 0.0 && beta <= std::numeric_limits<double>::max(), "beta: not positive or not finite");
        TN_CHECK_ARG(uniforms, "uniforms: null in heat-bath mode");
        TN_CHECK_ARG(ldu >= M, "ldu: rows of uniforms shorter than M");
    } else {
        TN_CHECK_ARG(!uniforms, "uniforms: must be null in quench mode");
    }
    const int64_t need = tn_line_sweep_ws_bytes(Nx, Ny, M);
    TN_CHECK_ARG(need > 0, "Nx x Ny x M: too large");
    const int64_t ncell = Nx * Ny;
    const int P = lines == 2 ? 2 : 1;
    TN_CHECK_ARG(mode == 1 || mul_fits({sweeps, P, ncell, ldu}), "sweeps x passes x cells x ldu: too large");
    SweepPlan plan;
    BS(sweep_plan(__func__, Nx, Ny, cells, M, plan));
    // what a group keeps: a vector over the states of a cell and the messages of the longest line of either direction in use
    int64_t maxq = 0, maxmsg = 0;
    for (int dir = 0; dir < 2; ++dir) {
        if (lines != 2 && lines != dir) continue;
        const int64_t nl = dir ? Nx : Ny, n = dir ? Ny : Nx;
        for (int64_t i = 0; i < nl; ++i) {
            int64_t sum = 0;
            for (int64_t x = 1; x < n; ++x) {
                const SweepCell& c = plan.tab[(size_t)(dir ? x * Nx + i : i * Nx + x)];
                sum += dir ? c.e4cols : c.e1cols;
            }
            maxmsg = std::max(maxmsg, sum);
        }
    }
    for (const SweepCell& c : plan.tab) maxq = std::max<int64_t>(maxq, c.q);
    const int64_t per = maxq + maxmsg;
    TN_CHECK_ARG(per * 8 <= LINE_SCRATCH_BYTES, "cells: the messages of one line exceed the scratch of a group (16 MiB)");
    TN_CHECK_ARG(ws, "ws: null");
    if (ws_bytes < need) {
        set_error("tn_line_sweep: workspace too small (%lld bytes, tn_line_sweep_ws_bytes asks for %lld)", (long long)ws_bytes, (long long)need);
        return -3;
    }
    hipStream_t st = (hipStream_t)stream;
    const LineWs w = line_layout(ws, Nx, Ny, M);
    const unsigned mblk = (unsigned)cdiv(M, 256);
    if (sweeps > 0) {
        BS(sweep_put_cells(st, plan, w.cells));
        if (mode == 0) {
            // the range guard: the one check that needs the tables, and with it the call's one wait for the stream.  Only the ranges
            // (and the table of the cells) have been written when it refuses.
            hipLaunchKernelGGL(line_ranges_kernel, dim3((unsigned)(2 * ncell)), dim3(256), 0, st, w.cells, ncell, w.ranges);
            TN_CHECK_LAUNCH("line_ranges_kernel");
            std::vector<double> host((size_t)(4 * ncell));
            BSH(hipMemcpyAsync(host.data(), w.ranges, host.size() * 8, hipMemcpyDeviceToHost, st), "tn_line_sweep: ranges");
            BSH(hipStreamSynchronize(st), "tn_line_sweep: ranges");
            for (int64_t t = 0; t < 2 * ncell; ++t) {
                if (lines != 2 && lines != (int)(t / ncell)) continue;
                const double range = host[(size_t)(2 * t + 1)] - host[(size_t)(2 * t)];
                if (!(beta * range <= LINE_BETA_RANGE)) {
                    set_error("tn_line_sweep: range guard: beta x (max - min) of the %s table of cell %lld is %g, above %g (linear-domain heat bath)",
                              t / ncell ? "E4" : "E1", (long long)(t % ncell), beta * range, LINE_BETA_RANGE);
                    return -1;
                }
            }
        }
        hipLaunchKernelGGL(line_offsets_kernel, dim3(1), dim3(1), 0, st, w.cells, ncell, lines, line_table_limit(), w.toff);
        TN_CHECK_LAUNCH("line_offsets_kernel");
        hipLaunchKernelGGL(line_tables_kernel, dim3((unsigned)(2 * ncell * LINE_BUILD_BLOCKS)), dim3(256), 0, st, w.cells, ncell, w.ranges, w.toff, mode, beta,
                           w.tables);
        TN_CHECK_LAUNCH("line_tables_kernel");
        const int Wl = maxq <= 8 ? 8 : maxq <= 32 ? 32 : 64, G = 256 / Wl;
        const bool use_lds = G * per * 8 <= LINE_LDS_BYTES;
        const int64_t lds = use_lds ? G * per * 8 : 0;
        const int64_t max_blocks = use_lds ? LINE_MAX_BLOCKS : std::min<int64_t>(LINE_MAX_BLOCKS, std::max<int64_t>(1, LINE_SCRATCH_BYTES / (per * 8) / G));
        LineArgs a;
        a.cells = w.cells; a.states = states; a.chg = w.chg; a.ranges = w.ranges; a.toff = w.toff; a.tables = w.tables; a.scratch = w.scratch;
        a.Nx = Nx; a.Ny = Ny; a.M = M; a.ldu = ldu; a.per = per; a.maxq = maxq; a.ntiles = cdiv(M, G); a.use_lds = use_lds ? 1 : 0; a.beta = beta;
        for (int64_t j = 0; j < sweeps; ++j)
            for (int p = 0; p < P; ++p) {
                a.dir = lines == 2 ? p : lines;
                a.uniforms = mode == 0 ? uniforms + (j * P + p) * ncell * ldu : nullptr;
                const int64_t nl = a.dir ? Nx : Ny;
                for (int parity = 0; parity < 2; ++parity) {
                    const int64_t nlp = (nl + 1 - parity) / 2;
                    if (nlp == 0) continue;
                    a.parity = parity;
                    a.nunits = nlp * a.ntiles;
                    const int64_t nblocks = std::min(a.nunits, max_blocks);
                    if (Wl == 8) BS(launch_lines<8>(st, a, mode, nblocks, lds));
                    else if (Wl == 32) BS(launch_lines<32>(st, a, mode, nblocks, lds));
                    else BS(launch_lines<64>(st, a, mode, nblocks, lds));
                }
                if (moves_out || last_moves_out) {
                    hipLaunchKernelGGL(line_moves_kernel, dim3(mblk), dim3(256), 0, st, w.chg, ncell, M, (j == 0 && p == 0) ? 1 : 0, p == 0 ? 1 : 0, moves_out,
                                       last_moves_out);
                    TN_CHECK_LAUNCH("line_moves_kernel");
                }
            }
    } else {
        BS(sweep_put_cells(st, plan, w.cells));
        if (moves_out) BSH(hipMemsetAsync(moves_out, 0, (size_t)M * 4, st), "tn_line_sweep: clear");
        if (last_moves_out) BSH(hipMemsetAsync(last_moves_out, 0, (size_t)M * 4, st), "tn_line_sweep: clear");
    }
    return sweep_energy(st, plan, w.cells, states, energy_out);
}

}  // extern "C"
