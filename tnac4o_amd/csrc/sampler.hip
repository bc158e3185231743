// The sampling walk -- gibbs_sampling of the reference (tnac4o.py:553-650) in the library: M configurations drawn cell by cell from
// the conditional tables of the boundary-MPS contraction, each with the log-probability it was drawn with.
//
// sample_pn: one workgroup per DISTINCT boundary row of the sample set.  The front half is calc_pn's (pn.h: the table comes out with
// the same bits); the table never leaves LDS: its running sum is formed there and every sample of the row finds its state by binary
// search with its own uniform number.  The running sum is taken in a fixed order that depends on q alone (chunks of 256, in a chunk
// a shuffle scan per wave and the waves' totals added in wave order), so a draw does not depend on which other samples share the
// call.  Draw rule = np.searchsorted(cum, r), side 'left' (tnac4o.py:616-622), with two edge rules: a landing on a zero entry moves
// forward to the next positive one, and r above cum[q-1] (the sum may end an ulp below 1) takes the last positive one.
//
// score_pn: the same workgroup per distinct boundary row and the same table, but every member brings its state instead of a uniform
// number: no running sum, no search; the increment log2 P[s] is -inf where P[s] is not positive or s lies outside [0, q).
//
// tn_gibbs_sample / tn_gibbs_score: the walk over rows and sites on one stream (gibbs_walk), samples keep their slot (no cut, no merge,
// no selection), on the scaffolding it shares with the beam search (walk.h).  The two entries differ in the draw step alone.  Two
// count read-backs per site-step, none of size M.
#include "walk.h"
#include "devprim.h"
#include "pn.h"

namespace tn {

namespace {

// inclusive running sum of sP[0..q) into sC[0..q): chunks of 256 with a running carry; scr: 4 doubles of LDS
__device__ __forceinline__ void table_cumsum(const double* sP, double* sC, int q, double* scr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double carry = 0.0;
    for (int base = 0; base < q; base += 256) {
        const int s = base + tid;
        double v = s < q ? sP[s] : 0.0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double t = __shfl_up(v, o, 64);
            if (lane >= o) v += t;
        }
        if (lane == 63) scr[wave] = v;
        __syncthreads();
        double pre = carry;
        for (int w = 0; w < wave; ++w) pre += scr[w];
        if (s < q) sC[s] = pre + v;
        carry = ((carry + scr[0]) + scr[1]) + scr[2] + scr[3];
        __syncthreads();                                   // scr is rewritten by the next chunk
    }
}

__global__ __launch_bounds__(256) void sample_pn_kernel(const double* __restrict__ T1, const double* __restrict__ RR, const double* __restrict__ F,
                                                        const int32_t* __restrict__ dmap, const int32_t* __restrict__ rmap,
                                                        const int32_t* __restrict__ pref, const int32_t* __restrict__ suf,
                                                        const int32_t* __restrict__ lidx, const int32_t* __restrict__ uidx,
                                                        const int32_t* __restrict__ perm, const int64_t* __restrict__ starts,
                                                        const double* __restrict__ uniforms, int q, int nl, int nu, int p, int Dr, int br, int tab_off,
                                                        int32_t* __restrict__ child, double* __restrict__ log2p, double* __restrict__ minP) {
    extern __shared__ double lds[];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    double* sP = lds + tab_off;         // [q]; the front of the LDS holds T1 / RR / T2 first, the running sum afterwards
    double* sC = lds;                   // [q]
    const double mPn = pn_table(T1 + (int64_t)pref[g] * p * Dr, RR + (int64_t)suf[g] * Dr * br, F, dmap, rmap, lidx[g], uidx[g], q, nl, nu, p, Dr, br, lds,
                                sP, red);
    if (tid == 0) minP[g] = mPn;
    __syncthreads();
    table_cumsum(sP, sC, q, red);
    const int64_t lo = starts[g], hi = starts[g + 1];
    for (int64_t m = lo + tid; m < hi; m += 256) {
        const int32_t k = perm[m];
        const double r = uniforms[k];
        int a = 0, b = q;                                  // first s with cum[s] >= r
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (sC[mid] < r) a = mid + 1; else b = mid;
        }
        int s = a;
        while (s < q && !(sP[s] > 0.0)) ++s;
        if (s >= q) {
            s = q - 1;
            while (s > 0 && !(sP[s] > 0.0)) --s;
        }
        child[k] = s;
        log2p[k] += log2(sP[s]);
    }
}

// the forced twin of sample_pn_kernel: member k of the row takes its state from forced[k * ld + pos].  A state outside [0, q) never
// indexes the table: it scores -inf and walks on as state 0.  log2p[k] += -inf stays -inf under every later finite increment.
__global__ __launch_bounds__(256) void score_pn_kernel(const double* __restrict__ T1, const double* __restrict__ RR, const double* __restrict__ F,
                                                       const int32_t* __restrict__ dmap, const int32_t* __restrict__ rmap,
                                                       const int32_t* __restrict__ pref, const int32_t* __restrict__ suf,
                                                       const int32_t* __restrict__ lidx, const int32_t* __restrict__ uidx,
                                                       const int32_t* __restrict__ perm, const int64_t* __restrict__ starts,
                                                       const int16_t* __restrict__ forced, int64_t ld, int64_t pos, int q, int nl, int nu, int p, int Dr,
                                                       int br, int32_t* __restrict__ child, double* __restrict__ log2p, double* __restrict__ cell_log2p,
                                                       double* __restrict__ minP) {
    extern __shared__ double lds[];
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    double* sP = lds + pn_front_doubles(p, Dr, br);    // [q]
    const double mPn = pn_table(T1 + (int64_t)pref[g] * p * Dr, RR + (int64_t)suf[g] * Dr * br, F, dmap, rmap, lidx[g], uidx[g], q, nl, nu, p, Dr, br, lds,
                                sP, red);
    if (tid == 0) minP[g] = mPn;
    __syncthreads();
    const int64_t lo = starts[g], hi = starts[g + 1];
    for (int64_t m = lo + tid; m < hi; m += 256) {
        const int32_t k = perm[m];
        int s = forced[k * ld + pos];
        const bool inside = s >= 0 && s < q;
        if (!inside) s = 0;
        const double v = sP[s];
        const double inc = (inside && v > 0.0) ? log2(v) : -std::numeric_limits<double>::infinity();
        child[k] = s;
        log2p[k] += inc;
        if (cell_log2p) cell_log2p[k * ld + pos] = inc;
    }
}

// row keys of the samples (prefix rank, left index, up index, suffix rank): equal keys = equal boundary rows at this site
__global__ __launch_bounds__(256) void row_key_kernel(const int32_t* pref, const int32_t* lcol, const int32_t* ucol, const int32_t* suf, int64_t B,
                                                     int64_t nsuf, int64_t n, int64_t* key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) key[i] = (((int64_t)pref[i] * B + lcol[i]) * B + ucol[i]) * nsuf + suf[i];
}
__global__ __launch_bounds__(256) void group_gather_kernel(const int32_t* first, const int32_t* pref, const int32_t* lcol, const int32_t* ucol,
                                                          const int32_t* suf, int64_t ng, int32_t* gpref, int32_t* gl, int32_t* gu, int32_t* gsuf) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= ng) return;
    const int32_t f = first[g];
    gpref[g] = pref[f];
    gl[g] = lcol[f];
    gu[g] = ucol[f];
    gsuf[g] = suf[f];
}
// the drawn state of every sample becomes part of its configuration: what expand_kernel and commit_kernel of the beam search do for
// a kept candidate, for the one child of every sample (tnac4o.py:623-627, 1506-1558)
__global__ __launch_bounds__(256) void advance_kernel(const int32_t* child, int64_t n, CellDev c, int16_t* states, int64_t nsites, int64_t pos, int64_t Nx,
                                                     int has_left, int has_up, double* Eng, const int32_t* pref, int64_t B, int32_t* down_col,
                                                     int32_t* right_col, int64_t* pkey) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t ch = child[i];
    const int64_t dn = c.down[ch], rt = c.right[ch];
    const double dE = cell_energy(c, ch, states + i * nsites, pos, Nx, has_left, has_up);
    states[i * nsites + pos] = (int16_t)ch;
    down_col[i] = (int32_t)dn;
    right_col[i] = (int32_t)rt;
    Eng[i] = Eng[i] + dE;
    pkey[i] = (int64_t)pref[i] * B + dn;
}

inline int64_t sample_tab_off(int64_t q, int64_t p, int64_t Dr, int64_t br) { return std::max(pn_front_doubles(p, Dr, br), q); }
inline int64_t sampler_cub_bytes(int64_t M) { return M * 32 + ((int64_t)1 << 20); }
inline bool mul_fits(int64_t a, int64_t b, int64_t& out) { return !__builtin_mul_overflow(a, b, &out); }

}  // namespace

int sample_pn(hipStream_t st, const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap, const int32_t* pref,
              const int32_t* suf, const int32_t* lidx, const int32_t* uidx, const int32_t* perm, const int64_t* starts, int64_t ng,
              const double* uniforms, int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr, int64_t br, int32_t* child, double* log2p, double* minP) {
    if (ng <= 0) return 0;
    TN_CHECK_ARG(q >= 1 && nl >= 1 && nu >= 1 && p >= 1 && Dr >= 1 && br >= 1, "non-positive dimension");
    TN_CHECK_ARG(ng < ((int64_t)1 << 31), "too many groups");
    const int64_t off = sample_tab_off(q, p, Dr, br), lds = (off + q) * 8;      // (calc_pn's own bound, (front + q) * 8, is never the larger)
    TN_CHECK_ARG(lds <= 150 * 1024, "site too large for sample_pn (the table, its running sum and the environments must fit 150 KiB of LDS)");
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)sample_pn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(sample_pn_kernel, dim3((unsigned)ng), dim3(256), (size_t)lds, st, T1, RR, F, dmap, rmap, pref, suf, lidx,
                       uidx, perm, starts, uniforms, (int)q, (int)nl, (int)nu, (int)p, (int)Dr, (int)br, (int)off, child, log2p, minP));
    TN_CHECK_LAUNCH("sample_pn_kernel");
    return 0;
}

int score_pn(hipStream_t st, const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap, const int32_t* pref,
             const int32_t* suf, const int32_t* lidx, const int32_t* uidx, const int32_t* perm, const int64_t* starts, int64_t ng,
             const int16_t* forced, int64_t ld, int64_t pos, int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr, int64_t br, int32_t* child,
             double* log2p, double* cell_log2p, double* minP) {
    if (ng <= 0) return 0;
    TN_CHECK_ARG(q >= 1 && nl >= 1 && nu >= 1 && p >= 1 && Dr >= 1 && br >= 1, "non-positive dimension");
    TN_CHECK_ARG(ng < ((int64_t)1 << 31), "too many groups");
    TN_CHECK_ARG(pos >= 0 && pos < ld, "forced states: column outside the row");
    const int64_t lds = (pn_front_doubles(p, Dr, br) + q) * 8;                  // calc_pn's bound: no running sum is kept
    TN_CHECK_ARG(lds <= 150 * 1024, "site too large for score_pn (the table and the environments must fit 150 KiB of LDS)");
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)score_pn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    TN_PROF_LAUNCH(st, PROF_MISC, hipLaunchKernelGGL(score_pn_kernel, dim3((unsigned)ng), dim3(256), (size_t)lds, st, T1, RR, F, dmap, rmap, pref, suf, lidx,
                       uidx, perm, starts, forced, ld, pos, (int)q, (int)nl, (int)nu, (int)p, (int)Dr, (int)br, child, log2p, cell_log2p, minP));
    TN_CHECK_LAUNCH("score_pn_kernel");
    return 0;
}

namespace {

int64_t gibbs_walk_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t max_env, int64_t max_t1, int64_t max_w) {
    const int64_t cap = M, nsites = Nx * Ny;
    int64_t b = 0;
    auto add = [&](int64_t bytes) { b = align_up(b, 256) + bytes; };
    add((Nx + 1) * cap * 4); add((Nx + 1) * cap * 4); add(Nx * cap * 4); add(cap * 4); add(cap * 4);      // index rows (+ shifted copy), suffix and prefix ranks
    add(cap * nsites * 2); add(cap * 8); add(cap * 8);                                                    // states, energies, log2 q
    add(cap * 4); add(64);                           // iota, scalars
    add(sampler_cub_bytes(M));                       // rocPRIM temporary storage (checked against its queries at run time)
    // a row: right environments and MPO site of every level, the levels' index scratch, two generations of left environments
    add(256);
    for (int64_t l = 0; l < Nx; ++l) { add(cap * max_env * 8); add(max_w * 8); add(cap * 64 + 4096); }
    add(cap * max_env * 8); add(cap * max_env * 8);
    // a site-step
    add(cap * max_t1 * 8);                           // T1
    add(cap * 8); add(cap * 4); add(cap * 4); add((cap + 1) * 8);      // row keys, first members, members by group, group offsets
    for (int i = 0; i < 4; ++i) add(cap * 4);        // per group: prefix, left, up, suffix
    add(cap * 4); add(cap * 8); add(cap * 8);        // drawn states, table flags, prefix keys
    add(cap * 4);                                    // first members of the prefixes
    add(cap * 8); add(cap * 4 * 3);                  // unique: sorted keys, order, heads, group ids
    add(cap * 4); add(cap * 4);                      // prefix parents, down indices
    return b + 4096;
}

#define WK_ARG(cond, msg)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            set_error("%s: %s", who, msg);                 \
            return -1;                                     \
        }                                                  \
    } while (0)

// The walk of both entries (`who`: the entry, for the error text).  score = false: tn_gibbs_sample, the draw step is sample_pn with
// `uniforms` and the configurations go to states_out.  score = true: tn_gibbs_score, the draw step is score_pn along `forced`
// (M x Nx*Ny) and cell_log2p_out (may be NULL) takes the increments.  Everything else -- right_levels, the row keys and unique,
// advance_kernel, env_rl_batched, the workspace layout -- is the same code.
int gibbs_walk(const char* who, bool score, int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t B, const double* uniforms,
               int64_t ldu, const int16_t* forced, int16_t* states_out, double* energy_out, double* log2p_out, double* cell_log2p_out,
               double* globalmin_host, int64_t* max_groups_host, void* ws, int64_t ws_bytes, void* stream) {
    WK_ARG(Nx >= 1 && Ny >= 1 && M >= 1 && B >= 1 && cells && ws, "bad arguments");
    WK_ARG(M < ((int64_t)1 << 31), "too many samples in one call");
    if (score) {
        WK_ARG(forced, "states: null");
    } else {
        WK_ARG(uniforms && ldu >= M, "uniforms: null, or rows shorter than M");
    }
    WK_ARG((score || states_out) && energy_out && log2p_out && globalmin_host, "null result pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nsites = Nx * Ny, cap = M, ncol = Nx + 1;
    int64_t qmax = 1, max_env = 1, max_t1 = 1, max_w = 1;
    WALK_CHECK_CELLS(cells, nsites, qmax, max_env, max_t1, max_w)
    for (int64_t i = 0; i < nsites; ++i) {
        const tn_beam_cell& c = cells[i];
        if (score) {
            WK_ARG((pn_front_doubles(c.p, c.Dr, c.br) + c.q) * 8 <= 150 * 1024, "a cell's table and environments exceed 150 KiB of LDS (tn_score_pn)");
        } else {
            WK_ARG((sample_tab_off(c.q, c.p, c.Dr, c.br) + c.q) * 8 <= 150 * 1024, "a cell's table, its running sum and environments exceed 150 KiB of LDS (tn_sample_pn)");
        }
    }
    {   // the radix product of the row keys (prefix rank, left, up, suffix rank) must fit int64 in the worst case of M distinct prefixes and suffixes
        int64_t r = 0;
        WK_ARG(mul_fits(M, B, r) && mul_fits(r, B, r) && mul_fits(r, M, r), "M x B x B x M exceeds int64 (row keys): use fewer samples per call");
    }
    if (ws_bytes < gibbs_walk_ws_bytes(Nx, Ny, M, max_env, max_t1, max_w)) {
        set_error("%s: workspace too small (%lld bytes, %s_ws_bytes asks for %lld)", who, (long long)ws_bytes, who,
                  (long long)gibbs_walk_ws_bytes(Nx, Ny, M, max_env, max_t1, max_w));
        return -3;
    }
    Bump bump;
    bump.base = (char*)ws; bump.cap = ws_bytes; bump.who = who;
    TAKE(vind, int32_t, bump, ncol * cap, "index rows");
    TAKE(vind2, int32_t, bump, ncol * cap, "index rows");
    TAKE(sufmat, int32_t, bump, Nx * cap, "suffix ranks");
    TAKE(pref, int32_t, bump, cap, "prefix ranks");
    TAKE(pref2, int32_t, bump, cap, "prefix ranks");
    TAKE(states, int16_t, bump, cap * nsites, "states");
    TAKE(Eng, double, bump, cap, "energies");
    TAKE(lq, double, bump, cap, "log2 q");
    Walk S;
    S.st = st;
    S.iota = bump.take<int32_t>(cap);
    double* scal = bump.take<double>(8);             // device scalars: [0] globalmin, [1] min of minP
    S.cub_bytes = (size_t)sampler_cub_bytes(M);
    S.cub_tmp = bump.take<char>((int64_t)S.cub_bytes);
    if (!S.iota || !scal || !S.cub_tmp) { set_error("%s: workspace too small (sort storage)", who); return -3; }
    {   // the temporary storage rocPRIM asks for at the largest sizes must fit the slot
        size_t need = 0, t = 0;
        (void)rocprim::radix_sort_pairs(nullptr, t, (const int64_t*)nullptr, (int64_t*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr, (int)M, 0, 64, st);
        need = std::max(need, t);
        (void)rocprim::inclusive_scan(nullptr, t, (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)M, rocprim::plus<int32_t>(), st);
        need = std::max(need, t);
        (void)rocprim::reduce(nullptr, t, (const double*)nullptr, (double*)nullptr, std::numeric_limits<double>::max(), (size_t)M, rocprim::minimum<double>(), st);
        need = std::max(need, t);
        WK_ARG(need <= S.cub_bytes, "rocPRIM temporary storage exceeds its slot");
    }
    hipLaunchKernelGGL(iota_kernel, dim3((unsigned)cdiv(cap, 256)), dim3(256), 0, st, S.iota, cap);
    TN_CHECK_LAUNCH("iota_kernel");
    {   // every sample starts at the open boundary with energy 0 and log2 q = 0; globalmin = 1 (tnac4o.py:584-590)
        const double h[8] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        BS(upload(st, scal, h, 64, PIN_SHARED, "sampling walk: scalars"));
        BSH(hipMemsetAsync(vind, 0, (size_t)ncol * cap * 4, st), "sampling walk: clear");
        BSH(hipMemsetAsync(states, 0, (size_t)cap * nsites * 2, st), "sampling walk: clear");
        BSH(hipMemsetAsync(Eng, 0, (size_t)cap * 8, st), "sampling walk: clear");
        BSH(hipMemsetAsync(lq, 0, (size_t)cap * 8, st), "sampling walk: clear");
    }
    int64_t max_groups = 1;
    const unsigned mblk = (unsigned)cdiv(M, 256);
    const int64_t row_mark = bump.off;
    for (int64_t ny = 0; ny < Ny; ++ny) {
        bump.off = row_mark;
        const tn_beam_cell* row = cells + ny * Nx;
        std::vector<double*> RRs;
        std::vector<int64_t> nsuf;
        BS(S.right_levels(bump, row, Nx, vind, sufmat, cap, M, RRs, nsuf));
        hipLaunchKernelGGL(fill_i32_kernel, dim3(mblk), dim3(256), 0, st, pref, M, 0);
        TN_CHECK_LAUNCH("fill_i32_kernel");
        TAKE(RLa, double, bump, cap * max_env, "left environments");
        TAKE(RLb, double, bump, cap * max_env, "left environments");
        double* RL = RLa;
        double* RLn = RLb;
        hipLaunchKernelGGL(ones_kernel, dim3(1), dim3(256), 0, st, RL, (int64_t)1);
        TN_CHECK_LAUNCH("ones_kernel");
        int64_t npref = 1;
        const int64_t step_mark = bump.off;
        for (int64_t nx = 0; nx < Nx; ++nx) {
            bump.off = step_mark;
            const tn_beam_cell& c = row[nx];
            const int64_t pos = ny * Nx + nx, lvl = Nx - nx - 1;
            int32_t* lcol = vind + nx * cap;
            int32_t* ucol = vind + (nx + 1) * cap;
            const int32_t* suf = sufmat + lvl * cap;
            // T1[prefix] = RL[prefix] . A   (tnac4o.py:596-599); never split over K: a row of T1 must not depend on how many prefixes there are
            TAKE(T1, double, bump, npref * c.p * c.Dr, "T1");
            BS(gemm(st, npref, c.p * c.Dr, c.Dl, 1.0, RL, c.Dl, 1, c.A, c.p * c.Dr, 1, 0.0, T1, c.p * c.Dr, 1, 1, 0, 0, 0, nullptr, 0));
            // ---- the distinct boundary rows of the samples (the reference's `seen` dictionary, tnac4o.py:601-612)
            TAKE(key, int64_t, bump, M, "row keys");
            TAKE(first, int32_t, bump, M, "first members");
            TAKE(perm, int32_t, bump, M, "group order");
            TAKE(starts, int64_t, bump, M + 1, "group offsets");
            hipLaunchKernelGGL(row_key_kernel, dim3(mblk), dim3(256), 0, st, pref, lcol, ucol, suf, B, nsuf[(size_t)lvl], M, key);
            TN_CHECK_LAUNCH("row_key_kernel");
            int64_t ng = 0;
            BS(S.unique(bump, key, M, ng, nullptr, first, perm, starts));
            max_groups = std::max(max_groups, ng);
            TAKE(gpref, int32_t, bump, ng, "group prefixes");
            TAKE(gl, int32_t, bump, ng, "group left indices");
            TAKE(gu, int32_t, bump, ng, "group up indices");
            TAKE(gsuf, int32_t, bump, ng, "group suffixes");
            hipLaunchKernelGGL(group_gather_kernel, dim3((unsigned)cdiv(ng, 256)), dim3(256), 0, st, first, pref, lcol, ucol, suf, ng, gpref, gl, gu, gsuf);
            TN_CHECK_LAUNCH("group_gather_kernel");
            // ---- the draw (tnac4o.py:614-622), or the caller's state in its place
            TAKE(child, int32_t, bump, M, "drawn states");
            TAKE(mP, double, bump, ng, "table flags");
            if (score) {
                BS(score_pn(st, T1, RRs[(size_t)lvl], c.F, c.dmap, c.rmap, gpref, gsuf, gl, gu, perm, starts, ng, forced, nsites, pos, c.q, c.nl, c.nu,
                            c.p, c.Dr, c.br, child, lq, cell_log2p_out, mP));
            } else {
                BS(sample_pn(st, T1, RRs[(size_t)lvl], c.F, c.dmap, c.rmap, gpref, gsuf, gl, gu, perm, starts, ng, uniforms + pos * ldu, c.q, c.nl, c.nu, c.p,
                             c.Dr, c.br, child, lq, mP));
            }
            size_t tb = S.cub_bytes;
            BSH(rocprim::reduce(S.cub_tmp, tb, mP, scal + 1, std::numeric_limits<double>::max(), (size_t)ng, rocprim::minimum<double>(), st), "sampling walk: minimum");
            hipLaunchKernelGGL(scalar_min_kernel, dim3(1), dim3(1), 0, st, scal, 0, scal + 1);
            TN_CHECK_LAUNCH("scalar_min_kernel");
            // ---- states, boundary indices, energies, prefix keys (tnac4o.py:623-627)
            TAKE(pkey, int64_t, bump, M, "prefix keys");
            hipLaunchKernelGGL(advance_kernel, dim3(mblk), dim3(256), 0, st, child, M, cell_dev(c), states, nsites, pos, Nx, nx > 0 ? 1 : 0, ny > 0 ? 1 : 0, Eng,
                               pref, B, lcol, ucol, pkey);
            TN_CHECK_LAUNCH("advance_kernel");
            // ---- left environments of the new distinct prefixes: rows of T1 (tnac4o.py:628-636)
            TAKE(nfirst, int32_t, bump, M, "first members of the prefixes");
            int64_t np2 = 0;
            BS(S.unique(bump, pkey, M, np2, pref2, nfirst, nullptr, nullptr));
            TAKE(par, int32_t, bump, np2, "prefix parents");
            TAKE(didx, int32_t, bump, np2, "prefix down indices");
            hipLaunchKernelGGL(prefix_gather_kernel, dim3((unsigned)cdiv(np2, 256)), dim3(256), 0, st, nfirst, pref, lcol, np2, par, didx);
            TN_CHECK_LAUNCH("prefix_gather_kernel");
            BS(env_rl_batched(st, T1, par, didx, np2, c.p, c.Dr, RLn));
            std::swap(RL, RLn);
            std::swap(pref, pref2);
            npref = np2;
        }
        hipLaunchKernelGGL(shift_columns_kernel, dim3((unsigned)cdiv(M * ncol, 256)), dim3(256), 0, st, vind, vind2, cap, ncol, M);      // tnac4o.py:638-639
        TN_CHECK_LAUNCH("shift_columns_kernel");
        std::swap(vind, vind2);
    }
    if (states_out) BSH(hipMemcpyAsync(states_out, states, (size_t)M * nsites * 2, hipMemcpyDeviceToDevice, st), "sampling walk: results");
    BSH(hipMemcpyAsync(energy_out, Eng, (size_t)M * 8, hipMemcpyDeviceToDevice, st), "sampling walk: results");
    BSH(hipMemcpyAsync(log2p_out, lq, (size_t)M * 8, hipMemcpyDeviceToDevice, st), "sampling walk: results");
    double hs = 0.0;
    BS(read_back(st, &hs, scal, 8, PIN_SHARED, "sampling walk: scalars"));
    *globalmin_host = hs;
    if (max_groups_host) *max_groups_host = max_groups;
    return 0;
}

}  // namespace

}  // namespace tn

using namespace tn;

extern "C" {

int tn_sample_pn(const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap, const int32_t* pref,
                 const int32_t* suf, const int32_t* lidx, const int32_t* uidx, const int32_t* perm, const int64_t* starts, int64_t ng,
                 const double* uniforms, int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr, int64_t br, int32_t* child_out,
                 double* log2p_inout, double* minP_out, void* stream) {
    TN_CHECK_ARG(ng >= 0, "negative group count");
    TN_CHECK_ARG(T1 && RR && F && dmap && rmap && pref && suf && lidx && uidx && perm && starts && uniforms && child_out && log2p_inout && minP_out,
                 "null operand");
    return sample_pn((hipStream_t)stream, T1, RR, F, dmap, rmap, pref, suf, lidx, uidx, perm, starts, ng, uniforms, q, nl, nu, p, Dr, br, child_out,
                     log2p_inout, minP_out);
}

int tn_score_pn(const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap, const int32_t* pref,
                const int32_t* suf, const int32_t* lidx, const int32_t* uidx, const int32_t* perm, const int64_t* starts, int64_t ng,
                const int16_t* forced, int64_t ld, int64_t pos, int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr, int64_t br, int32_t* child_out,
                double* log2p_inout, double* cell_log2p, double* minP_out, void* stream) {
    TN_CHECK_ARG(ng >= 0, "negative group count");
    TN_CHECK_ARG(T1 && RR && F && dmap && rmap && pref && suf && lidx && uidx && perm && starts && forced && child_out && log2p_inout && minP_out,
                 "null operand");
    return score_pn((hipStream_t)stream, T1, RR, F, dmap, rmap, pref, suf, lidx, uidx, perm, starts, ng, forced, ld, pos, q, nl, nu, p, Dr, br, child_out,
                    log2p_inout, cell_log2p, minP_out);
}

int64_t tn_gibbs_sample_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t qmax, int64_t max_env, int64_t max_t1, int64_t max_w) {
    (void)qmax;                                      // no table is ever materialised: nothing here grows with q
    return gibbs_walk_ws_bytes(Nx, Ny, M, max_env, max_t1, max_w);
}

int tn_gibbs_sample(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t B, const double* uniforms, int64_t ldu, int16_t* states_out,
                    double* energy_out, double* log2p_out, double* globalmin_host, int64_t* max_groups_host, void* ws, int64_t ws_bytes, void* stream) {
    return gibbs_walk("tn_gibbs_sample", false, Nx, Ny, cells, M, B, uniforms, ldu, nullptr, states_out, energy_out, log2p_out, nullptr, globalmin_host,
                      max_groups_host, ws, ws_bytes, stream);
}

int64_t tn_gibbs_score_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t qmax, int64_t max_env, int64_t max_t1, int64_t max_w) {
    (void)qmax;                                      // the walk's own workspace: the forced states and the increments are the caller's
    return gibbs_walk_ws_bytes(Nx, Ny, M, max_env, max_t1, max_w);
}

int tn_gibbs_score(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t B, const int16_t* states, double* energy_out, double* log2p_out,
                   double* cell_log2p_out, double* globalmin_host, int64_t* max_groups_host, void* ws, int64_t ws_bytes, void* stream) {
    return gibbs_walk("tn_gibbs_score", true, Nx, Ny, cells, M, B, nullptr, 0, states, nullptr, energy_out, log2p_out, cell_log2p_out, globalmin_host,
                      max_groups_host, ws, ws_bytes, stream);
}

}  // extern "C"

