// Scaffolding of the walks over the rows and sites of the lattice that run in the library: the beam search (beamsearch.hip) and the
// sampling walk (sampler.hip).  Both keep their index rows column-major (a column of boundary indices is contiguous), rank the
// boundary prefixes and suffixes through sorted int64 keys, and build the right environments of a row level by level.  Sorting is
// rocPRIM's radix sort (stable; called directly, no CUDA-compat layer); "unique" = sort, head flags, prefix sum.  Internal header:
// everything here has internal linkage, each of the two translation units gets its own copy of the small kernels.
#pragma once
#include <string.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/tnpeps.h"
#include "common.h"

namespace tn {

namespace {

#define BS(call)                   \
    do {                           \
        const int rc__ = (call);   \
        if (rc__) return rc__;     \
    } while (0)
#define BSH(call, what)                                   \
    do {                                                  \
        const hipError_t e__ = (call);                    \
        if (e__ != hipSuccess) return hip_fail(e__, what); \
    } while (0)

// ---- small kernels -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void iota_kernel(int32_t* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
}
__global__ __launch_bounds__(256) void fill_i32_kernel(int32_t* out, int64_t n, int32_t v) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = v;
}
// key of the suffix vind[:, c:] = (vind[:, c], rank of vind[:, c+1:])
__global__ __launch_bounds__(256) void suffix_key_kernel(const int32_t* col, const int32_t* suf_prev, int64_t nkeys_prev, int64_t n, int64_t* key) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) key[i] = (int64_t)col[i] * nkeys_prev + suf_prev[i];
}
__global__ __launch_bounds__(256) void heads_kernel(const int64_t* skey, int64_t n, int32_t* head) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) head[i] = (i == 0 || skey[i] != skey[i - 1]) ? 1 : 0;
}
// after the prefix sum of the head flags: inverse (group of every element), first member of every group (stable sort: the head
// of a group is its smallest original index), offsets of the groups in the sorted order (starts[ng] = n)
__global__ __launch_bounds__(256) void unique_scatter_kernel(const int32_t* sidx, const int32_t* head, const int32_t* gid, int64_t n, int32_t* inv,
                                                            int32_t* first, int64_t* starts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int32_t g = gid[i] - 1;
    if (inv) inv[sidx[i]] = g;
    if (head[i]) {
        if (first) first[g] = sidx[i];
        if (starts) starts[g] = i;
    }
    if (i == n - 1 && starts) starts[g + 1] = n;
}
__global__ __launch_bounds__(256) void level_gather_kernel(const int32_t* first, const int32_t* suf_prev, const int32_t* col, int64_t nk, int32_t* parent,
                                                          int32_t* uidx) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nk) return;
    const int32_t f = first[k];
    parent[k] = suf_prev[f];
    uidx[k] = col[f];
}
__global__ __launch_bounds__(256) void ones_kernel(double* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 1.0;
}
// scal[dst] = min (scal[dst], *src)
__global__ void scalar_min_kernel(double* scal, int dst, const double* src) { scal[dst] = fmin(scal[dst], *src); }

struct CellDev {                       // what the step from a cell's state to the next boundary needs of the cell (device pointers)
    const int64_t* down;
    const int64_t* right;
    const double* Es;
    const double* E1;
    const double* E4;
    const int64_t* left_map;
    const int64_t* up_map;
    int64_t q, e1cols, e4cols;
};
inline CellDev cell_dev(const tn_beam_cell& c) {
    CellDev cd;
    cd.down = c.down; cd.right = c.right; cd.Es = c.Es; cd.E1 = c.E1; cd.E4 = c.E4; cd.left_map = c.left_map; cd.up_map = c.up_map;
    cd.q = c.q; cd.e1cols = c.e1cols; cd.e4cols = c.e4cols;
    return cd;
}
// energy a cell in state ch adds to a configuration whose earlier cells are in `states` (tnac4o.py:1506-1558), in the order the
// reference adds it up
__device__ __forceinline__ double cell_energy(const CellDev& c, int64_t ch, const int16_t* states, int64_t pos, int64_t Nx, int has_left, int has_up) {
    double dE = 1.0 * c.Es[ch];
    if (has_left) {
        const int64_t left = states[pos - 1];
        dE = dE + c.E1[ch * c.e1cols + (c.left_map ? c.left_map[left] : left)];
    }
    if (has_up) {
        const int64_t up = states[pos - Nx];
        dE = dE + c.E4[ch * c.e4cols + (c.up_map ? c.up_map[up] : up)];
    }
    return dE;
}
__global__ __launch_bounds__(256) void prefix_gather_kernel(const int32_t* nfirst, const int32_t* prefc, const int32_t* col, int64_t npref, int32_t* par,
                                                           int32_t* didx) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= npref) return;
    const int32_t f = nfirst[g];
    par[g] = prefc[f];
    didx[g] = col[f];
}
// end of a row (tnac4o.py:540-542): the down indices of the row become the up indices of the next, column 0 is the open left edge
__global__ __launch_bounds__(256) void shift_columns_kernel(const int32_t* vind, int32_t* vind_n, int64_t cap, int64_t ncol, int64_t nb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nb * ncol) return;
    const int64_t c = i / nb, b = i % nb;
    vind_n[c * cap + b] = (c == 0) ? 0 : vind[(c - 1) * cap + b];
}

struct Bump {
    char* base = nullptr;
    int64_t cap = 0, off = 0;
    const char* who = "walk";           // the entry point, for the error text
    template <typename T>
    T* take(int64_t count) {
        const int64_t o = align_up(off, 256), bytes = count * (int64_t)sizeof(T);
        if (o + bytes > cap) return nullptr;
        off = o + bytes;
        return (T*)(base + o);
    }
};
#define TAKE(ptr, T, bump, count, what)                                                     \
    T* ptr = (bump).take<T>(count);                                                         \
    if (!ptr) { set_error("%s: workspace too small (%s)", (bump).who, what); return -3; }

struct Walk {
    hipStream_t st;
    void* cub_tmp = nullptr;
    size_t cub_bytes = 0;
    int32_t* iota = nullptr;            // 0 .. (largest number of keys) - 1

    int read_i32(const int32_t* dev, int32_t& v) { return read_back(st, &v, dev, 4, PIN_SHARED, "walk: read-back"); }
    // sorted unique of n int64 keys: number of groups (host), inverse, first members, sorted order, group offsets (any may be NULL)
    int unique(Bump scratch, const int64_t* key, int64_t n, int64_t& ng, int32_t* inv, int32_t* first, int32_t* sidx_out, int64_t* starts) {
        TAKE(skey, int64_t, scratch, n, "sorted keys");
        int32_t* sidx = sidx_out;
        if (!sidx) { sidx = scratch.take<int32_t>(n); if (!sidx) { set_error("%s: workspace too small (sort order)", scratch.who); return -3; } }
        TAKE(head, int32_t, scratch, n, "head flags");
        TAKE(gid, int32_t, scratch, n, "group ids");
        size_t tb = cub_bytes;
        BSH(rocprim::radix_sort_pairs(cub_tmp, tb, key, skey, iota, sidx, (int)n, 0, 64, st), "walk: sort keys");
        const unsigned nblk = (unsigned)cdiv(n, 256);
        hipLaunchKernelGGL(heads_kernel, dim3(nblk), dim3(256), 0, st, skey, n, head);
        TN_CHECK_LAUNCH("heads_kernel");
        tb = cub_bytes;
        BSH(rocprim::inclusive_scan(cub_tmp, tb, head, gid, (size_t)n, rocprim::plus<int32_t>(), st), "walk: scan");
        hipLaunchKernelGGL(unique_scatter_kernel, dim3(nblk), dim3(256), 0, st, sidx, head, gid, n, inv, first, starts);
        TN_CHECK_LAUNCH("unique_scatter_kernel");
        int32_t g = 0;
        BS(read_i32(gid + (n - 1), g));
        ng = g;
        return 0;
    }

    // Right environments of every distinct suffix of the nb index rows `vind` (Nx + 1 columns of `cap`) for the row of cells `row`
    // (tnac4o._setup_RR, tnac4o.py:1768-1784): level j serves site Nx-1-j.  sufmat (Nx x cap) receives the suffix rank of every
    // index row at every level, RRs[j] the level's environments and nsuf[j] their number; they are taken from `bump` and live as
    // long as the caller keeps its mark.
    int right_levels(Bump& bump, const tn_beam_cell* row, int64_t Nx, const int32_t* vind, int32_t* sufmat, int64_t cap, int64_t nb,
                     std::vector<double*>& RRs, std::vector<int64_t>& nsuf) {
        RRs.assign((size_t)Nx, nullptr);
        nsuf.assign((size_t)Nx, 1);
        TAKE(rr0, double, bump, 1, "right edge");
        hipLaunchKernelGGL(ones_kernel, dim3(1), dim3(256), 0, st, rr0, (int64_t)1);
        TN_CHECK_LAUNCH("ones_kernel");
        RRs[0] = rr0;
        hipLaunchKernelGGL(fill_i32_kernel, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, st, sufmat, nb, 0);
        TN_CHECK_LAUNCH("fill_i32_kernel");
        int64_t nkeys_prev = 1;
        for (int64_t nx = Nx - 1; nx >= 1; --nx) {
            const int64_t lvl = Nx - nx;
            const tn_beam_cell& c = row[nx];
            const int32_t* col = vind + (nx + 1) * cap;
            const int32_t* suf_prev = sufmat + (lvl - 1) * cap;
            int32_t* suf_new = sufmat + lvl * cap;
            Bump scratch = bump;                                   // released at the end of the level (a copy: the row keeps bump)
            TAKE(key, int64_t, scratch, nb, "suffix keys");
            TAKE(first, int32_t, scratch, nb, "first members");
            hipLaunchKernelGGL(suffix_key_kernel, dim3((unsigned)cdiv(nb, 256)), dim3(256), 0, st, col, suf_prev, nkeys_prev, nb, key);
            TN_CHECK_LAUNCH("suffix_key_kernel");
            int64_t nk = 0;
            BS(unique(scratch, key, nb, nk, suf_new, first, nullptr, nullptr));
            TAKE(parent, int32_t, scratch, nk, "level parents");
            TAKE(uidx, int32_t, scratch, nk, "level up indices");
            hipLaunchKernelGGL(level_gather_kernel, dim3((unsigned)cdiv(nk, 256)), dim3(256), 0, st, first, suf_prev, col, nk, parent, uidx);
            TN_CHECK_LAUNCH("level_gather_kernel");
            // the level's results live until the end of the row: take them from the row's allocator, past the scratch in use
            bump.off = scratch.off;
            TAKE(W, double, bump, c.nl * c.pd * c.br * c.nu, "MPO site");
            TAKE(RR, double, bump, nk * c.Dl * c.nl, "right environments");
            BS(mpo_from_factor(st, c.F, c.dmap, c.rmap, c.q, c.nl, c.nu, c.pd, c.br, W));
            BS(env_rr_batched(st, c.A, RRs[(size_t)lvl - 1], W, parent, uidx, nk, c.Dl, c.p, c.Dr, c.nl, c.br, c.nu, RR));
            RRs[(size_t)lvl] = RR;
            nsuf[(size_t)lvl] = nk;
            nkeys_prev = nk;
        }
        return 0;
    }
};

// what both walks ask of every cell, and the sizes their workspace queries take
#define WALK_CHECK_CELLS(cells, nsites, qmax, max_env, max_t1, max_w)                                                                             \
    for (int64_t i__ = 0; i__ < (nsites); ++i__) {                                                                                                \
        const tn_beam_cell& c = (cells)[i__];                                                                                                     \
        TN_CHECK_ARG(c.q >= 1 && c.q <= 32767 && c.nl >= 1 && c.nu >= 1 && c.pd >= 1 && c.br >= 1 && c.Dl >= 1 && c.p >= 1 && c.Dr >= 1, "bad cell"); \
        TN_CHECK_ARG(c.p == c.pd, "boundary MPS and PEPS cell disagree on the vertical bond");                                                    \
        TN_CHECK_ARG(c.Dl * c.nl <= 2048, "Dl x (left PEPS bond) exceeds 2048 (tn_env_rr): use the Python path");                               \
        qmax = std::max(qmax, c.q);                                                                                                               \
        max_env = std::max(max_env, std::max(c.Dl * c.nl, c.Dr * c.br));                                                                          \
        max_t1 = std::max(max_t1, c.p * c.Dr);                                                                                                    \
        max_w = std::max(max_w, c.nl * c.pd * c.br * c.nu);                                                                                       \
    }

}  // namespace

}  // namespace tn
