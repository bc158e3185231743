// Shared helpers for libtnpeps (gfx950 only).  Internal header — the public C-ABI is include/tnpeps.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace tn {

// thread-local error text, retrievable through tn_last_error()
void set_error(const char* fmt, ...);
const char* get_error();

inline int hip_fail(hipError_t e, const char* what) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return (int)e > 0 ? (int)e : 1;
}

#define TN_CHECK_ARG(cond, msg)                \
    do {                                       \
        if (!(cond)) {                         \
            tn::set_error("%s: %s", __func__, msg); \
            return -1;                         \
        }                                      \
    } while (0)

#define TN_CHECK_LAUNCH(what)                          \
    do {                                               \
        hipError_t e__ = hipGetLastError();            \
        if (e__ != hipSuccess) return tn::hip_fail(e__, what); \
    } while (0)

// ---- environment switches: one reader per kind.  Whether a switch is read once (`static const` at the
// call site) or on every call (the tests switch it) is the caller's decision; these only parse.
inline const char* env_str(const char* name) { return getenv(name); }                                             // raw text, NULL when unset
inline bool env_flag_on(const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); }           // on unless it starts with '0'
inline bool env_flag_set(const char* name) { const char* e = getenv(name); return e && e[0] == '1'; }             // off unless it starts with '1'
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline int64_t env_i64(const char* name, int64_t dflt) { const char* e = getenv(name); return e ? (int64_t)atoll(e) : dflt; }
inline double env_double(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }

// ---- page-locked staging of the small host copies around host decisions (misc.hip) ------------------------------------
// Thread-local page-locked host buffers, one per slot (grown on demand, released when the thread exits).  A copy into pageable
// memory makes hipMemcpyAsync drain the stream on the host first and only then enqueue the transfer (15-20 us of idle device per
// read-back, 15 k read-backs per sweep); with page-locked memory the transfer is queued right behind the producing kernel.
// A slot belongs to the code named here; what it holds is valid until that code's next use of it on the same thread.
enum PinSlot {
    PIN_QR = 0,             // qr.hip: column norms and the permutation of the pivoted / rank-revealing factorisation
    PIN_SVD_READ = 2,       // (1 is free)  svd.hip: norms, convergence measures, results of the Jacobi SVD; site.hip: bond_deflate's norms
    PIN_SVD_UPLOAD = 3,     // svd.hip: tournament schedule, kept values / order (guarded by upload_slot_guard)
    PIN_CHAIN_PACK = 4,     // chain.hip: the packed statistics of the weighted pass
    PIN_CHAIN_UPLOAD = 5,   // chain.hip: row order of the weighted pass, Schmidt descriptors
    PIN_CHAIN_READ = 6,     // chain.hip: overlaps, Schmidt table
    PIN_SHARED = 7,         // three users, a few words each, none of which keeps the content across a call into another: the mailbox
                            // ring of the device-side pivoting (qr.hip, which clears it before use for that reason), the count of
                            // launches that gave up (cholqr_gaveup_count), the scalars of the beam search (beamsearch.hip)
    PIN_NSLOTS
};
void* pinned_host(size_t bytes, PinSlot slot);      // nullptr if the allocation fails (callers fall back to pageable memory)
// Read-back: `bytes` from `dev` on `st` through the slot (straight into pageable memory when there is none), then synchronise `st`.
// On return the data is in `host`.  A HIP failure comes back as the library's error code with "memcpy <what>" / "sync <what>".
int read_back(hipStream_t st, void* host, const void* dev, size_t bytes, PinSlot slot, const char* what);
// ... for a caller that reads in place: *data points at the staged bytes (or at a pageable buffer of the thread when there is no slot)
int read_back_staged(hipStream_t st, void** data, const void* dev, size_t bytes, PinSlot slot, const char* what);
// Upload: stage `bytes` from `host` in the slot and enqueue the copy to `dev` on `st`; `host` may be reused at once.  No
// synchronisation, unless there is no slot: a pageable source must outlive the copy, so `st` is synchronised then.
int upload(hipStream_t st, void* dev, const void* host, size_t bytes, PinSlot slot, const char* what);

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t align_up(int64_t a, int64_t b) { return cdiv(a, b) * b; }

// ---- workspace layouts -------------------------------------------------------------------------------------------------------
// The regions of a step's workspace are written down once, in its *_layout function, as a sequence of take() calls.  Run with a
// null base the sequence only adds the sizes up (the *_ws_bytes query), with the caller's workspace it hands out the pointers.
// Every region is rounded up to 256 bytes.
struct WsCarve {
    char* base;                     // nullptr: size run, every take() returns nullptr
    int64_t off = 0;
    template <typename T = char>
    T* take(int64_t bytes) {
        char* p = base ? base + off : nullptr;
        off += align_up(bytes, 256);
        return (T*)p;
    }
    int64_t total() const { return off; }
};
constexpr int64_t NORMALIZE_SCRATCH_BYTES = 8192;      // the scratch normalize_pow2 asks for (misc.hip; tn_normalize_pow2 in tnpeps.h)

// ---- optional event timing per kernel family (prof.hip) ---------------------------------------------
enum { PROF_GEMM_128x128 = 0, PROF_GEMM_128x32, PROF_GEMM_32x128, PROF_GEMM_64x64, PROF_SPLITK_REDUCE, PROF_ABSORB,
       PROF_GRAM, PROF_EIG, PROF_ROWS_SMALL, PROF_VECS_SMALL,
       PROF_PANEL,     // panel step of tn_qr (cholqr.hip) and the one-launch factorisation (smallqr.hip)
       PROF_LU,        // lu_reconstruct_kernel (Householder reconstruction of a panel)
       PROF_QR_AUX,    // diag_qr, assemble_R, init_Q, column norms, panel copies
       PROF_SVD_AUX,   // vector norms, init, gather of the Jacobi SVD
       PROF_MISC,      // nfactor / scaling / builders / beam kernels
       PROF_NKERNEL,   // ---- families above bracket kernel launches with events; the ones below are pure counters ----
       PROF_QR_NOMINAL = PROF_NKERNEL,   // per tn_qr call: calls, 4mn^2 - 4/3 n^3 flops, 8(2mn + n^2) bytes
       PROF_SVD_NOMINAL,                 // per tn_svd_trunc call: 14mn^2 + 8n^3 flops, 8(2mn + n^2 + n) bytes
       PROF_SVD_STREAM,                  // per tn_svd_trunc call: calls += executed sweeps, bytes += sweeps*(n-1)*16*n*(m+n)
       PROF_SVDVALS_NOMINAL,             // per tn_svdvals call: 4mn^2 - 4/3 n^3 flops, 8(mn + n) bytes
       PROF_SVD_ROUNDS,                  // per block-Jacobi SVD: calls += executed rounds (sweeps x rounds per sweep), flops += pair eigenproblems
       PROF_NFAM };
// phase a launch is attributed to (thread-local; set by the entry points that own a phase)
enum { PH_OTHER = 0, PH_ABSORB, PH_QR, PH_SVD, PH_SVDVALS, PH_BUILD, PH_N };
bool prof_on(int fam);
void prof_begin(hipStream_t st, int fam);
void prof_end(hipStream_t st, int fam, double flops, double bytes);
void prof_note(int fam, double calls, double flops, double bytes);   // counter-only families
// the nominal counts of the factorisations, booked by every entry point that runs one (formulas: the PROF_*_NOMINAL lines above)
void prof_note_qr(int64_t m, int64_t n, int64_t batch);              // PROF_QR_NOMINAL: `batch` factorisations of m x n
void prof_note_svd(int64_t k, int64_t n, int sweeps);                // PROF_SVD_NOMINAL + PROF_SVD_STREAM: one truncated SVD of k x n
void prof_note_svdvals(int64_t k, int64_t n);                        // PROF_SVDVALS_NOMINAL: the singular values of k x n
int prof_phase(int phase);                                           // returns the previous phase
struct ProfPhase {                                                    // scoped phase
    int prev;
    explicit ProfPhase(int ph) : prev(prof_phase(ph)) {}
    ~ProfPhase() { prof_phase(prev); }
};
// bracket one kernel launch of a family that has no flop/byte model
#define TN_PROF_LAUNCH(st, fam, launch) do { prof_begin(st, fam); launch; prof_end(st, fam, 0.0, 0.0); } while (0)
void prof_set_mask(unsigned mask);
void prof_set_sample(unsigned n);
void prof_reset();
void prof_get(int phase, int fam, uint64_t* calls, double* ms, double* flops, double* bytes);   // phase < 0: all phases

// ---- strided matrix view (element strides) -------------------------------------------------
struct Mat {
    double* p;
    int64_t rs, cs;     // row stride, column stride (in doubles)
};
static inline Mat mat(double* p, int64_t rs, int64_t cs) { return Mat{p, rs, cs}; }
static inline Mat sub(Mat a, int64_t i, int64_t j) { return Mat{a.p + i * a.rs + j * a.cs, a.rs, a.cs}; }
static inline Mat tr(Mat a) { return Mat{a.p, a.cs, a.rs}; }

// ---- internal GEMM entry (gemm_f64.hip) --------------------------------------------------------
// C[M,N] = alpha * A[M,K] * B[K,N] + beta * C, arbitrary element strides, optional batch.
// ws/ws_bytes: optional split-K scratch (may be null -> no split).
int gemm(hipStream_t st, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t rsa, int64_t csa,
         const double* B, int64_t rsb, int64_t csb, double beta, double* C, int64_t rsc, int64_t csc,
         int64_t batch = 1, int64_t bsa = 0, int64_t bsb = 0, int64_t bsc = 0, double* ws = nullptr,
         int64_t ws_bytes = 0);
int64_t gemm_ws_bytes(int64_t M, int64_t N, int64_t K, int64_t batch);
// Extended form: block-pair row indirection (see GemmP in gemm_f64.hip), forced split-K with the partial sums left in
// ws as [(batch*splitk + s)][M][N] (raw_partials), per-batch skip flags.
struct GemmExtra {
    const int* pairs = nullptr;
    const int* skip = nullptr;
    int pw = 0, mapA = 0, mapB = 0, mapC = 0;
    int force_splitk = 0;
    bool raw_partials = false;
    int* splitk_used = nullptr;
};
// how gemm_ex cuts K for force_splitk = s: returns the number of splits actually used, *kchunk = elements per split
int gemm_forced_split(int64_t K, int s, int64_t* kchunk);
int gemm_ex(hipStream_t st, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t rsa, int64_t csa,
            const double* B, int64_t rsb, int64_t csb, double beta, double* C, int64_t rsc, int64_t csc, int64_t batch,
            int64_t bsa, int64_t bsb, int64_t bsc, double* ws, int64_t ws_bytes, const GemmExtra* x);

static inline int gemm(hipStream_t st, int64_t M, int64_t N, int64_t K, double alpha, Mat A, Mat B, double beta, Mat C,
                       double* ws = nullptr, int64_t ws_bytes = 0) {
    return gemm(st, M, N, K, alpha, A.p, A.rs, A.cs, B.p, B.rs, B.cs, beta, C.p, C.rs, C.cs, 1, 0, 0, 0, ws, ws_bytes);
}
// the profiling family (PROF_GEMM_*) under which gemm books an unbatched M x N x K product with these strides of C
int gemm_prof_family(int64_t M, int64_t N, int64_t K, int64_t rsc, int64_t csc);

// ---- rank-b update of a trailing matrix (rank_update.hip): the K <= 32 products of the QR panel loops ---------------------------
// C (m x n) -= W (m x b) X (b x n), 1 <= b <= 32, element strides; bit for bit what gemm(..., -1.0, W, X, 1.0, C) computes.
// active (DEVICE, may be null): *active == 0 -> nothing is written
int rank_update(hipStream_t st, int64_t m, int64_t n, int b, const double* W, int64_t wrs, int64_t wcs, const double* X, int64_t xrs,
                int64_t xcs, double* C, int64_t rsc, int64_t csc, const int* active);
static inline int rank_update(hipStream_t st, int64_t m, int64_t n, int b, Mat W, Mat X, Mat C, const int* active = nullptr) {
    return rank_update(st, m, n, b, W.p, W.rs, W.cs, X.p, X.rs, X.cs, C.p, C.rs, C.cs, active);
}

// ---- the two products of a contraction through the MPS (x) MPO factors in one launch (factor_products.hip) ---------------------
//     S_z[(i, j), n] = sum_k P[z, i, k] X[k, j, n],    Out_z[m_hi Mlo + m_lo, n] = sum_q W[m, q] S_z[q, n],  q = i J + j
// element strides throughout.  Bit for bit what gemm (first product, K not split) followed by a batched gemm computes.
struct FactorProducts {
    int64_t Z, I, J, K1, N, Mhi, Mlo;
    const double* P; int64_t pz, pi, pk;
    const double* X; int64_t xk, xj, xn;
    const double* W; int64_t wm, wq;                // row m = m_hi Mlo + m_lo, column q
    double* Out; int64_t oz, ohi, olo, on;
};
bool factor_products_fits(int64_t Z, int64_t I, int64_t J, int64_t K1, int64_t N, int64_t M);      // the kernel's static limits
inline bool factor_products_on() { return env_flag_on("TN_FACTOR_FUSED"); }                          // read per call: the tests switch it
int factor_products(hipStream_t st, const FactorProducts& f);

// ---- small dense kernels (small.hip) ------------------------------------------------------------
constexpr int NBMAX = 64;      // largest panel / Jacobi pair width handled by the single-workgroup kernels

// Partial Gram matrices of `nvec` vectors of length L:  G[i][j] = sum_c X(i,c) X(j,c).
// Vector v, element c lives at X + vec_off[v] + c*es  where vec_off is given by (blk0,blk1,w,vs):
//   v <  w : (blk0*w + v) * vs ;  v >= w : (blk1*w + v - w) * vs.   pairs==nullptr -> single group blk0=0,blk1=1.
// Output: part[(g*nchunk + chunk)*nvec*nvec + i*nvec + j].
int gram_partial(hipStream_t st, const double* X, int64_t vs, int64_t es, int64_t L, int nvec, int w, const int* pairs,
                 int ngroups, int nchunk, double* part);
int gram_nchunk(int64_t L);

// Sum partials, (optionally) scale to unit diagonal, diagonalise with parallel-order Jacobi.
// mode 0: QR panel step  -> out = D^-1 J         (columns with squared norm <= dead_thresh are flagged in
//         dead[g*nvec+i] and get a zero row/column in out)
// mode 1: normalise only -> out = D^-1
// mode 2: SVD pair step  -> out = J (orthogonal), unscaled Gram; nrot[g] = rotations applied, maxoff[g] = largest
//         relative off-diagonal seen before rotating.
// relevant2 (mode 2): vectors with squared norm <= relevant2 are left out of the convergence measure maxoff.
// allow_fast (mode 2, 64 vectors): pairs in the quadratic regime may take the near-diagonal steps on the matrix cores instead of the
// cyclic sweeps (TN_EIG_FAST; see eig_small3_kernel).
int eig_small(hipStream_t st, const double* part, int nchunk, int nvec, int ngroups, int mode, int max_sweeps,
              double dead_thresh, double* out, int* dead, int* nrot, double* maxoff, double relevant2 = 0.0, int allow_fast = 1);

// In place:  X(r, 0:b) <- X(r, 0:b) * S   for r < nrows  (S is b x b row-major in global memory).
int rows_times_small(hipStream_t st, double* X, int64_t rs, int64_t cs, int64_t nrows, int b, const double* S);

// Out(v, c) = sum_u S[u][v] * In(u, c)  for the nvec vectors of each group (same addressing as gram_partial),
// c < L; in place when Out == In.  If nrot != nullptr groups with nrot[g]==0 are skipped.
// All Jacobi rounds of a block-pair SVD (jacobi_core, svd.hip) in one launch (small.hip).  norms: nvp + 4 doubles.
struct SvdRoundsJob {
    double* X; int64_t pitch, L; int nvp, w;
    const int* pairs; int ng, nr, nchunk;
    double* part; int64_t part_bytes; double* Js; int* nrot; double* maxoff;
    double relevant2, last_tol; int inner_first, inner_later;
    double* norms;
};
int svd_rounds_fused(hipStream_t st, const SvdRoundsJob& j);       // 0 launched, 1 not taken
int small_t_times_vecs(hipStream_t st, const double* S, double* X, int64_t vs, int64_t es, int64_t L, int nvec, int w,
                       const int* pairs, int ngroups, const int* nrot);


// ---- blocked QR (qr.hip): the factorisation behind tn_qr, tn_qr_batched, tn_site_qr and the chain driver -------------
int qr_factor(hipStream_t st, double* A, int64_t rs, int64_t cs, int64_t m, int64_t n, double* Q, int64_t qrs, int64_t qcs, double* R,
              int64_t rrs, int64_t rcs, int nb, void* ws, int64_t ws_bytes, double rank_tol, int64_t* keff_host,
              double* dropped2_host = nullptr, int frob_exit = 0, int64_t* pivot_perm_host = nullptr, double* nf_out2 = nullptr,
              int* nf_done = nullptr);
int64_t qr_ws_bytes(int64_t m, int64_t n, int nb);


// ---- iterated Cholesky-QR panel orthonormalisation (cholqr.hip), the default panel step -------------------------------
// the numbers of the iteration, shared with the one-launch factorisation (smallqr.hip)
constexpr int CQ_MAXPASS = 4;         // substitution passes enqueued per panel (later ones return at once when converged)
constexpr double CQ_THETA = 1e-10;    // deferral threshold on pivot / squared column norm
constexpr double CQ_DONE = 5e-15;     // Gram matrix = identity to rounding: converged
constexpr double CQ_LAST = 1e-8;      // below this one more pass lands at rounding level without another check
int64_t cholqr_ws_bytes(int64_t nrows, int b);
int cholqr_reset(hipStream_t st, void* ws);          // zero the state block at the head of ws once per call, before the first panel
// the stream's own state block (zero on return; see cholqr.hip) -- *state_out goes to the panel calls of this factorisation; the
// caller's first launch after the last panel clears the block (CQ_STATE_BYTES) and then tells cholqr_end_ok
int cholqr_begin(hipStream_t st, void* ws, void** state_out);
void cholqr_end_ok(hipStream_t st);
// fused_base: host counter of the call (0 at its start) for the single-launch form of small panels; NULL = six-launch chain
// state: the block from cholqr_begin, or NULL = the head of ws (cleared with cholqr_reset)
int cholqr_orthonormalize(hipStream_t st, const double* X, int64_t irs, int64_t ics, double* Y, int64_t rs, int64_t cs, int64_t nrows,
                          int b, void* ws, int64_t ws_bytes, uint64_t seed, int* fused_base, void* state = nullptr);
// the whole panel step: orthonormal basis, and with reconstruct != 0 the Householder reconstruction (Y, T, W = Y T^T, Wq = Y T)
int cholqr_panel(hipStream_t st, const double* X, int64_t irs, int64_t ics, double* Y, int64_t rs, int64_t cs, int64_t nrows, int b, void* ws,
                 int64_t ws_bytes, uint64_t seed, int reconstruct, double* Tp, double* W, int64_t wrs, int64_t wcs, double* Wq, int* fused_base,
                 void* state = nullptr, const int* active = nullptr);       // active (DEVICE, may be null): 0 = every launch of this panel returns at once
int cholqr_debug_state(hipStream_t st, const void* ws, int* ints9, double* dev_hist);
int cholqr_stats(unsigned long long* out16, int reset, hipStream_t st_or_null, int all_streams);
// one-launch factorisation of m x n, n <= 64 (smallqr.hip): 0 done, 1 shape / stream not taken, else error
bool smallqr_fits(int64_t m, int64_t n);
int64_t smallqr_ws_bytes(int64_t m, int64_t n);
int smallqr_factor(hipStream_t st, const double* A, int64_t rs, int64_t cs, int64_t m, int64_t n, double* Q, int64_t qrs, int64_t qcs, double* R,
                   int64_t rrs, int64_t rcs, double* nf_out2, void* ws, int64_t ws_bytes);

// ---- host side of the launches with in-kernel barriers (fused.hip): cq_fused_kernel, sq_kernel, svdl_kernel ---------------------
constexpr int CQ_FUSED_MAXBLK = 32;           // workgroups of an ordinary launch (a tall panel: up to twice that, see FusedTallLaunch)
constexpr unsigned CQ_SPIN_LIMIT = 1u << 22;  // looks at a barrier's counter before a launch gives up (seconds)
constexpr int CHOLQR_SLOTS = 64;              // streams with a slot of their own
int cholqr_stream_slot(hipStream_t st);       // statistics / state slot of a stream (CHOLQR_SLOTS = no slot of its own)
// address of slot `slot` (slot_bytes each) of the __device__ pool `symbol` (HIP_SYMBOL of the caller's own translation unit) on the
// current device; nullptr (and no HIP error left behind) when there is no current device or the symbol cannot be resolved
void* device_pool_slot(const void* symbol, size_t slot_bytes, int slot);
unsigned panel_spin_limit();                  // TN_PANEL_SPIN_LIMIT (tests: force the barriers to give up), read per call
int panel_maxpass();                          // TN_PANEL_MAXPASS (1 .. CQ_MAXPASS; tests: drive the Householder fallbacks), read once
// co-residency budget and time-outs, see fused.hip
int fused_maxblk();                           // largest ordinary launch the budget of this process allows (<= CQ_FUSED_MAXBLK)
bool fused_forms_allowed(hipStream_t st, int nwg);
void fused_forms_disable(hipStream_t st);
void fused_stream_released(hipStream_t st);
// admission of one launch of up to 2 fused_maxblk() workgroups (wanted == false: nothing is asked, nothing is held): when `admitted`,
// the admission lock is held until launched(), which records the launch, or the end of the scope
struct FusedTallLaunch {
    FusedTallLaunch(hipStream_t st, bool wanted);
    ~FusedTallLaunch();
    FusedTallLaunch(const FusedTallLaunch&) = delete;
    FusedTallLaunch& operator=(const FusedTallLaunch&) = delete;
    void launched();
    bool admitted = false;
private:
    hipStream_t st_;
    int slot_;
    void release();
};
void fused_note_launch();
bool fused_check_needed();
bool fused_check_deferred();
void fused_defer_push();
void fused_defer_pop();
struct FusedDeferCheck { FusedDeferCheck() { fused_defer_push(); } ~FusedDeferCheck() { fused_defer_pop(); } };
int fused_timeouts(hipStream_t st, int* count_out);       // synchronises st; *count_out > 0: redo the work since the last check
// what fused_timeouts needs from the two kernels: their sticky per-stream counts of launches that gave up, and a clean slate afterwards
int cholqr_gaveup_count(hipStream_t st, int slot, unsigned long long* count);     // (synchronises st)
void cholqr_state_dirty(int slot);            // the next cholqr_begin on this slot clears the state block with a memset
int smallqr_stats(hipStream_t st, unsigned long long* out4, int reset);
int smallqr_reset_state(hipStream_t st);

// ---- copies between strided matrices (qr.hip) ------------------------------------------------------------------------------------
// D (m x n, strides drs/dcs) <- S (m x n, strides srs/scs)
int copy_mat(hipStream_t st, const double* S, int64_t srs, int64_t scs, double* D, int64_t drs, int64_t dcs, int64_t m, int64_t n);

// ---- one-sided block Jacobi SVD (svd.hip): behind tn_svd_trunc, tn_svdvals* and the chain driver -----------------------------------
// C is k x n (element strides crs, ccs).  U: k x keep (urs, ucs), Vt: keep x n (vrs, vcs), S: keep values (all DEVICE); keep <= Dmax
// values above tol x the largest.  keep_out / discarded_out / sweeps_out / info are HOST pointers (info: 0 converged, 1 sweep cap).
int svd_trunc(hipStream_t st, const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, int64_t Dmax, double tol, double* U,
              int64_t urs, int64_t ucs, double* S, double* Vt, int64_t vrs, int64_t vcs, int64_t* keep_out, double* discarded_out,
              int* sweeps_out, int* info, void* ws, int64_t ws_bytes);
// singular values only, sorted descending, min(k, n) of them (deflated ones reported as 0) into hostS (HOST)
int svd_vals(hipStream_t st, const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, double* hostS, int* sweeps_out, int* info,
             void* ws, int64_t ws_bytes);
int64_t svd_ws_bytes(int64_t k, int64_t n, int vectors);
// both dimensions <= 64, no read-back: out (DEVICE, 66 doubles) = 64 values descending (zero padded), executed sweeps, convergence flag
int svd_vals_small_async(hipStream_t st, const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, double* out);
// ... `batch` of them in one launch: desc (DEVICE, 5 int64 per item: address, vector stride, element stride, vectors <= length, length)
int svd_vals_small_batched(hipStream_t st, const int64_t* desc, int64_t batch, double* out);

// ---- strided-batch forms (batch.hip): item i at base + i * bs*, results as for the single calls ------------------------------------
// side / nside: up to 8 streams the items are spread over (forked from and joined back into st); ws: batch x qr_ws_bytes, 256-aligned
int qr_batched(hipStream_t st, double* A, int64_t rs, int64_t cs, int64_t m, int64_t n, double* Q, int64_t qrs, int64_t qcs, double* R,
               int64_t rrs, int64_t rcs, int nb, double rank_tol, int64_t* keff_host, int64_t batch, int64_t bsA, int64_t bsQ, int64_t bsR,
               void* ws, int64_t ws_bytes, void* const* side, int nside);
// the items share ws and run one after the other (each reads its rank / convergence back); host outputs are arrays of `batch`
int svd_trunc_batched(hipStream_t st, const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, int64_t Dmax, double tol, double* U,
                      int64_t urs, int64_t ucs, double* S, double* Vt, int64_t vrs, int64_t vcs, int64_t* keep_host, double* discarded_host,
                      int* sweeps_host, int* info_host, int64_t batch, int64_t bsC, int64_t bsU, int64_t bsS, int64_t bsV, void* ws,
                      int64_t ws_bytes);
int svd_vals_batched(hipStream_t st, const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, double* S_host, int* sweeps_host,
                     int* info_host, int64_t batch, int64_t bsC, void* ws, int64_t ws_bytes);

// ---- absorption of an MPO site into an MPS site (absorb.hip), K1 ---------------------------------------------------------------
// out (Dl ba, pnew, Dr bb) = sum_s A (Dl, pold, Dr) W (ba, po, bb, pi); hconj: contracts po (pnew = pi), else pi (pnew = po); strided batch
int absorb(hipStream_t st, const double* A, const double* W, double* out, int64_t Dl, int64_t pold, int64_t Dr, int64_t ba, int64_t po,
           int64_t bb, int64_t pi, int hconj, int64_t batch, int64_t bsA, int64_t bsW, int64_t bsO);

// ---- power-of-two normalisation and elementwise scaling (misc.hip) ---------------------------------------------------------------
// out2 (DEVICE) = [nf, 1 / nf] with nf = 2^floor(log2(max|x|)); slot8: 8 bytes of device scratch
int nfactor(hipStream_t st, const double* x, int64_t n, double* out2, void* slot8);
// x /= nfactor(x), out2 as above; scratch: 8 KiB of device memory always suffice (unused for n <= 32768)
int normalize_pow2(hipStream_t st, double* x, int64_t n, double* out2, void* scratch, int64_t scratch_bytes);
int scale_by(hipStream_t st, double* x, int64_t n, const double* scalar_dev);                                    // x *= scalar_dev[0]
int scale_phys(hipStream_t st, double* A, int64_t Dl, int64_t p, int64_t Dr, const double* diag, int inv);       // A[dl, s, dr] *= diag[s] (inv: /=)

// ---- kernels of the branch-and-bound search (beam.hip, env.hip, peps.hip) ------------------------------------------------------
// conditional probabilities of the q states of the next cluster for nb branches (tnac4o.py:430-453): P (nb x q), minP (nb),
// log2p_out (may be null) = log2 P + parent_log2p
int calc_pn(hipStream_t st, const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap, const int32_t* pref,
            const int32_t* suf, const int32_t* lidx, const int32_t* uidx, int64_t nb, int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr,
            int64_t br, double* P, double* minP, const double* parent_log2p, double* log2p_out);
// one state of the next cluster drawn per sample from the conditional table of its boundary row, the table kept in LDS (sampler.hip):
// group g = samples perm[starts[g] .. starts[g+1]-1] sharing (pref, suf, lidx, uidx)[g]; child[k] = the state drawn with uniforms[k],
// log2p[k] += log2 P[child[k]], minP[g] = the table's flag as calc_pn's
int sample_pn(hipStream_t st, const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap, const int32_t* pref,
              const int32_t* suf, const int32_t* lidx, const int32_t* uidx, const int32_t* perm, const int64_t* starts, int64_t ng,
              const double* uniforms, int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr, int64_t br, int32_t* child, double* log2p, double* minP);
// the forced twin of sample_pn: member k takes its state s = forced[k * ld + pos] (int16) from the caller; child[k] = s, log2p[k] += log2 P[s],
// cell_log2p (may be null) [k * ld + pos] = that increment.  P[s] <= 0 or s outside [0, q): the increment is -inf (and child = 0 for the latter)
int score_pn(hipStream_t st, const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap, const int32_t* pref,
             const int32_t* suf, const int32_t* lidx, const int32_t* uidx, const int32_t* perm, const int64_t* starts, int64_t ng,
             const int16_t* forced, int64_t ld, int64_t pos, int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr, int64_t br, int32_t* child,
             double* log2p, double* cell_log2p, double* minP);
// merges the branches of each of ng groups (starts: ng + 1 offsets) that lie within min_dEng of the group's lowest energy
int merge_groups(hipStream_t st, const double* E, const double* lp, const int64_t* deg, const int64_t* pos, const int64_t* starts, int64_t ng,
                 double min_dEng, int64_t* rep_pos, int64_t* degn, double* lpn);
int nfactor_batched(hipStream_t st, double* x, int64_t batch, int64_t len);          // every row of x (batch x len) /= its own nfactor
// right / left environments of nk branch keys from those of their parents, each normalised by its power-of-two factor
int env_rr_batched(hipStream_t st, const double* A, const double* RRprev, const double* W, const int32_t* parent, const int32_t* uidx, int64_t nk,
                   int64_t Dl, int64_t p, int64_t Dr, int64_t bl, int64_t br, int64_t pu, double* out);
int env_rl_batched(hipStream_t st, const double* T1, const int32_t* par, const int32_t* didx, int64_t nk, int64_t p, int64_t Dr, double* out);
// diagonal scaling that balances the n x n matrix A (scale_out: n factors, clamped to [1 / max_scale, max_scale] when max_scale > 0)
int balance(hipStream_t st, const double* A, int64_t rs, int64_t cs, int64_t n, double max_scale, double* scale_out, int* iters_out);
// F (q, nl, nu): Boltzmann factor of a cluster with its left / upper couplings;  W (nl, pd, br, nu): the MPO site built from it
int peps_factor(hipStream_t st, const double* Es, const double* E1, const double* E4, const double* Xu, const double* Xl, const double* Xr,
                const double* Xd, const int32_t* dmap, const int32_t* rmap, int64_t q, int64_t nl, int64_t nu, double* F);
int mpo_from_factor(hipStream_t st, const double* F, const int32_t* dmap, const int32_t* rmap, int64_t q, int64_t nl, int64_t nu, int64_t pd,
                    int64_t br, double* W);
// Wops (1 + nop, nl, pd, br, nu): plane 0 = W, plane a = the same sum with F[s,l,u] weighted by O[a-1][s]  (O: nop x q)
int mpo_from_factor_ops(hipStream_t st, const double* F, const int32_t* dmap, const int32_t* rmap, const double* O, int64_t nop, int64_t q,
                        int64_t nl, int64_t nu, int64_t pd, int64_t br, double* Wops);

// ---- site steps of the boundary-MPS sweeps (site.hip); layouts and formulas at the definitions ----------------------------------
// attach (C != NULL) + QR + normalisation of one site.  side 0: Q (m x k), R (k x n) row-major; side 1: Q^T, R^T.  keff_host,
// normalised_host, dropped2_host, pivot_perm_host: HOST; nf_out2: DEVICE [nf, 1 / nf] (may be null: no normalisation)
int64_t site_qr_ws_bytes(int side, int64_t Dl, int64_t p, int64_t Dr, int64_t kc, int attach);
int site_qr(hipStream_t st, int side, double* A, int64_t Dl, int64_t p, int64_t Dr, const double* C, int64_t kc, double* Q, double* R,
            double rank_tol, int64_t* keff_host, double* nf_out2, int* normalised_host, void* ws, int64_t ws_bytes, double* dropped2_host,
            int frob_exit, int64_t* pivot_perm_host);
// out (c, s, c2) = RL (c x a) . A (a, s, a2) . RR (a2 x c2)
int64_t rar_ws_bytes(int64_t c, int64_t a, int64_t s, int64_t a2, int64_t c2);
int rar(hipStream_t st, const double* RL, const double* A, const double* RR, int64_t c, int64_t a, int64_t s, int64_t a2, int64_t c2, double* out,
        void* ws, int64_t ws_bytes);
// mixed environment of A (a, s, a2) and Ac (c, s, c2).  side 0: out (c2 x a2) from R (c x a); side 1: out (a x c) from R (a2 x c2)
int64_t env_mix_ws_bytes(int side, int64_t a, int64_t s, int64_t a2, int64_t c, int64_t c2);
int env_mix(hipStream_t st, int side, const double* R, const double* A, const double* Ac, int64_t a, int64_t s, int64_t a2, int64_t c, int64_t c2,
            double* out, void* ws, int64_t ws_bytes);
// projectors of a truncation: Al_new (ml x keep) = Al (ml x k0) U, Ar_new (keep x nr) = Vt Ar (k1 x nr), Cdiag = diag(S)
int64_t apply_truncation_ws_bytes(int64_t ml, int64_t k0, int64_t keep, int64_t k1, int64_t nr);
int apply_truncation(hipStream_t st, const double* Al, int64_t ml, int64_t k0, const double* U, int64_t urs, int64_t ucs, int64_t keep,
                     const double* Vt, int64_t vrs, int64_t vcs, const double* Ar, int64_t k1, int64_t nr, const double* S, double* Al_new,
                     double* Ar_new, double* Cdiag, void* ws, int64_t ws_bytes);
// bond weights from the Gram matrix G (n x n): d2 (n) = floored diagonal, stats (65) = 64 partial sums of ||K||_F^2 and max G_cc
int gram_weights(hipStream_t st, const double* G, int64_t n, double floor_rel, double* d2, double* stats);
int rows_norm2(hipStream_t st, const double* A, int64_t rows, int64_t cols, double* out);                       // out[r] = sum_c A[r, c]^2
// out[j, :] = sqrt(w2[perm[j]]) A[perm[j], :];  inverse: out[perm[j], :] = A[j, :] / sqrt(w2[perm[j]])
int gather_scale_rows(hipStream_t st, const double* A, int64_t rows, int64_t cols, const int64_t* perm, const double* w2, double* out, int inverse);
// drops the bond indices of a centre matrix C (k <= 256) that carry nothing, from C and the neighbouring site Q; *k_out (HOST) = kept
// indices, nothing is written when none is dropped.  ws: k doubles.  One read-back.
int bond_deflate(hipStream_t st, int side, const double* C, int64_t k, int64_t n, const double* Q, int64_t m, double* C_out, double* Q_out,
                 int64_t* k_out, double* dropped2_rel_out, void* ws, int64_t ws_bytes);

// ---- the two small reductions of the weighted first pass (chain.hip), exported as tn_weighted_sum / tn_argsort_desc ------------------
int weighted_sum(hipStream_t st, const double* a, const double* b, int64_t n, double* w, double* sum);     // w = a * b, sum[0] = sum_i w[i] in a fixed order
int argsort_desc(hipStream_t st, const double* w, int64_t n, int64_t* perm);                               // stable descending argsort (NaN first)

}  // namespace tn
