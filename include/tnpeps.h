/* libtnpeps — C-ABI of the MI355X boundary-MPS PEPS contraction kernels.
 *
 * The reference (marekrams/tnac4o) has no FFI layer; its hot path is the module surface of tnac4o/mps.py as
 * consumed by tnac4o/tnac4o.py.  Each entry point below names the reference code it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to float64 data unless its name ends in `_host`;
 *   - matrices are passed with explicit element strides (rs = row stride, cs = column stride), so transposed
 *     or sliced views never need a copy;
 *   - the caller owns every buffer including workspaces (sizes from the *_ws_bytes queries); nothing is
 *     allocated or freed by the library; outputs never alias inputs unless stated;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it.  tn_svd_trunc / tn_svdvals
 *     synchronise the stream internally (rank decisions are made on the host), the rest is asynchronous;
 *   - return 0 = ok, < 0 = argument error (nothing launched; -3 = a caller-sized buffer was too small, -7 = a launch with
 *     in-kernel barriers gave up and the inputs were consumed: rerun from a copy), > 0 = HIP runtime error code.  The
 *     message is available from tn_last_error() (thread-local).  Numerical events (non-convergence) are reported
 *     through `info` outputs, never as errors.
 *
 * State the library keeps (SURVEY.md 8b asks for none; what there is, is bookkeeping -- no result depends on it being there):
 *   - per host thread: the error text; a few page-locked staging buffers for small read-backs / uploads (grown on demand,
 *     freed when the thread exits); the event ring of the optional profiler (tn_profile_*); the stamp counter of the
 *     device-side panel pivoting (tn_qr / tn_site_qr with pivot_perm_host);
 *   - per (device, stream), created at the stream's first use and released by tn_stream_destroy (streams the caller
 *     destroys otherwise keep their slot: at most 64 slots, the streams beyond share the last one for statistics and do not
 *     take the single-launch forms): a slot number; a 256-byte __device__ state block for the panel step, one for the
 *     one-launch factorisation and one for the one-launch Jacobi rounds (barrier counters, cleared by the launch that ends
 *     a call); DIAGNOSTIC counters (tn_panel_stats*, tn_smallqr_stats); the STICKY count of launches that gave up at an
 *     in-kernel barrier (read by tn_fused_timeouts, never reset by the statistics calls); a flag "this stream is off the
 *     single-launch forms" set after such a time-out (from then on the multi-launch forms run: same results bit for bit);
 *     the event of a tall panel launch in flight (admission control of launches that need co-resident workgroups);
 *   - process-wide, read once: the co-residency budget (CUs of the device, GPU_MAX_HW_QUEUES, TN_PANEL_CU_BUDGET) and the
 *     switches of INTEGRATION.md section 3 (the ones marked "per call" are read at every call).
 * Thread-safety: every entry point may be called concurrently from different host threads on DIFFERENT streams (the
 * product drives one chain per thread and stream); the tables above are guarded by mutexes.  Two threads must not
 * enqueue on the SAME stream at once (workspaces and state blocks are per stream).  The library allocates no device
 * memory; the __device__ state pools are static.
 */
#ifndef TNPEPS_H
#define TNPEPS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* version of this C-ABI, currently 26 (bumped whenever a signature below changes; the binding checks it at load time) */
int tn_version(void);
/* copies the hash of the sources the library was built from (set by the build recipe) into buf; returns its length */
int tn_build_id(char* buf, int n);
/* A stream confined to the compute units set in mask_host (nwords x 32 bits); see tnac4o_amd/parallel.py (TN_CU_MASK). */
int tn_stream_create_masked(const uint32_t* mask_host, int nwords, void** stream_out);
int tn_stream_destroy(void* stream);
/* copies the calling thread's last error text into buf (NUL-terminated); returns its length */
int tn_last_error(char* buf, int n);

/* ---- K2: strided (batched) GEMM.  C = alpha * A[M,K] * B[K,N] + beta * C.
 * Replaces every np.tensordot of mps.py (_mps_CA/_mps_AC :740-746, _mps_RL/_RR :655-663, _mps_RAR :748-751,
 * projector application :579-580, bond_env/expectation :694-698, :765-769) and tnac4o.py:532, 1779-1780, 1792-1794.
 * ws may be NULL (disables split-K). */
int tn_gemm(int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t rsa, int64_t csa,
            const double* B, int64_t rsb, int64_t csb, double beta, double* C, int64_t rsc, int64_t csc,
            int64_t batch, int64_t bsa, int64_t bsb, int64_t bsc, void* ws, int64_t ws_bytes, void* stream);
int64_t tn_gemm_ws_bytes(int64_t M, int64_t N, int64_t K, int64_t batch);

/* ---- a pair of products through the MPS (x) MPO factors (csrc/factor_products.hip), element strides throughout:
 *     S_z[(i, j), n] = sum_{k < K1} P[z pz + i pi + k pk] X[k xk + j xj + n xn]                      z < Z, i < I, j < J, n < N
 *     Out[z oz + m_hi ohi + m_lo olo + n on] = sum_{q < I J} W[m wm + q wq] S_z[q, n]         q = i J + j, m = m_hi Mlo + m_lo
 * Bit for bit what two tn_gemm calls compute: the first product as ONE product (Z I) x (J N) x K1 with the workspace
 * tn_gemm_ws_bytes asks for (first_batched = 0; needs pz = I pi and xj = N xn) or as J products (Z I) x N x K1 without a workspace
 * (first_batched = 1), the second as Z products (Mhi Mlo) x N x (I J) without one.  Where tn_factor_products_eligible says 1 (the
 * shape fits the kernel and the launch plan does not split K1 of the first product) and TN_FACTOR_FUSED is not 0 this is one launch
 * that never writes S; otherwise the entry runs those tn_gemm launches itself, with S in ws (tn_factor_products_ws_bytes). */
int tn_factor_products_eligible(int64_t Z, int64_t I, int64_t J, int64_t K1, int64_t N, int64_t M, int first_batched);
int64_t tn_factor_products_ws_bytes(int64_t Z, int64_t I, int64_t J, int64_t K1, int64_t N, int first_batched);
int tn_factor_products(int64_t Z, int64_t I, int64_t J, int64_t K1, int64_t N, int64_t Mhi, int64_t Mlo, const double* P, int64_t pz,
                       int64_t pi, int64_t pk, const double* X, int64_t xk, int64_t xj, int64_t xn, const double* W, int64_t wm,
                       int64_t wq, double* Out, int64_t oz, int64_t ohi, int64_t olo, int64_t on, int first_batched, void* ws,
                       int64_t ws_bytes, void* stream);

/* ---- K1: MPO.MPS absorption of one site.  Replaces MPS.apply_mpo (mps.py:353-359) -> _mps_HA (:753-763).
 * A: (Dl, pold, Dr) C-order.  W: (ba, po, bb, pi) C-order, legs (left, out, right, in).
 * hconj=1: out (Dl*ba, pi, Dr*bb), MPS index major;  hconj=0: out (ba*Dl, po, bb*Dr), MPO index major.
 * batch >= 1 equally shaped sites in one launch (item i at A + i*bsA, W + i*bsW, out + i*bsOut; a stride of 0 shares the
 * operand between the items, e.g. one MPO site absorbed into the same site of several boundary MPS). */
int tn_absorb(const double* A, const double* W, double* out, int64_t Dl, int64_t pold, int64_t Dr, int64_t ba,
              int64_t po, int64_t bb, int64_t pi, int hconj, int64_t batch, int64_t bsA, int64_t bsW, int64_t bsOut,
              void* stream);

/* ---- K3: economic QR, diag(R) >= 0.  Replaces mps.qr (mps.py:43-59) as used by _mps_decompose_AC/CA (:772-800).
 * A (m x n) is DESTROYED.  Q: m x min(m,n), R: min(m,n) x n.  nb in {32, 64} is the panel width.
 * rank_tol = 0: the plain factorisation (asynchronous).  rank_tol > 0 (nb = 32, keff_host != NULL): early exit for the
 * truncating canonisation passes — every second panel the largest column norm of the unfactored trailing block is read
 * back; once it is <= rank_tol x the largest column norm of A the factorisation stops and *keff_host (HOST) receives
 * the number of columns of Q / rows of R produced (A = Q[:, :keff] R[:keff, :] to rank_tol * max column norm).  With
 * rank_tol = 2^-56 this drops exactly the rows the Jacobi SVD (tn_svd_trunc) would deflate.  Synchronises the stream
 * at each check.  *keff_host = min(m, n) otherwise. */
int tn_qr(double* A, int64_t rs, int64_t cs, int64_t m, int64_t n, double* Q, int64_t qrs, int64_t qcs, double* R,
          int64_t rrs, int64_t rcs, int nb, double rank_tol, int64_t* keff_host, void* ws, int64_t ws_bytes, void* stream);
int64_t tn_qr_ws_bytes(int64_t m, int64_t n, int nb);
/* The panel step of tn_qr on its own (test and measurement hook): Y (nrows x b, b <= 32) <- an orthonormal basis of the column
 * space of the panel X (read only, must not overlap Y; completed arbitrarily where X is rank deficient).
 * method must be 0: iterated Cholesky-QR with deferral (csrc/cholqr.hip, what tn_qr uses); other values are rejected.
 * state9_host / dev_host (both or neither; synchronises the stream): {ticket counter, done, final_next, passes applied,
 * input exponent, refill mask, deferred pivots, refilled columns, Householder fallback taken} and max|X^T X - I| before each pass.
 * tn_panel_stats_stream: DIAGNOSTIC counters of the panels launched on `stream` since its last reset (the library keeps them per
 * stream, so that concurrent chains do not mix their counts; streams beyond the 64th share one slot); tn_panel_stats: their sum
 * over all streams (reset clears all).  16 words: {panels, substitution passes applied, deferred pivots,
 * refilled columns, Householder fallbacks, panels with >= 3 passes, panels with >= 4 passes, panel elements x passes applied by the
 * six-launch chain, the same for the single-launch form, panels handled by the single-launch form, 0...}.  They feed bench.py's
 * accounting of the work the passes really did and nothing else; no result depends on them. */
int64_t tn_panel_orth_ws_bytes(int64_t nrows, int b);
int tn_panel_orth(const double* X, int64_t rs, int64_t cs, int64_t nrows, int b, double* Y, int64_t yrs, int64_t ycs, int method,
                  int* state9_host, double* dev_host, void* ws, int64_t ws_bytes, void* stream);
int tn_panel_stats(uint64_t* out16_host, int reset);
int tn_panel_stats_stream(uint64_t* out16_host, int reset, void* stream);
/* Factorisations of up to 64 columns (m >= n, at most 32 workgroups of rows, no pivoting) -- the plain `qr` of mps.py:43-59 as the
 * variational sweeps (mps.py:238-279) and the canonisation passes (mps.py:202-236) call it on 1024 x 64-class site matrices -- run as
 * ONE launch inside tn_qr / tn_site_qr (csrc/smallqr.hip: explicit-Q iterated Cholesky-QR, the triangular factors multiplied up, the
 * norm factor of mps.py:76-85 taken in the same launch); TN_QR_SMALL=0 keeps the blocked path.  DIAGNOSTIC counters of `stream`:
 * {factorisations, substitution passes applied, Householder fallbacks, launches that gave up at an in-kernel barrier}.
 * tn_fused_timeouts: the launches with in-kernel barriers (this one and the single-launch panel step) rely on their workgroups being
 * co-resident; the budget is derived from the device's CU count, GPU_MAX_HW_QUEUES and TN_PANEL_CU_BUDGET (the CUs this process may
 * count on when the card is shared).  A launch that gives up all the same poisons its outputs with NaN and is counted; every entry
 * point that used such launches asks before it returns (tn_compress_mps: once per call) and redoes the work through the six-launch
 * panel chain / the blocked path (same bits), or fails with -7 when its input was overwritten.  The hook reports how many launches of
 * `stream` gave up since the last check (synchronises the stream; a positive count takes the stream off these launch forms). */
int tn_smallqr_stats(uint64_t* out4_host, int reset, void* stream);
int tn_fused_timeouts(int* count_host, void* stream);
/* Strided batch of `batch` equally shaped QR problems (the rotations of examples/e06:97-109 at one site): item i
 * at A + i*bsA, Q + i*bsQ, R + i*bsR, keff_host[i].  ws_bytes >= batch * roundup(tn_qr_ws_bytes(m,n,nb), 256).  A factorisation
 * is a chain of latency-bound single-workgroup kernels, so the items are made CONCURRENT rather than fused: item i is enqueued on
 * side_streams[i % nside] (hipStream_t owned by the caller, nside <= 8), forked from and joined back into `stream` with events;
 * nside = 0 runs them one after the other on `stream`.  Per-item results are bit-identical to tn_qr. */
int tn_qr_batched(double* A, int64_t rs, int64_t cs, int64_t m, int64_t n, double* Q, int64_t qrs, int64_t qcs, double* R,
                  int64_t rrs, int64_t rcs, int nb, double rank_tol, int64_t* keff_host, int64_t batch, int64_t bsA, int64_t bsQ,
                  int64_t bsR, void* ws, int64_t ws_bytes, void* stream, void* const* side_streams, int nside);

/* ---- K4: truncated SVD of a centre matrix.  Replaces mps.svd (mps.py:24-40, sign gauge included) +
 * _mps_truncateC (:802-811): keep = min(#(S > S0*max(eps,tol)), Dmax), discarded = sqrt(sum S[keep:]^2)/S0.
 * C: k x n.  U: k x keep, S: keep values, Vt: keep x n are written for the first `keep` vectors only; buffers must
 * hold min(k, n, Dmax) vectors.  keep_host/discarded_host/sweeps_host/info_host are HOST pointers (may be NULL
 * except keep_host).  info: 0 converged, 1 sweep cap reached.
 * With up to 256 live vectors all Jacobi rounds run in ONE launch with the vectors resident in LDS (svdl_kernel: in-kernel barriers,
 * within the co-residency budget of the panel step; TN_SVD_FUSED=0 keeps three launches per round): same results bit for bit.  A launch
 * in which a barrier gave up reports it, the rounds are redone as separate launches inside the same call and the stream stays off the
 * single-launch forms (message on stderr); nothing non-finite is returned.
 * Range: the whole double range is served on every path.  The one-launch kernel (both dimensions <= 64) always scales its input by a
 * power of two; the block path does so when the largest squared row norm leaves 2^-320 .. 2^500 (entries of about 1e-48 .. 1e75) and
 * otherwise computes exactly what it computed before.  U, Vt, keep and discarded of 2^e C are those of C, S is 2^e S(C), while
 * nothing leaves the range.  -2 "svd: non-finite input" is returned only when an entry is NaN or Inf; nothing is written then.
 * An all-zero C: return 0, keep = 0, discarded = 0.0, nothing written. */
int tn_svd_trunc(const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, int64_t Dmax, double tol, double* U,
                 int64_t urs, int64_t ucs, double* S, double* Vt, int64_t vrs, int64_t vcs, int64_t* keep_host,
                 double* discarded_host, int* sweeps_host, int* info_host, void* ws, int64_t ws_bytes, void* stream);
/* ---- K5: singular values only, sorted descending, min(k,n) values written to HOST memory.
 * Replaces mps.svd_S (mps.py:62-73) as used by MPS.update_S (:550-560).
 * With both dimensions <= 64 (one launch) the input is scaled by a power of two inside the kernel: the full double range is served,
 * and S(2^e C) = 2^e S(C) bit for bit while nothing leaves the range.  A longer side above 64 (the block path of tn_svd_trunc, same
 * window: scaled by a power of two when the largest squared row norm leaves 2^-320 .. 2^500, untouched otherwise) serves the whole
 * range as well.  An all-zero C gives zeros.  A NaN or Inf entry, and nothing else: -2, "svd: non-finite input". */
int tn_svdvals(const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, double* S_host, int* sweeps_host,
               int* info_host, void* ws, int64_t ws_bytes, void* stream);
int64_t tn_svd_ws_bytes(int64_t k, int64_t n, int vectors);
/* K5 without the read-back, for centre matrices with both dimensions <= 64 (the Schmidt-value checks of the variational sweeps,
 * mps.py:550-560, whose results are only needed at the end of a sweep): one asynchronous launch; out66_dev (DEVICE) receives 64
 * values sorted descending (zero padded), then the executed sweeps and a convergence flag (1 = converged) as doubles.  Same range
 * as tn_svdvals; a NaN or Inf entry leaves 64 NaN values, sweeps 0 and flag 0 (the return code cannot know: the caller tests the
 * flag and the values, and takes such a matrix to tn_svdvals).  tn_svdvals_small_batched: per item, the others are unaffected. */
int tn_svdvals_async(const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, double* out66_dev, void* stream);
/* The same for `batch` centre matrices in ONE launch (one workgroup each): the Schmidt spectra of a whole variational sweep
 * (mps.py:550-560) are only compared at its end, so they are taken together after it.  Item i is described by 5 int64
 * {device address of C_i, vector stride, element stride, number of vectors, vector length} with the shorter side of C_i as the
 * vectors (k <= n: {C, crs, ccs, k, n}, else {C, ccs, crs, n, k}); desc_dev is that table on the device, desc_host the caller's
 * host copy of it (validated here, nothing on the device is dereferenced by the host); out66_dev + 66 i receives item i. */
int tn_svdvals_small_batched(const int64_t* desc_dev, int64_t batch, const int64_t* desc_host, double* out66_dev, void* stream);
/* Strided batches of the two SVD entry points (item i at C + i*bsC, U + i*bsU, S + i*bsS, Vt + i*bsV; the *_host outputs are
 * arrays of `batch` entries, S_host holds batch * min(k,n) values).  Ranks and convergence are read back per item, so the items
 * are issued one after the other and share the workspace of a single problem. */
int tn_svd_trunc_batched(const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, int64_t Dmax, double tol, double* U,
                         int64_t urs, int64_t ucs, double* S, double* Vt, int64_t vrs, int64_t vcs, int64_t* keep_host,
                         double* discarded_host, int* sweeps_host, int* info_host, int64_t batch, int64_t bsC, int64_t bsU,
                         int64_t bsS, int64_t bsV, void* ws, int64_t ws_bytes, void* stream);
int tn_svdvals_batched(const double* C, int64_t crs, int64_t ccs, int64_t k, int64_t n, double* S_host, int* sweeps_host,
                       int* info_host, int64_t batch, int64_t bsC, void* ws, int64_t ws_bytes, void* stream);

/* ---- K6: out2[0] = 2^floor(log2 max|x|), out2[1] = 1/out2[0] (device).  Replaces mps.nfactor (mps.py:76-85).
 * slot8: 8 bytes of device scratch. */
int tn_nfactor(const double* x, int64_t n, double* out2, void* slot8, void* stream);
/* x /= nfactor(x) in place and out2 = [nfactor, 1/nfactor] (the fused form of tn_nfactor + tn_scale_by used after every QR,
 * mps.py:781-782, 796-797): two launches, no memset.  scratch: >= 8 KiB of device memory owned by the caller. */
int tn_normalize_pow2(double* x, int64_t n, double* out2, void* scratch, int64_t scratch_bytes, void* stream);
/* x[i] *= scalar_dev[0]  (used with out2+1 of tn_nfactor: mps.py:782, 797; tnac4o.py:533, 1781) */
int tn_scale_by(double* x, int64_t n, const double* scalar_dev, void* stream);
/* A[dl, s, dr] *= diag[s] (inv=0) or /= diag[s] (inv=1).  Replaces MPS.apply_diagonalO (mps.py:361-366). */
int tn_scale_phys(double* A, int64_t Dl, int64_t p, int64_t Dr, const double* diag, int inv, void* stream);

/* ---- K7: structured PEPS-factor and MPO-site builder.  Replaces tnac4o._peps_tensor (tnac4o.py:1562-1672) and the sum
 * over the physical index at tnac4o.py:1686 without ever forming the dense (q,l,d,r,u) tensor:
 *   F[s,l,u] = exp((Es[s] + E1[s,l]) + E4[s,u]) * Xu[u] * Xl[l] * Xr[rmap[s]] * Xd[dmap[s]]     (q, nl, nu)
 *   W[l,d,r,u] = sum_{s: dmap[s]=d, rmap[s]=r} F[s,l,u]                                          (nl, pd, br, nu)
 * Es/E1/E4 are the beta-scaled min-shifted energy tables beta*(min E - E); dmap/rmap are int32. */
int tn_peps_factor(const double* Es, const double* E1, const double* E4, const double* Xu, const double* Xl, const double* Xr,
                   const double* Xd, const int32_t* dmap, const int32_t* rmap, int64_t q, int64_t nl, int64_t nu, double* F,
                   void* stream);
int tn_mpo_from_factor(const double* F, const int32_t* dmap, const int32_t* rmap, int64_t q, int64_t nl, int64_t nu, int64_t pd,
                       int64_t br, double* W, void* stream);
/* The same sum with operator weights on the cell's states, for the in-line correlation functions below:
 *   Wops[0] = W (bit for bit);   Wops[a][l,d,r,u] = sum_{s: dmap[s]=d, rmap[s]=r} O[a-1][s] F[s,l,u],  a = 1 .. nop
 * O (nop, q) row-major (may be NULL when nop = 0), Wops (1 + nop, nl, pd, br, nu).  One launch.  q <= 8192. */
int tn_mpo_from_factor_ops(const double* F, const int32_t* dmap, const int32_t* rmap, const double* O, int64_t nop, int64_t q, int64_t nl,
                           int64_t nu, int64_t pd, int64_t br, double* Wops, void* stream);

/* ---- K8: conditional probabilities of one cell for a batch of branches.  Replaces the per-branch loop
 * tnac4o.py:444-448 around _calculate_Pn (:1786-1807), including the negative-probability rule.
 *   T1: (npref, p, Dr)  left environment times the top MPS site, one row block per distinct prefix
 *   RR: (nsuf, Dr, br)  right environments per distinct suffix
 *   F : (q, nl, nu)     non-zero factor of the PEPS tensor, T[s,l,d,r,u] = F[s,l,u] [d=dmap[s]] [r=rmap[s]]
 *   per branch kk: pref[kk], suf[kk], lidx[kk], uidx[kk] (int32).  Out: P (nb, q) normalised, minP (nb).
 *   parent_log2p (nb) / log2p_out (nb, q), both or neither: log2p_out[kk, s] = log2(P[kk, s]) + parent_log2p[kk], the expansion of
 *   the branch log-probabilities of tnac4o.py:450-453 in the same launch: -inf where P is 0 or the parent is -inf, never NaN.
 * A NaN in one row d of one prefix's T1 stays in the branches of that prefix: their states with dmap[s] = d come back NaN (the other
 * entries of those tables mean nothing) and their flag is -1; every other branch is unchanged bit for bit.
 * Limit (argument error otherwise): (p Dr + Dr br + p br + q) * 8 <= 150 KiB of LDS.  tn_calc_pn, tn_sample_pn, tn_score_pn,
 * tn_env_rr_batched and tn_env_rl_batched check their arguments before the launch: a refused call (-1) writes nothing. */
int tn_calc_pn(const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap,
               const int32_t* pref, const int32_t* suf, const int32_t* lidx, const int32_t* uidx, int64_t nb,
               int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr, int64_t br, double* P, double* minP,
               const double* parent_log2p, double* log2p_out, void* stream);
/* ---- K8s: one state of the next cell drawn per sample, from the conditional table of the sample's boundary row.  Replaces the
 * table read-back, cumsum and per-sample np.searchsorted of gibbs_sampling (tnac4o.py:614-622).  Samples with the same boundary row
 * form a group; one workgroup per group builds the table exactly as tn_calc_pn does (same bits), keeps it in LDS, forms its running
 * sum there in an order that depends on q alone, and every member finds its state by binary search.
 *   T1, RR, F, dmap, rmap, q, nl, nu, p, Dr, br   as tn_calc_pn
 *   pref, suf, lidx, uidx (int32[ng])             the boundary row of every GROUP
 *   perm (int32), starts (int64[ng + 1])          members of group g: the sample indices perm[starts[g] .. starts[g+1]-1]
 *   uniforms (double, indexed by sample index)    numbers in [0, 1)
 * Out, per sample k: child_out[k] (int32) = first s with cum[s] >= uniforms[k] (np.searchsorted, side 'left'), moved forward to the
 * next s with P[s] > 0 when P[s] = 0, and the last s with P[s] > 0 when uniforms[k] > cum[q-1]; log2p_inout[k] += log2 P[child].
 * Per group: minP_out[g] as tn_calc_pn's.  Limits (argument error otherwise): tn_calc_pn's, and the table with its running sum in
 * 150 KiB of LDS: (max(p Dr + Dr br + p br, q) + q) * 8 <= 150 KiB. */
int tn_sample_pn(const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap, const int32_t* pref,
                 const int32_t* suf, const int32_t* lidx, const int32_t* uidx, const int32_t* perm, const int64_t* starts, int64_t ng,
                 const double* uniforms, int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr, int64_t br, int32_t* child_out,
                 double* log2p_inout, double* minP_out, void* stream);
/* ---- K8f: the forced twin of tn_sample_pn: every sample brings the state of its next cell instead of a uniform number, and gets the
 * log2 of the conditional probability of that state.  Groups, table (built exactly as tn_calc_pn builds it: same bits) and minP_out as
 * tn_sample_pn; no running sum is formed and nothing is searched.
 *   forced (int16, DEVICE), ld, pos               the state of sample k is s = forced[k * ld + pos], 0 <= pos < ld
 * Out, per sample k: child_out[k] (int32) = s; log2p_inout[k] += log2 P[s]; cell_log2p (may be NULL) [k * ld + pos] = that increment.
 * An entry P[s] that is not positive gives the increment -inf, never NaN, and every later finite increment leaves the sum -inf.  A state
 * outside [0, q) is never used as an index: its increment is -inf and child_out[k] = 0.  Limits (argument error otherwise):
 * tn_calc_pn's, (p Dr + Dr br + p br + q) * 8 <= 150 KiB of LDS. */
int tn_score_pn(const double* T1, const double* RR, const double* F, const int32_t* dmap, const int32_t* rmap, const int32_t* pref,
                const int32_t* suf, const int32_t* lidx, const int32_t* uidx, const int32_t* perm, const int64_t* starts, int64_t ng,
                const int16_t* forced, int64_t ld, int64_t pos, int64_t q, int64_t nl, int64_t nu, int64_t p, int64_t Dr, int64_t br,
                int32_t* child_out, double* log2p_inout, double* cell_log2p, double* minP_out, void* stream);
/* ---- a12: merge of the branches of a site-step with identical boundary indices (tnac4o.py:481-509).  The candidates arrive sorted by
 * group, in candidate order inside a group: E, log2p, deg, pos (their position in the candidate list), group g = members starts[g] ..
 * starts[g+1]-1 (ngroups + 1 offsets).  Per group: rep_pos_out = position of the FIRST member of minimal energy, deg_out = sum of the
 * degeneracies of the members within min_dEng of that minimum, log2p_out = the representative's log2p when it is alone in that set,
 * else the mean over the set added up in member order.  An empty group (starts[g] == starts[g+1]) reads no member and returns
 * rep_pos_out = -1, deg_out = 0, log2p_out = -inf. */
int tn_merge_groups(const double* E, const double* log2p, const int64_t* deg, const int64_t* pos, const int64_t* starts, int64_t ngroups,
                    double min_dEng, int64_t* rep_pos_out, int64_t* deg_out, double* log2p_out, void* stream);
/* ---- K9: per-item power-of-two normalisation of a batch of environments (tnac4o.py:533, 1781):
 * each of the `batch` contiguous blocks of `len` doubles is divided by its own nfactor. */
int tn_nfactor_batched(double* x, int64_t batch, int64_t len, void* stream);
/* ---- K9: right environments of every distinct boundary suffix of the beam for one site.  Replaces the body of the key loop
 * of tnac4o._setup_RR (tnac4o.py:1777-1783): gather of the parent environment, both contractions and the nfactor rescale,
 * one launch for all keys, no (Dl p) x br intermediate.
 *   A: (Dl, p, Dr) top boundary-MPS site;  RRprev: (nprev, Dr, br) environments of the previous level;
 *   W: (bl, p, br, pu) row-MPO site (legs left, down, right, up);  parent[k] (row of RRprev), uidx[k] (up index) int32;
 *   out[k, x, l] = sum_{d, x', r} A[x, d, x'] RRprev[parent[k], x', r] W[l, d, r, uidx[k]]  / nfactor(out[k]).   (nk, Dl, bl)
 * Limits (argument error otherwise): Dl * bl <= 2048, (Dr*br + bl*p*br + Dr*bl) * 8 <= 150 KiB. */
int tn_env_rr_batched(const double* A, const double* RRprev, const double* W, const int32_t* parent, const int32_t* uidx,
                      int64_t nk, int64_t Dl, int64_t p, int64_t Dr, int64_t bl, int64_t br, int64_t pu, double* out,
                      void* stream);
/* ---- K9: left environments of the new distinct prefixes (tnac4o.py:528-535).  T1 = RL . A (npref, p, Dr) is the product K8
 * already uses, so RL'[k] = RL[par] . A[:, d, :] is row (par[k], didx[k]) of it:  out[k, :] = T1[par[k], didx[k], :] / nfactor. */
int tn_env_rl_batched(const double* T1, const int32_t* par, const int32_t* didx, int64_t nk, int64_t p, int64_t Dr,
                      double* out, void* stream);
/* ---- bond balancing of the preconditioner.  Replaces scipy.linalg.matrix_balance(env, permute=False, separate=True) and the
 * clamp that follows it (tnac4o.py:1845-1847): LAPACK dgebal, job 'S' (radix 2, 2-norms), on the n x n matrix A (n <= 64,
 * element strides rs/cs).  scale_out[i] (device, n doubles) = min(max(scale[i], 1/max_scale), max_scale); max_scale <= 0
 * disables the clamp.  iters_out (device int, may be NULL) = passes of the outer loop. */
int tn_balance(const double* A, int64_t rs, int64_t cs, int64_t n, double max_scale, double* scale_out, int* iters_out,
               void* stream);

/* ---- site steps of the sweeps as single calls (compositions of the kernels above with their temporaries in `ws`; results are
 * bit-identical to the separate calls).  They exist for the host: with 4 chains driven by 4 host threads every separate call and
 * every temporary tensor is a GIL hand-over.  All matrices contiguous, row-major (C order).
 * tn_site_qr: attach + QR + nfactor of one canonisation step (mps.py:368-380, 532-548, 772-800).
 *   side 0 (left sweep):  M = C (kc x Dl) . A (Dl, p, Dr), QR of the (kc p) x Dr matrix: Q (kc p x k), R (k x Dr).
 *   side 1 (right sweep): M = A (Dl, p, Dr) . C (Dr x kc), QR of the transposed (p kc) x Dl view: Q receives Q^T (k x p kc),
 *                         R receives R^T (Dl x k).        k = min of the two matrix dimensions.
 *   C == NULL: no attach, A itself is factored and DESTROYED (kc ignored).  rank_tol / keff_host as in tn_qr.
 *   nf_out2 != NULL: when the factorisation ran to the end the triangular factor is divided by its nfactor and nf_out2 (device)
 *   = [nf, 1/nf]; *normalised_host tells whether that happened (it does not after an early exit: the caller slices first).
 *   dropped2_host (HOST, may be NULL): squared Frobenius norm of the trailing block an early exit dropped (0 otherwise).
 *   frobenius_exit = 1: the early exit compares the Frobenius norm of the trailing block with rank_tol x the Frobenius norm of
 *   the input (instead of the largest column norms of the two).
 *   pivot_perm_host (HOST, n int64 with n = columns of the factored matrix, may be NULL): panel pivoting.  Before every panel
 *   the residual norms of all remaining columns are read back; the factorisation stops when their Frobenius norm is below
 *   rank_tol x the input's, otherwise the 32 columns with the largest residuals form the next panel.  The triangular factor
 *   is returned in the pivoted column order; pivot_perm_host[j] = input column at position j. */
int64_t tn_site_qr_ws_bytes(int side, int64_t Dl, int64_t p, int64_t Dr, int64_t kc, int attach);
int tn_site_qr(int side, double* A, int64_t Dl, int64_t p, int64_t Dr, const double* C, int64_t kc, double* Q, double* R,
               double rank_tol, int64_t* keff_host, double* nf_out2, int* normalised_host, double* dropped2_host,
               int frobenius_exit, int64_t* pivot_perm_host, void* ws, int64_t ws_bytes, void* stream);
/* ---- helpers of the weighted rank-revealing first canonisation pass (tnac4o_amd/mps.py: canonise_right_weighted; no
 * counterpart in the reference, whose first pass factors every site in full, mps.py:187):
 * tn_gram_weights: from the Gram matrix G (n x n) of the unfactored part on the other side of a bond, the squared weight of
 *   every bond index, d2[c] = max(G_cc, floor_rel max G), and stats65 = [ 64 partial sums of ||K||_F^2 with K = G / (d d^T) (to be
 *   added in order: reproducible bit for bit), max_c G_cc ].  Precondition: max_c G_cc > 0 (the chain's G is the Gram matrix of a
 *   nonzero state).  An all-zero G is not rejected (that would take a read-back): it yields d2 = 0, stats65[64] = 0 -- the sign a caller
 *   tests -- and NaN partial sums for the parts that hold rows.
 * tn_rows_norm2: out[r] = sum_c A[r,c]^2 for a row-major rows x cols matrix.
 * tn_gather_scale_rows: inverse = 0: out[j,:] = sqrt(w2[perm[j]]) A[perm[j],:];  inverse = 1: out[perm[j],:] = A[j,:] / sqrt(w2[perm[j]])
 *   (perm: int64 device vector). */
int tn_gram_weights(const double* G, int64_t n, double floor_rel, double* d2_out, double* stats65_out, void* stream);
int tn_rows_norm2(const double* A, int64_t rows, int64_t cols, double* out, void* stream);
int tn_gather_scale_rows(const double* A, int64_t rows, int64_t cols, const int64_t* perm, const double* w2, double* out, int inverse,
                         void* stream);
/* ---- a truncation that cannot truncate (reference: MPS.truncateC, mps.py:562-585 -> _mps_truncateC, mps.py:802-811, as called by the
 * 4 chi / 2 chi passes of compress_mps, mps.py:192-195).  With min(C.shape) <= Dmax and tol <= eps the reference's rule only removes
 * singular values below eps S0 and turns the bond into the Schmidt basis; inside an intermediate pass neither is visible afterwards
 * (the next canonisation step's triangular factor does not depend on an orthogonal change of the bond, the variational sweep is
 * covariant under it).  tn_bond_deflate removes the same noise without a decomposition: C sits between an orthonormal site Q and a
 * canonical rest, so zeroing bond index i changes the state by exactly the norm of row (side 0) / column (side 1) i of C; indices are
 * dropped in ascending order of that norm while the dropped squares add up to at most eps^2 max_i ||C_i||^2 (<= (eps S0)^2), and C and
 * Q are gathered to the kept indices (in their order).
 *   side 0 (left sweep):  C (k x n), Q (m x k)  ->  C_out (k' x n), Q_out (m x k')        side 1: C (n x k), Q (k x m) -> (n x k'), (k' x m)
 * all row-major and contiguous, 1 <= k <= 256.  *k_out_host = k'; when k' == k nothing was written and the caller keeps C and Q.
 * *dropped2_rel_host = dropped squares / max_i ||C_i||^2.  ws: k doubles.  One read-back (synchronises the stream). */
int tn_bond_deflate(int side, const double* C, int64_t k, int64_t n, const double* Q, int64_t m, double* C_out, double* Q_out,
                    int64_t* k_out_host, double* dropped2_rel_host, void* ws, int64_t ws_bytes, void* stream);
/* out (c, s, c2) = RL (c x a) . A (a, s, a2) . RR (a2 x c2)      (MPS._mps_RAR, mps.py:748-751) */
int64_t tn_rar_ws_bytes(int64_t c, int64_t a, int64_t s, int64_t a2, int64_t c2);
int tn_rar(const double* RL, const double* A, const double* RR, int64_t c, int64_t a, int64_t s, int64_t a2, int64_t c2, double* out,
           void* ws, int64_t ws_bytes, void* stream);
/* mixed environments (MPS._mps_RL / _mps_RR, mps.py:655-663), A (a, s, a2), Ac (c, s, c2):
 *   side 0: out (c2 x a2) = sum_{c,s,a} Ac[c,s,c2] R[c,a] A[a,s,a2];   side 1: out (a x c) = sum A[a,s,a2] R[a2,c2] Ac[c,s,c2] */
int64_t tn_env_mix_ws_bytes(int side, int64_t a, int64_t s, int64_t a2, int64_t c, int64_t c2);
int tn_env_mix(int side, const double* R, const double* A, const double* Ac, int64_t a, int64_t s, int64_t a2, int64_t c, int64_t c2,
               double* out, void* ws, int64_t ws_bytes, void* stream);
/* projectors of a truncation pushed into the neighbouring sites and the diagonal centre (mps.py:579-583):
 *   Al_new (ml x keep) = Al (ml x k0) . U (k0 x keep, strides urs/ucs);  Ar_new (keep x nr) = Vt (keep x k1, strides vrs/vcs) . Ar (k1 x nr);
 *   Cdiag (keep x keep) = diag(S). */
int64_t tn_apply_truncation_ws_bytes(int64_t ml, int64_t k0, int64_t keep, int64_t k1, int64_t nr);
int tn_apply_truncation(const double* Al, int64_t ml, int64_t k0, const double* U, int64_t urs, int64_t ucs, int64_t keep,
                        const double* Vt, int64_t vrs, int64_t vcs, const double* Ar, int64_t k1, int64_t nr, const double* S,
                        double* Al_new, double* Ar_new, double* Cdiag, void* ws, int64_t ws_bytes, void* stream);

/* ---- thermal cluster marginals (tnac4o.calculate_marginals; no counterpart in the reference, which only samples).
 * One row ny of the lattice between its two boundaries: At (Dt, pd, Dt2) a site of rhoT[ny+1], W (bl, pd, br, pu) the row-MPO site
 * W[l,d,r,u], Ab (Db, pu, Db2) a site of rhoB[ny]; all contiguous.  Environments keep the MPO bond outermost.
 *   tn_env3 side 0 (left step):  out EL' (br, Dt2, Db2) = sum EL (bl, Dt, Db) . At . W . Ab
 *           side 1 (right step): out ER (bl, Dt, Db)    = sum At . W . Ab . ER' (br, Dt2, Db2)
 *   the result is divided by its nfactor (a power of two); *log2nf_out = *log2nf_in (0 when null) + log2(nfactor), a device scalar.
 *   half_out (may be null): receives the step's first product, the half of the cell marginal this side contributes:
 *           side 0: HL (bl, pd, Dt2, Db) = sum_t EL . At;   side 1: HR (pu, br, Dt2, Db) = sum_b' ER' . Ab.
 * No counterpart in the reference. */
int64_t tn_env3_ws_bytes(int side, int64_t Dt, int64_t pd, int64_t Dt2, int64_t bl, int64_t br, int64_t pu, int64_t Db, int64_t Db2);
int tn_env3(int side, const double* E, const double* At, const double* W, const double* Ab, int64_t Dt, int64_t pd, int64_t Dt2, int64_t bl,
            int64_t br, int64_t pu, int64_t Db, int64_t Db2, const double* log2nf_in, double* out, double* log2nf_out, double* half_out,
            void* ws, int64_t ws_bytes, void* stream);
/* Marginal of one cell from the two half-products of tn_env3 at that cell (K = Dt2 Db):
 *   X[l,d,u,r] = sum_K HL[(l,d),K] HR[(u,r),K];   P[s] prop. to sum_{l,u} F[s,l,u] X[l,dmap[s],u,rmap[s]]   (F (q, bl, pu); int32 maps)
 * then the negative-probability rule of tn_calc_pn (minP: its relative magnitude, <= 0; -1 for an all-zero table, which comes back
 * uniform) and the normalisation to sum 1.  *log2z = log2(sum of the raw table) + *log2L + *log2R (nulls count 0): the log2 of the
 * row contraction <rhoB[ny]| row ny |rhoT[ny+1]> when log2L / log2R are the running totals of the environments.  q <= 16384.
 * No counterpart in the reference. */
int64_t tn_cluster_marginal_ws_bytes(int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K);
int tn_cluster_marginal(const double* HL, const double* HR, const double* F, const int32_t* dmap, const int32_t* rmap, int64_t q, int64_t bl,
                        int64_t pd, int64_t br, int64_t pu, int64_t K, const double* log2L, const double* log2R, double* P, double* minP,
                        double* log2z, void* ws, int64_t ws_bytes, void* stream);
/* Nearest-neighbour bond marginals of one cell (tnac4o.calculate_correlations), same operands and X as tn_cluster_marginal:
 *   Pl (q, bl)[s,l] = sum_u F[s,l,u] X[l,dmap[s],u,rmap[s]] / T,   Pu (q, pu)[s,u] = sum_l F[s,l,u] X[l,dmap[s],u,rmap[s]] / T
 * row-major fp64, T = sum_{s,l,u} F X the raw total of both (no negative-probability rule: sums stay exact); l and u carry the
 * left and the upper neighbour's bond index, so Pl / Pu are the joint laws of the cell with those neighbours.  minB =
 * min(0, smallest entry of either table); an all-zero T gives uniform tables and minB = -1.  *log2z = log2(T) + *log2L + *log2R,
 * as tn_cluster_marginal.  dmap / rmap entries out of range contribute 0.  q <= 16384.  No counterpart in the reference. */
int64_t tn_cluster_bond_marginal_ws_bytes(int64_t q, int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K);
int tn_cluster_bond_marginal(const double* HL, const double* HR, const double* F, const int32_t* dmap, const int32_t* rmap, int64_t q,
                             int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K, const double* log2L, const double* log2R, double* Pl,
                             double* Pu, double* minB, double* log2z, void* ws, int64_t ws_bytes, void* stream);
/* In-line two-point functions (tnac4o.calculate_correlation_function): a STACK of left environments of one row, E (nE, bl, Dt, Db).
 * Slot 0 is the plain environment of tn_env3; every other slot has an operator inserted at an earlier cell.
 *   tn_env3_stack: the left step of the whole stack through (At, Wops, Ab), Wops (1 + nop, bl, pd, br, pu) from
 *   tn_mpo_from_factor_ops.  out (nE + nop, br, Dt2, Db2): slots 0 .. nE-1 are the input slots stepped through Wops[0], slot nE + a
 *   is slot 0 stepped through Wops[1 + a] (nop = 0: pure propagation).  ALL slots are divided by the nfactor of slot 0 (a power of
 *   two, so ratios between slots are untouched); *log2nf_out = *log2nf_in (0 when null) + its log2, as tn_env3.
 *   half_out (may be null; nE, bl, pd, Dt2, Db): the first products HL of the input slots, what tn_stack_cell_law consumes.
 *   The workspace query takes own_half = 1 when half_out is null (the first products then live in the workspace), else 0.
 *   2 + min(br, pu) GEMM launches (3 + with nop > 0) whatever nE; no atomics, the result does not depend on the workspace.
 *   tn_stack_cell_law: closes every slot at one cell with the right half-product HR (pu, br, Dt2, Db) of tn_env3 (K = Dt2 Db):
 *   D (nE, q)[e,s] = sum_{l,u} F[s,l,u] X_e[l,dmap[s],u,rmap[s]],  X_e = HL[e] . HR^T.   Raw: no negativity rule, no division;
 *   D[0,:] / sum(D[0,:]) is the cell law, sum(D[0,:]) the raw row total.  dmap / rmap entries out of range contribute 0.
 * No counterpart in the reference. */
int64_t tn_env3_stack_ws_bytes(int64_t nE, int64_t nop, int64_t Dt, int64_t pd, int64_t Dt2, int64_t bl, int64_t br, int64_t pu, int64_t Db,
                               int64_t Db2, int own_half);
int tn_env3_stack(const double* E, const double* At, const double* Wops, const double* Ab, int64_t nE, int64_t nop, int64_t Dt, int64_t pd,
                  int64_t Dt2, int64_t bl, int64_t br, int64_t pu, int64_t Db, int64_t Db2, const double* log2nf_in, double* out,
                  double* log2nf_out, double* half_out, void* ws, int64_t ws_bytes, void* stream);
int64_t tn_stack_cell_law_ws_bytes(int64_t nE, int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K);
int tn_stack_cell_law(const double* HL, const double* HR, const double* F, const int32_t* dmap, const int32_t* rmap, int64_t q, int64_t nE,
                      int64_t bl, int64_t pd, int64_t br, int64_t pu, int64_t K, double* D, void* ws, int64_t ws_bytes, void* stream);

/* ---- measurement: bracket every launch of the selected kernel families with HIP events on the launch stream.
 * family ids: 0-3 gemm_kernel<128,128> / <128,32> / <32,128> / <64,64> (all operand layouts), 4 splitk_reduce,
 * 5 absorb, 6 gram_partial, 7 eig_small, 8 rows_times_small, 9 small_t_times_vecs, 10 panel step (cholqr.hip, smallqr.hip),
 * 11 lu_reconstruct, 12 QR auxiliaries (diag_qr, assemble_R, init_Q, norms, copies), 13 SVD auxiliaries (norms, init,
 * gather), 14 misc (nfactor, scaling, builders, beam kernels).
 * mask bit f enables family f.  tn_profile_get synchronises the recorded events and returns totals since the last
 * reset: launches, summed duration (ms), algorithmic flops and bytes (SURVEY.md §8d counts).
 * Counter-only families (no events; active whenever any family is enabled): 15 tn_qr nominal (calls, 4mn^2-4/3n^3,
 * 8(2mn+n^2)), 16 tn_svd_trunc nominal (14mn^2+8n^3, 8(2mn+n^2+n)), 17 Jacobi streaming model (calls = executed
 * sweeps, bytes = sweeps*(n-1)*16*n*(m+n)), 18 tn_svdvals nominal (4mn^2-4/3n^3, 8(mn+n)), 19 block-Jacobi rounds (calls =
 * executed rounds of all tn_svd_trunc / tn_svdvals calls, flops = pair eigenproblems).
 * tn_profile_get_phase splits the same totals by the entry point that issued the launch: phase 0 other (attach /
 * projector / environment GEMMs, scaling), 1 tn_absorb, 2 tn_qr, 3 tn_svd_trunc, 4 tn_svdvals, 5 MPO builders;
 * phase -1 = all. */
void tn_profile_enable(unsigned mask);
void tn_profile_reset(void);
/* bracket only every `every`-th launch of an enabled family (default 1 = all): totals then cover the sampled launches */
void tn_profile_sample(unsigned every);
int tn_profile_get(int family, uint64_t* calls_host, double* ms_host, double* flops_host, double* bytes_host);
int tn_profile_get_phase(int phase, int family, uint64_t* calls_host, double* ms_host, double* flops_host, double* bytes_host);

/* ---- the chain driver: MPS.apply_mpo (mps.py:353-359) + MPS.compress_mps (mps.py:175-200) of ONE boundary MPS in ONE call ------------
 * What tnac4o.py:1688-1693 does per row (copy, apply_mpo, compress_mps) without a host interpreter between the ~600 kernel-launching
 * steps: the same kernels on the same operands in the same order as the per-step entry points above (bit-identical results), walked in
 * C++ on the caller's thread.  Every intermediate tensor lives in `arena` (DEVICE, 256-byte aligned, arena_bytes >=
 * tn_compress_mps_arena_bytes(...)), managed by a host-side allocator inside the call; the library still allocates nothing on the device.
 *   sites_host[n]   DEVICE pointer to MPS site n, (Dl, p, Dr) C-order, dims in site_dims_host[3n .. 3n+2]; read only
 *   mpo_host[n]     DEVICE pointer to MPO site n (ba, po, bb, pi) C-order (dims in mpo_dims_host[4n ..]) or NULL = no absorption at
 *                   that site; mpo_host itself may be NULL (compress only).  hconj as for tn_absorb
 *   Dmax, tolS, tolV, max_sweeps, graduate   the arguments of compress_mps (graduate_truncation as 0/1)
 *   flags           bit 0: weighted rank-revealing first pass (MPS.canonise_right_weighted), bit 1: its Gram recursion
 *                   through the MPS (x) MPO structure, bit 2: lazy Schmidt values in a stage's last sweep
 *   out             DEVICE, L slots of out_slot doubles: compressed site n (left-canonical, C-order) at out + n*out_slot, its dims in
 *                   out_dims_host[3n ..]
 *   overlap_host    <psi|phi> returned by compress_mps;  discarded_host[L+1]: MPS.discarded;  schmidt_host ((L+1) x schmidt_pitch) /
 *                   schmidt_len_host[L+1]: MPS.S (-1: bond never measured)
 *   nfs_dev         DEVICE table of nfs_cap pairs [nf, 1/nf]: the power-of-two factors taken out of the centre matrices (normC is
 *                   their product), *nfs_count_host of them written
 *   info_host[8]    {a-posteriori bound of the weighted pass, plain-pass fallbacks, weighted pass used, peak arena bytes, sum of the
 *                   bond dimensions before / after the first canonisation pass, attempts redone after a barrier time-out (see
 *                   tn_fused_timeouts: the call checks once, at its end, and redoes the row through the multi-launch forms), 0}
 * tn_compress_mps_arena_bytes: Dmax >= 0 -> what a call needs when the weighted first pass is accepted (~1.6x the measured peak at
 * L = 2048); Dmax < 0 -> the conservative bound that also covers the plain first pass on the kept input.  A call that runs out of arena
 * fails with -3 and has returned nothing: retry with the conservative size (tnac4o_amd.ops does).  nfs_cap too small: -3 as well (size
 * it (2 max_sweeps + 16) L + 64).
 * Synchronises `stream` wherever the algorithm needs a number on the host (kept ranks, convergence, overlaps).  On return the results
 * have been copied out of the arena by `stream`; the arena may be reused by the next call on the same stream.
 * Errors: -3 arena (or factor table) too small, -4 Jacobi sweeps did not converge even after QR preconditioning, -5 zero centre matrix,
 * -7 launches with in-kernel barriers gave up twice in a row. */
int64_t tn_compress_mps_arena_bytes(int64_t L, const int64_t* site_dims_host, const int64_t* mpo_dims_host, int64_t Dmax);
int tn_compress_mps(int64_t L, const double* const* sites_host, const int64_t* site_dims_host, const double* const* mpo_host,
                    const int64_t* mpo_dims_host, int hconj, int64_t Dmax, double tolS, double tolV, int max_sweeps, int graduate, int flags,
                    double* out, int64_t out_slot, int64_t* out_dims_host, double* overlap_host, double* discarded_host, double* schmidt_host,
                    int64_t schmidt_pitch, int64_t* schmidt_len_host, double* nfs_dev, int64_t nfs_cap, int64_t* nfs_count_host, double* info_host,
                    void* arena, int64_t arena_bytes, void* stream);
/* The two small reductions of the weighted first pass whose order is part of the result (both drivers call these):
 * perm_out (DEVICE int64[n]) = stable descending argsort of w (NaN first);  w_out[i] = a[i] * b[i] and sum_out[0] = their sum in a fixed order. */
int tn_argsort_desc(const double* w, int64_t n, int64_t* perm_out, void* stream);
int tn_weighted_sum(const double* a, const double* b, int64_t n, double* w_out, double* sum_out, void* stream);

/* ---- K8 driver: the beam search of search_ground_state walked in C++ (reference tnac4o.py:429-542) -------------------------
 * One lattice cell (ny, nx) as the search sees it; every pointer is a DEVICE pointer that stays valid for the call:
 *   F, dmap, rmap, q, nl, nu, pd, br   the PEPS factor of the cell as tn_peps_factor builds it (tnac4o.py:1562-1672)
 *   down, right (int64[q])             boundary index a cell state sends to the row below / the cell to its right (:1469-1489)
 *   Es (q), E1 (q x e1cols), E4 (q x e4cols)   energy tables of tnac4o._update_Eng (:1506-1558); E1 / E4 may be NULL in column / row 0
 *   left_map / up_map (int64)          Ising: state of the left / upper neighbour -> column of E1 / E4 (that neighbour's right / down
 *                                      table); NULL: the neighbour's state itself is the column
 *   A, Dl, p, Dr                       site nx of the boundary MPS above the row (rhoT[ny+1]), C-order; p must equal pd */
typedef struct tn_beam_cell {
    const double* F;
    const int32_t* dmap;
    const int32_t* rmap;
    const int64_t* down;
    const int64_t* right;
    const double* Es;
    const double* E1;
    const double* E4;
    const int64_t* left_map;
    const int64_t* up_map;
    const double* A;
    int64_t q, nl, nu, pd, br, e1cols, e4cols, Dl, p, Dr;
} tn_beam_cell;
/* tn_beam_search: rows ny = 0 .. Ny-1, sites nx = 0 .. Nx-1 (cells[ny * Nx + nx], HOST array), at most M branches, candidates cut at
 * log2 p <= max + log2_cutoff when has_cut, merge window min_dEng, B > every boundary index (radix of the row keys).  Canonical
 * order of tnac4o_amd/beam.py (ascending candidate index, lexicographic merge groups, first member of minimal energy, stable top M).
 * Results (DEVICE, room for M branches): states_out (M x Nx*Ny int16, lattice order of this rotation), energy_out, log2p_out, deg_out;
 * HOST: *nb_host branches returned, *pd_max_host largest log2 p cut or dropped, *globalmin_host smallest conditional-table flag.
 * Synchronises `stream` four times per site-step (counts).  Needs Dl * nl <= 2048 at every site (tn_env_rr_batched).
 * Errors: -3 workspace too small, -6 no candidate left. */
int64_t tn_beam_search_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t qmax, int64_t max_env, int64_t max_t1, int64_t max_w);
int tn_beam_search(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int has_cut, double log2_cutoff, double min_dEng, int64_t B,
                   int16_t* states_out, double* energy_out, double* log2p_out, int64_t* deg_out, int64_t* nb_host, double* pd_max_host,
                   double* globalmin_host, void* ws, int64_t ws_bytes, void* stream);
/* The same walk shared by a TEAM of `team` processes (one per GPU; SURVEY.md 8e-ii: the beam shards of one lattice rotation).  Every rank
 * holds the whole beam and calls tn_beam_search_team with the same arguments and its own `rank`; the conditional tables of a site-step
 * (tn_calc_pn, tnac4o.py:444-453) are evaluated for the rank's contiguous slice of the branches, [nb rank / team, nb (rank + 1) / team),
 * then `exchange` is called on every rank, in the same order, once per site-step:
 *     exchange(ctx, log2p (DEVICE, nb x q), minp (DEVICE, nb), nb, q, rank, team)
 * and must return 0 with the slices of ALL ranks in place on every rank (row b of log2p / entry b of minp belongs to the rank whose slice
 * holds b) -- e.g. one broadcast per rank over the team's communicator, enqueued on `stream` or ordered behind it.  From there on all
 * ranks run the identical deterministic cut, merge and selection: the results are those of tn_beam_search bit for bit, on every rank.
 * team = 1 (exchange may be NULL) is tn_beam_search.  Errors as tn_beam_search; -8: the exchange function returned non-zero. */
typedef int (*tn_beam_exchange_fn)(void* ctx, double* log2p, double* minp, int64_t nb, int64_t q, int rank, int team);
int tn_beam_search_team(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int has_cut, double log2_cutoff, double min_dEng, int64_t B,
                        int16_t* states_out, double* energy_out, double* log2p_out, int64_t* deg_out, int64_t* nb_host, double* pd_max_host,
                        double* globalmin_host, void* ws, int64_t ws_bytes, void* stream, int rank, int team, tn_beam_exchange_fn exchange,
                        void* exchange_ctx);

/* ---- K8s driver: the sampling walk of gibbs_sampling in C++ (reference tnac4o.py:553-650) ------------------------------------------
 * tn_gibbs_sample: rows ny = 0 .. Ny-1, sites nx = 0 .. Nx-1 over the cells of tn_beam_search (HOST array), M samples that keep their
 * slot from start to end (no cut, no merge, no selection), B > every boundary index.  uniforms (DEVICE): Nx*Ny rows of ldu >= M doubles
 * in [0, 1), row = cell in walk order, column = sample.  Per site-step: T1 = RL . A over the distinct prefixes, the samples grouped by
 * boundary row, tn_sample_pn on the groups, then states / boundary indices / energies (added up in tn_beam_search's order) of every
 * sample and the left environments of the new distinct prefixes.  A sample's result depends on its own column of uniforms only.
 * Results (DEVICE): states_out (M x Nx*Ny int16, lattice order of this rotation), energy_out (M), log2p_out (M) = log2 of the
 * probability q(x) the configuration was drawn with (the sum of log2 of the conditional probabilities of its cells).
 * HOST: *globalmin_host smallest conditional-table flag (1 when none is below), *max_groups_host (may be NULL) the largest number of
 * distinct boundary rows met.  Memory O(M (Nx + Nx*Ny) + distinct rows x environment), never O(M q); the query takes the worst case
 * (all rows distinct).  Synchronises `stream` twice per site-step (counts) and once per level of right environments.
 * Limits as tn_beam_search (q <= 32767, Dl * nl <= 2048, p == pd), tn_sample_pn's LDS bound at every cell, M^2 B^2 < 2^63.
 * Errors: -1 argument, -3 workspace too small; both before any launch. */
int64_t tn_gibbs_sample_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t qmax, int64_t max_env, int64_t max_t1, int64_t max_w);
int tn_gibbs_sample(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t B, const double* uniforms, int64_t ldu,
                    int16_t* states_out, double* energy_out, double* log2p_out, double* globalmin_host, int64_t* max_groups_host, void* ws,
                    int64_t ws_bytes, void* stream);
/* tn_gibbs_score: the same walk along GIVEN configurations -- the draw of every site-step replaced by tn_score_pn on the caller's
 * states (DEVICE, M x Nx*Ny int16, lattice order of this rotation; they are only read).  Row keys, grouping, energies (same order of
 * additions), environments and workspace layout are tn_gibbs_sample's own code, so a configuration that tn_gibbs_sample drew comes back
 * with the log2p_out and energy_out it was drawn with, bit for bit, whatever other configurations share the call.
 * Results (DEVICE): energy_out (M), log2p_out (M) = log2 q(x), the sum of the log2 conditional probabilities of the cells;
 * cell_log2p_out (may be NULL; M x Nx*Ny) those increments, every entry written.  A cell state whose table entry is not positive, or
 * that lies outside [0, q) of its cell, makes log2 q(x) = -inf (never NaN); the latter is walked on as state 0.
 * HOST: *globalmin_host, *max_groups_host (may be NULL) as tn_gibbs_sample.  Memory, synchronisations and limits as tn_gibbs_sample,
 * with tn_score_pn's LDS bound (tn_calc_pn's) at every cell.  Errors: -1 argument, -3 workspace too small; both before any launch. */
int64_t tn_gibbs_score_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t qmax, int64_t max_env, int64_t max_t1, int64_t max_w);
int tn_gibbs_score(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t B, const int16_t* states, double* energy_out,
                   double* log2p_out, double* cell_log2p_out, double* globalmin_host, int64_t* max_groups_host, void* ws, int64_t ws_bytes,
                   void* stream);

/* ---- K9: weighted histogram of the pairwise distances of a set of packed rows (no counterpart in the reference: the overlap
 * distribution of the samples, tnac4o.calculate_overlap_distribution) ---------------------------------------------------------------
 * tn_pair_hist: rows (DEVICE) = M rows of uint64 words at a stride of ldr words.  lanes16 = 0: a row is nbits bits, bit i in word i / 64
 * at position i % 64, nwords = ceil(nbits / 64), dist(a, b) = popcount(a XOR b).  lanes16 = 1: a row is nbits 16-bit lanes, four per
 * word (lane i in word i / 4 at bits 16 (i % 4) ..), nwords = ceil(nbits / 4), dist = the number of lanes that differ.  Whatever lies
 * beyond nbits in the last word is masked; the words nwords .. ldr-1 of a row are never read.  weights (DEVICE, M uint32; NULL = all 1).
 * hist_out (DEVICE, 16-byte aligned, nbits + 1 bins of two uint64: lo, hi): hist_out[d] = sum_{a<b} w_a w_b [dist(a, b) = d] as the
 * exact integer lo + 2^64 hi -- an integer function of the inputs, so bit-identical for every grid size, tile order and run (integer
 * atomics with an exact carry inside a workgroup, one slab per workgroup in ws, summed with carry).  Every bin is written; M < 2 gives
 * zeros.  ws: 16-byte aligned, tn_pair_hist_ws_bytes (which reads TN_PAIR_HIST_WGS as the call does; 0 for a shape the call refuses).
 * Asynchronous on `stream`.  Limits: M < 2^31; nbits <= 9183 (the histogram at 16 bytes per bin and 16.5 KiB of staging must fit the
 * 160 KiB of LDS).  Errors: -1 argument (M < 0, nbits out of range -- the message names the limit --, null rows / hist_out / ws,
 * ldr < nwords), -3 workspace too small; both before any launch. */
int64_t tn_pair_hist_ws_bytes(int64_t M, int64_t nbits, int lanes16);
int tn_pair_hist(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const uint32_t* weights, int lanes16, uint64_t* hist_out, void* ws,
                 int64_t ws_bytes, void* stream);

/* tn_pair_moments: second moments of the GROUPED pairwise distances (no counterpart in the reference: the overlap correlations of the
 * samples, tnac4o.calculate_overlap_correlations).  rows (DEVICE) = M rows at a stride of ldr words; a row is G groups of wpg uint64
 * words, group g = words [g wpg, (g+1) wpg); the caller pads a group with zeros to whole words (nothing is masked), the words
 * G wpg .. ldr-1 are never read.  d_g(a, b) = the distance of rows a and b within group g, tn_pair_hist's distance (lanes16 = 0:
 * popcount of the XOR, lanes16 = 1: 16-bit lanes that differ), and d_G = 1.  weights (DEVICE, M uint32; NULL = all 1); a weight above
 * wmax is read as wmax.  out (DEVICE, 16-byte aligned, (G+1) x (G+1) entries of two uint64: lo, hi), row-major and symmetric:
 * out[i][j] = sum_{a<b} w_a w_b d_i d_j as the exact integer lo + 2^64 hi, so out[G][G] = sum w_a w_b, out[g][G] = sum w_a w_b d_g.
 * An integer function of the inputs: bit-identical for every grid size, tile order and run (no atomics and no floating point; 128-bit
 * accumulators in registers, one slab per workgroup in ws, summed with carry).  Every entry is written; M < 2 gives zeros.
 * ws: 16-byte aligned, tn_pair_moments_ws_bytes (which reads TN_PAIR_MOMENTS_WGS as the call does; 0 for a shape the call refuses).
 * Asynchronous on `stream`.  Limits: 0 <= M < 2^31; 1 <= G <= 64; 1 <= wpg <= 32; ldr >= G wpg; wmax >= 1 and, with
 * dmax = (lanes16 ? 4 : 64) wpg, wmax dmax <= 2^32 - 1 -- every term is then below 2^64 and the fewer than 2^61 pairs fit two limbs.
 * Errors: -1 argument (the message names the limit), -3 workspace too small; both before any launch, nothing is written. */
int64_t tn_pair_moments_ws_bytes(int64_t M, int64_t G, int64_t wpg, int lanes16);
int tn_pair_moments(const uint64_t* rows, int64_t M, int64_t G, int64_t wpg, int64_t ldr, const uint32_t* weights, uint32_t wmax, int lanes16,
                    uint64_t* out, void* ws, int64_t ws_bytes, void* stream);

/* tn_spin_moments: for every pair of BITS of the rows, the weight of the samples in which they differ (no counterpart in the reference:
 * the sample correlations <s_i s_j> of all pairs of spins, tnac4o.calculate_sample_correlations).  rows (DEVICE) = M rows of nbits bits in
 * tn_pair_hist's layout (lanes16 = 0) at a stride of ldr words: whatever lies beyond nbits in the last word is masked, the words
 * ceil(nbits / 64) .. ldr-1 of a row are never read.  weights (DEVICE, M uint32; NULL = all 1); a weight above wmax is read as wmax, and
 * only the P = bit length of wmax weight bit-planes are processed (NULL weights: P = 1 whatever wmax).  With n = nbits and two constant
 * pseudo-bits x_a,n = 0 and x_a,n+1 = 1 appended to every row, out (DEVICE, (n+2) x (n+2) uint64 at a row stride of ldo entries) is
 * out[i][j] = sum_a w_a [x_a,i != x_a,j]: symmetric with a zero diagonal, out[i][n] = sum_a w_a x_a,i, out[i][n+1] = sum_a w_a (1 - x_a,i),
 * out[n][n+1] = sum_a w_a.  Every entry with i, j < n + 2 is written, nothing beyond column n+1 of a row; M = 0 gives zeros.  One limb
 * suffices: an entry is at most M (2^32 - 1) < 2^64 for M < 2^32, and a larger M is refused.  An integer function of the inputs:
 * bit-identical for every grid size, slicing and run (no atomics and no floating point).
 * ws: 8-byte aligned, tn_spin_moments_ws_bytes (which reads TN_SPIN_MOMENTS_WGS as the call does; 0 for a shape the call refuses): the
 * bit-major transpose of the rows, the weight planes and, with more than one workgroup, two slabs of 4096 partial sums per workgroup.
 * Asynchronous on `stream`.  Limits: 0 <= M < 2^32; 1 <= nbits <= 65534; wmax >= 1; ldr >= ceil(nbits / 64); ldo >= nbits + 2.
 * Errors: -1 argument (the message names the limit), -3 workspace too small; both before any launch, nothing is written. */
int64_t tn_spin_moments_ws_bytes(int64_t M, int64_t nbits, uint32_t wmax);
int tn_spin_moments(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const uint32_t* weights, uint32_t wmax, uint64_t* out, int64_t ldo,
                    void* ws, int64_t ws_bytes, void* stream);

/* ---- K10: cell sweeps over given configurations (no counterpart in the reference: tnac4o.relax_samples) ---------------------------
 * tn_cell_sweep: `sweeps` sweeps of block updates of whole cells over M configurations, IN PLACE in states (DEVICE, M x Nx*Ny int16,
 * lattice order of this rotation).  cells (HOST array, cells[ny * Nx + nx]): only the ENERGY part of a tn_beam_cell is read -- down,
 * right, Es, E1, E4, left_map, up_map, q, e1cols, e4cols; F, dmap, rmap, A and the MPS dimensions may be NULL / 0.  The call needs NO
 * boundary MPS and runs no contraction.  Conditional energy of cell c in state s given the states sl, su, sr, sb of its neighbours
 * (R, Bc: the right / lower cell; L = left_map ? left_map[sl] : sl, U likewise from up_map and su):
 *     e(s) = (((1.0 Es[s] + E1[s e1cols + L]) + E4[s e4cols + U]) + R.E1[sr R.e1cols + (R.left_map ? R.left_map[s] : s)])
 *                                                                 + Bc.E4[sb Bc.e4cols + (Bc.up_map ? Bc.up_map[s] : s)]
 * with these additions in this order, a term absent (not zero-added) at a lattice edge: the bits of the same expression in numpy.
 * One sweep = the cells of colour 0 (ny + nx even), then those of colour 1, every cell of a colour updated from the states as they stand
 * before that colour (one launch per colour).  sweeps = 0 updates nothing and only writes the outputs.
 * mode 0, heat bath at inverse temperature beta: w_s = exp(-beta (e(s) - min e)); the running sum c_s runs over s in an order that
 * depends on q alone, W = c_{q-1}; with t = u W the new state is the first s with c_s >= t and w_s > 0, otherwise the last s with
 * w_s > 0 (tn_sample_pn's rule).  uniforms (DEVICE): sweeps * Nx*Ny rows of ldu >= M doubles in [0, 1); the number of (sweep j, cell k
 * in walk order, sample m) is uniforms[(j Nx Ny + k) ldu + m].  mode 1, quench: the new state is the smallest s attaining min e(s) if
 * that minimum is strictly below e(current), otherwise the cell stays; uniforms must be NULL.
 * Results (DEVICE): energy_out (M) = the energy of the final configuration, added cell by cell in walk order with the additions of
 * tn_gibbs_score's energy_out (the same bits); moves_out (M int32, may be NULL) = the number of cell updates that changed the state;
 * last_moves_out (M int32, may be NULL) = the same for the final sweep only (quench: 0 = a local minimum of the cell moves).
 * A sample's result depends on its own row of states and its own column of uniforms only -- not on M, on the grid, or on how the
 * samples are cut into calls.  A state outside [0, q) of its cell is never used as an index: as a neighbour (and in energy_out) it is
 * read as 0, as the current state of a quench its energy counts as +inf.
 * ws: tn_cell_sweep_ws_bytes (0 for a shape the call refuses): the table of the cells and one flag per (cell, sample).
 * Asynchronous on `stream`, no host synchronisation; no barriers across workgroups and no atomics.  TN_CELL_SWEEP_LDS=<bytes> (read per
 * call; default 32768, at most 153600, 0: never) is the size up to which a cell's tables are staged in LDS instead of being read
 * from global memory: the same bits for every value.  Limits: q <= 32767, M < 2^31.
 * Errors: -1 argument (mode; beta <= 0 or not finite in mode 0; uniforms NULL in mode 0 or not NULL in mode 1; ldu < M; sweeps < 0; a
 * null pointer; a bad cell), -3 workspace too small; both before any launch, nothing is written. */
int64_t tn_cell_sweep_ws_bytes(int64_t Nx, int64_t Ny, int64_t M);
int tn_cell_sweep(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int16_t* states, int mode, double beta, int64_t sweeps,
                  const double* uniforms, int64_t ldu, double* energy_out, int32_t* moves_out, int32_t* last_moves_out, void* ws,
                  int64_t ws_bytes, void* stream);

/* ---- K11: isoenergetic cluster moves on pairs of configurations (no counterpart in the reference: tnac4o.exchange_clusters) --------
 * tn_cluster_exchange: one round of moves over P disjoint pairs of rows, IN PLACE.  rows (DEVICE) = M rows of nbits bits in
 * tn_pair_hist's layout (lanes16 = 0) at a stride of ldr words: the words ceil(nbits / 64) .. ldr-1 of a row are never read or written,
 * the bits beyond nbits in the last word are masked out of everything and written back unchanged.  The graph (DEVICE) is a CSR over
 * the bits: rowptr (nbits + 1 int32), cols (nnz int32); the arcs of bit i are cols[max(rowptr[i], 0) .. min(rowptr[i+1], nnz) - 1]
 * (an empty range when that is none), a neighbour outside [0, nbits) is skipped: nothing read from these arrays is used as an index
 * unchecked.  pairs (DEVICE, P x 2 int32 row indices), uniforms (DEVICE, P doubles in [0, 1)).
 * The move of pair p = (a, b): D = row_a XOR row_b (masked), cnt = popcount(D).  cnt = 0 (a == b included): nothing moves.  Otherwise
 * r = min(floor(uniforms[p] * cnt), cnt - 1) -- one IEEE multiplication and a floor, the only floating point of the call --, the seed
 * is the r-th set bit of D in ascending bit index, C = the bits reachable from the seed along listed arcs through bits of D (for a CSR
 * that lists every coupling in both directions: the seed's connected component of the subgraph induced on D; for any other CSR:
 * directed reachability), and row_a ^= C, row_b ^= C.  A uniform that is not in [0, 1) (NaN included) still gives an r in [0, cnt).
 * Results (DEVICE, P int32 each, always fully written): size_out[p] = |C| (0 when nothing moved), diff_out[p] = cnt; both are -1 for a
 * pair with an index outside [0, M), which touches nothing.
 * C is a set function of the inputs: the result is bit-identical for every grid, every schedule and every way of cutting the pairs
 * into calls.  Duty of the caller: every row appears in at most one pair (not checked: it would take a read of the device);
 * otherwise those rows are undefined, but nothing is accessed out of range.  The growth of C is bounded by construction: at most nbits
 * passes, every pass but the last adds at least one bit; no input makes it spin.
 * Asynchronous on `stream`; no global atomics, no barrier across workgroups, no host synchronisation, no workspace.  nbits <= 4096: one
 * wave per pair; above: one workgroup per pair.
 * Limits: 0 <= M < 2^31; 1 <= nbits <= 65534; ldr >= ceil(nbits / 64); 0 <= nnz < 2^31; 0 <= P < 2^31.
 * Errors: -1 argument (the message names the limit; a null operand -- cols may be NULL when nnz = 0), before any launch, nothing is
 * written.  P = 0 is a valid no-op (0, whatever the pointers). */
int tn_cluster_exchange(uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const int32_t* rowptr, const int32_t* cols, int64_t nnz,
                        const int32_t* pairs, int64_t P, const double* uniforms, int32_t* size_out, int32_t* diff_out, void* stream);

/* ---- K12: parallel tempering with isoenergetic cluster moves (no counterpart in the reference: tnac4o.temper_samples) ---------------
 * tn_temper: `rounds` rounds of heat-bath sweeps, cluster moves and temperature swaps over a population of M = R T configurations, IN
 * PLACE in states (DEVICE, M x Nx*Ny int16, tn_cell_sweep's layout; cells: the same HOST table).  Row m belongs to chain c = m / T.
 * betas (HOST, T doubles): strictly increasing, positive, finite.  The temperature assignment (DEVICE, in / out): tidx (M int32) = the
 * temperature index of every row, slot (R x T int32) = the row of chain c that sits at temperature t; slot[c][tidx[m]] == m on entry is
 * the caller's duty (a fresh run: tidx[m] = m % T, slot[c][t] = c T + t).  A swap exchanges temperature LABELS (two entries of slot,
 * two of tidx), never rows.  Round r of the call has the global index round0 + r:
 *  1. `sweeps` heat-bath sweeps of tn_cell_sweep's move (mode 0) with row m at betas[tidx[m]] (a tidx outside [0, T) is read as 0):
 *     the same conditional energy with the same additions in the same order, the same draw rule and chunked running sum, the same
 *     handling of a state outside its cell, the same TN_CELL_SWEEP_LDS staging -- one source of the move, instantiated with a
 *     per-row beta.  The number of (round r, sweep j, cell k in walk order, row m) is usweep[((r sweeps + j) Nx Ny + k) ldu + m].
 *  2. Cluster moves, only when nbits > 0: for every temperature t >= cluster_from (Tc = T - cluster_from of them) and every chain pair
 *     p = (ca, cb) of cpairs (DEVICE, rounds x Pc x 2 int32 chain indices, disjoint within a round: the caller's duty), the move of
 *     tn_cluster_exchange on the row pair (slot[ca][t], slot[cb][t]) with the uniform ucl[(r Tc + (t - cluster_from)) Pc + p]; a pair
 *     with a chain index outside [0, R) or a slot entry outside [0, M) moves nothing and reports -1, -1.  Before the moves all rows are
 *     converted to packed spin bits in the workspace, afterwards back: bitcell (DEVICE, nbits x 2 int32) = (cell k in walk order, bit
 *     j of its state) of every row position, cellbits (DEVICE, Nx*Ny x nbmax int32) = the row position of bit j of cell k's state,
 *     -1 beyond the cell's spins; a row bit is 1 - state bit (binary_states / states_from_binary).  One thread gathers each (row, word)
 *     and each (row, cell): no word is written by two threads; an entry of either table outside its range is skipped, never used
 *     as an index.  A state outside its cell is converted as 0, and a cell is written back only where the bits give another state
 *     than it was read as.  rowptr, cols, nnz: the CSR of tn_cluster_exchange.
 *  3. E[m] = the energy of every row by tn_cell_sweep's energy pass (the bits of its energy_out).
 *  4. Temperature swaps, par = (round0 + r) & 1: for every chain c and every t with t % 2 == par and t + 1 < T, a = slot[c][t],
 *     b = slot[c][t+1], D = (betas[t+1] - betas[t]) * (E[b] - E[a]) -- two subtractions and one multiplication in fp64, not contracted
 *     --; accepted iff D >= 0 or uswap[(r R + c) (T - 1) + t] < exp(D); a NaN energy never accepts.  swap_accepted[t] and
 *     swap_attempted[t] (DEVICE, T - 1 int32 each) are ADDED to, not cleared: they accumulate over calls.
 * Results (DEVICE): energy_out (M) = the energies of the final states (rounds = 0 writes nothing else).  Optional, NULL allowed:
 * energy_trace (rounds x M doubles) and tidx_trace (rounds x M int32), E and tidx after step 4 of every round; size_out and diff_out
 * (rounds x Tc x Pc int32), tn_cluster_exchange's outputs of every move in the order of ucl.
 * Degenerate forms, all valid: T = 1 (no swap; uswap and the counters may be NULL); nbits = 0 (no cluster move; the bit tables, the
 * graph, cpairs and ucl may be NULL); Pc = 0 or cluster_from = T; sweeps = 0 (usweep may be NULL); rounds = 0.
 * Determinism: the result is a function of the inputs alone.  It does not depend on the grid, and it does not depend on how the
 * rounds are cut into calls: calls with round0 advanced, the slices of usweep, cpairs, ucl and uswap that belong to their rounds, and
 * tidx, slot and the counters carried over give the same bits as one call.  With nbits = 0 the chains are independent: the result
 * of a chain does not depend on R or on which other chains share the call.
 * ws: tn_temper_ws_bytes(Nx, Ny, M, T, nbits, Pc) (0 for a shape the call refuses): the table of the cells, the betas, the packed rows,
 * the row pairs of a round.  Asynchronous on `stream`; no host synchronisation, no barrier across workgroups, no global atomics (the
 * counters are reduced in the one workgroup that serves a temperature).
 * Limits: those of tn_cell_sweep; M a multiple of T; 0 <= nbits <= 65534; 1 <= nbmax <= 15; 0 <= cluster_from <= T; 0 <= 2 Pc <= R.
 * Errors: -1 argument (the message names the limit), -3 workspace too small; both before any launch, nothing is written. */
int64_t tn_temper_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t T, int64_t nbits, int64_t Pc);
int tn_temper(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t T, const double* betas, int16_t* states, int32_t* tidx,
              int32_t* slot, int64_t round0, int64_t rounds, int64_t sweeps, const double* usweep, int64_t ldu, int64_t nbits, int64_t nbmax,
              const int32_t* cellbits, const int32_t* bitcell, const int32_t* rowptr, const int32_t* cols, int64_t nnz, int64_t cluster_from,
              const int32_t* cpairs, int64_t Pc, const double* ucl, const double* uswap, double* energy_out, int32_t* swap_accepted,
              int32_t* swap_attempted, double* energy_trace, int32_t* tidx_trace, int32_t* size_out, int32_t* diff_out, void* ws, int64_t ws_bytes,
              void* stream);

/* ---- K13: population annealing (no counterpart in the reference: tnac4o.anneal_population) -----------------------------------------
 * tn_anneal: a population of M configurations is taken along the schedule betas (HOST, K doubles), IN PLACE in states (DEVICE,
 * M x Nx*Ny int16, tn_cell_sweep's layout; cells: the same HOST table) and family (DEVICE, M int32, in / out: a label that travels with
 * its row; a fresh run: family[m] = m).  betas[0] >= 0 is the inverse temperature whose law the incoming rows sample -- no sweep is made
 * at it --; betas[1 ..] are strictly increasing above it and finite.  On entry E[m] = the energy of every row by tn_cell_sweep's energy
 * pass (the bits of its energy_out).  Step s = 1 .. K-1, db = betas[s] - betas[s-1] (one subtraction on the host):
 *  1. Emin = the smallest E[m] that is no NaN (NaN when every one is)                                          -> emin_out[s-1].
 *  2. w_m = exp(-(db * (E[m] - Emin))): one subtraction, one multiplication, one exp in fp64, not contracted; a w_m that is NaN counts
 *     as 0.
 *  3. Running sums in a fixed SEQUENTIAL order that depends on M alone.  Rows are cut into tiles of 256, a tile into four groups of 64:
 *     inside a group g_i = g_{i-1} + w_i, row after row (g_{-1} = 0); inside a tile the group bases b_0 = 0, b_{k+1} = b_k + (the last
 *     g of group k) and l_m = b_k + g_i (group 0: l_m = g_i); across tiles t_0 = 0, t_{k+1} = t_k + (the last l of tile k), tile after
 *     tile, and C_m = t_k + l_m.  W = t after the last tile                                                   -> wsum_out[s-1].
 *     The sum of w_m^2 is added in the same order (group after group inside a tile)                            -> w2sum_out[s-1].
 *     Every partial sum is a sequential sum of non-negative numbers on top of the one before it, so C is non-decreasing in m.
 *  4. Systematic resampling with u = ures[s-1] (DEVICE, K-1 doubles in [0, 1)): O_{-1} = 0, O_{M-1} = M and for m < M-1
 *     O_m = min(M, max(O_{m-1}, floor(((C_m / W) * (double)M) + u))): one division, one multiplication, one addition, one floor in fp64,
 *     a negative or NaN value read as 0.  (C is non-decreasing and each of the four operations is monotone, so the maximum is attained
 *     by its second operand.)  Row m gets n_m = O_m - O_{m-1} copies; survivors_out[s-1] = the number of rows with n_m >= 1.  W zero
 *     or not finite (every weight zero or NaN; an infinite sum): the step is the identity, O_m = m + 1.
 *  5. parent[j] = the m with O_{m-1} <= j < O_m, by binary search over O once per row; states'[j] = states[parent[j]],
 *     family'[j] = family[parent[j]].  A row is copied in pieces of the widest power of two, at most 16 bytes, that divides 2 Nx Ny
 *     and the addresses of both copies (an odd number of cells: element by element).  The second copy of the rows lives in ws; when
 *     the call returns, states and family hold the result in stream order.  The search keeps inside [0, M) whatever O holds, and a
 *     parent is checked again before it indexes a row.
 *  6. `sweeps` heat-bath sweeps of tn_cell_sweep's move (mode 0) at betas[s]: the same kernels.  The number of (step s, sweep j, cell k
 *     in walk order, row m) is usweep[(((s-1) sweeps + j) Nx Ny + k) ldu + m] (DEVICE, ldu >= M).
 *  7. E[m] = the energy of every row by tn_cell_sweep's energy pass                                            -> energy_out (M).
 * Optional, NULL allowed: energy_trace ((K-1) x M doubles), E after step 7 of every step; parent_trace ((K-1) x M int32), parent.
 * The estimate the outputs carry: ln Z(betas[s]) / Z(betas[s-1]) ~ ln(W / M) - db Emin.
 * Degenerate forms, all valid: K = 1 (energy_out only; ures and the four per-step outputs may be NULL); sweeps = 0 (usweep may be
 * NULL); M = 1.
 * Determinism: the result is a function of the inputs alone -- not of the grid, and not of how the schedule is cut into calls: a call on
 * betas[a .. b] followed by one on betas[b .. c] with the slices of ures and usweep that belong to their steps, states and family
 * carried over, gives the bits of one call on betas[a .. c].
 * ws: tn_anneal_ws_bytes(Nx, Ny, M) (0 for a shape the call refuses): the table of the cells, the second copy of rows and families,
 * l, O, parent and three numbers per tile.  Asynchronous on `stream`; no host synchronisation, no barrier across workgroups, no
 * kernel that waits for another workgroup, no global atomics.
 * Limits: those of tn_cell_sweep (q <= 32767, M < 2^31); 1 <= K <= 2^31.
 * Errors: -1 argument (the message names the limit: betas[0] negative, betas not strictly increasing or not finite, ldu < M, a null
 * pointer, a bad cell), -3 workspace too small; both before any launch, nothing is written. */
int64_t tn_anneal_ws_bytes(int64_t Nx, int64_t Ny, int64_t M);
int tn_anneal(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t K, const double* betas, int16_t* states, int32_t* family,
              int64_t sweeps, const double* usweep, int64_t ldu, const double* ures, double* energy_out, double* emin_out, double* wsum_out,
              double* w2sum_out, int32_t* survivors_out, double* energy_trace, int32_t* parent_trace, void* ws, int64_t ws_bytes, void* stream);

/* ---- K14: uniform numbers from a counter-based generator (no counterpart in the reference: the seed= of the Monte Carlo calls) ------
 * tn_uniforms: out[r ld + c] = U(seed, stream0 + r, first + c) for r < rows, c < cols (DEVICE, doubles, ld >= cols; the elements
 * c >= cols of a row are never touched).  U is a pure function of three unsigned 64-bit numbers:
 *   Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85;
 *   one of the ten rounds maps (c0, c1, c2, c3), (k0, k1) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the key is
 *   bumped by its increments.
 *   U(seed, stream, i): b = i >> 1, x = philox(counter (b lo32, b hi32, stream lo32, stream hi32), key (seed lo32, seed hi32)), h = i & 1,
 *   v = x[2h] + 2^32 x[2h+1], U = (v >> 11) 2^-53: both steps exact in fp64, U in [0, 1 - 2^-53].
 * One Philox block is two numbers, 16 bytes: a block that lies inside the row at an address that is a multiple of 16 is stored with one
 * 16-byte store, every other number (a row that starts at an odd `first`, an odd cols, an odd ld or base) with an 8-byte store; the
 * bits do not depend on which.  The result is a function of the arguments alone, not of the grid; a fill of [first, first + n) equals
 * the fills of [first, first + a) and [first + a, first + n).
 * rows = 0 or cols = 0 is a valid no-op.  Asynchronous on `stream`: one launch, no workspace, no atomics, no barrier across workgroups,
 * no host synchronisation.
 * Errors: -1 before any launch, the message names the limit: rows or cols negative, ld < cols, rows ld >= 2^62, first + cols above 2^64,
 * stream0 + rows above 2^64, and (rows, cols > 0) out null or not aligned to 8 bytes. */
int tn_uniforms(uint64_t seed, uint64_t stream0, uint64_t first, int64_t rows, int64_t cols, double* out, int64_t ld, void* stream);

/* ---- K15: droplets of configurations relative to a reference (the search of the reference does this per branch, on the host; for
 * stored states there is no counterpart: tnac4o.calculate_droplets) ------------------------------------------------------------------
 * tn_droplets: rows (DEVICE) = M rows of nbits bits in tn_cluster_exchange's layout at a stride of ldr words, ref (DEVICE) = one such
 * row of ceil(nbits / 64) words; neither is written.  Words behind a row and bits beyond nbits (of rows and of ref) are ignored.  The
 * graph (DEVICE) is tn_cluster_exchange's CSR, rowptr (nbits + 1 int32), cols (nnz int32), with one coupling per arc, vals (nnz
 * doubles), and the fields, field (nbits doubles, or NULL: none): the arcs of bit i are e = max(rowptr[i], 0) .. min(rowptr[i+1], nnz) - 1
 * (an empty range when that is none), an arc to a neighbour outside [0, nbits) is skipped for growth and for energy: nothing read from
 * these arrays or from rows is used as an index unchecked.
 * For row m: D = row XOR ref (masked).  Its droplets are the sets C reachable along listed arcs through bits of D -- for a CSR that
 * lists every coupling in both directions: the connected components of the subgraph induced on D; a one-way arc is followed as it is
 * given, for growth and for energy --, grown one after the other, each from the lowest bit of D that no earlier droplet holds (its
 * root): droplets are numbered 0, 1, ... by ascending root.  A bit that an earlier droplet holds is not taken again (one-way arcs can
 * lead into one): the droplets are a partition of D for every CSR.  With g_i = 2 ref_i - 1 the excitation energy of C is
 *   dE_C = 2 (sum over i in C of (-field[i] g_i + sum over the arcs e = (i -> j) of i with j not in D of -vals[e] g_i g_j)),
 * which for a symmetric CSR of an Ising energy E = sum_{i<j} J_ij s_i s_j + sum_i h_i s_i is E(ref with C flipped) - E(ref): an arc that
 * leaves C ends outside D, because a neighbour in D belongs to C.  The same walk of the arcs grows C and adds the terms.
 * Results (DEVICE), per row m, always fully written: count_out[m] = the number of droplets (all of them, also beyond K), diff_out[m] =
 * popcount(D), largest_out[m] = the largest size (0: none), de_total_out[m] = dE of droplet 0 + dE of droplet 1 + ..., added in this
 * order from 0.0, over ALL droplets (int32, int32, int32, double).  Per row and slot k < K (root_out, size_out int32, de_out double,
 * M x K each, NULL allowed when K = 0): the first min(count, K) droplets in root order; the slots behind them hold -1, 0, 0.0.
 * size_hist (nbits + 1 int64): size_hist[s] is INCREASED by the number of droplets of size s over all rows of the call (all of them,
 * also beyond K), with integer atomics; the caller zeroes it, calls over slices of the rows accumulate.  labels (M x nbits int32 at a
 * stride of ldl, or NULL): labels[m ldl + i] = the number of the droplet of row m that holds bit i, -1 where the row equals the
 * reference; entries i >= nbits of a row are never touched.
 * Floating point: every term is a coupling or a field times +-1, so for exactly summable values (integers, say) every energy is exact.
 * Otherwise: the frontier of a growth pass is a level of the breadth-first search from the root; a thread adds the terms of its words'
 * bits in the order (level, bit ascending, field, arcs as listed), from 0.0; the threads' sums are added in a fixed tree.  The result
 * is a function of the inputs alone: the same bits for every grid, every schedule and every way of cutting the rows into calls.  An
 * energy that is zero is +0.0.
 * Asynchronous on `stream`; no barrier across workgroups, no host synchronisation, no workspace; the only global atomics are the integer
 * additions to size_hist.  nbits <= 4096: one wave per row, no workgroup barrier; above: one workgroup per row.  The growth is bounded
 * by construction (at most nbits + 1 passes per droplet, at most popcount(D) droplets); no input makes it spin.
 * Limits: 0 <= M < 2^31; 1 <= nbits <= 65534; ldr >= ceil(nbits / 64); 0 <= nnz < 2^31; 0 <= K < 2^31, M K < 2^60; with labels:
 * ldl >= nbits, M ldl < 2^60.
 * Errors: -1 argument (the message names the limit; a null operand -- cols and vals may be NULL when nnz = 0, the slot arrays when
 * K = 0, field and labels always), before any launch, nothing is written.  M = 0 is a valid no-op (0, whatever the pointers). */
int tn_droplets(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const uint64_t* ref, const int32_t* rowptr, const int32_t* cols,
                const double* vals, int64_t nnz, const double* field, int64_t K, int32_t* count_out, int32_t* diff_out, int32_t* largest_out,
                double* de_total_out, int32_t* root_out, int32_t* size_out, double* de_out, int64_t* size_hist, int32_t* labels, int64_t ldl,
                void* stream);

/* ---- K16: single-linkage clusters of configurations (no counterpart in the reference: tnac4o.calculate_state_linkage) ---------------
 * Rows.  rows (DEVICE) = M rows in tn_pair_hist's layout at a stride of ldr words, in one of two forms.  lanes16 = 0: nbits bits per
 * row, d(a, b) = popcount(a XOR b).  lanes16 = 1: nbits 16-bit lanes per row, d = the number of lanes that differ.  Whatever lies beyond
 * nbits in the last word is masked.  Words nwords .. ldr-1 are never read (nwords = ceil(nbits / 64), lanes16: ceil(nbits / 4)).
 * Fold.  With fold = 1 (bits only) the distance is d'(a, b) = min(d, nbits - d).  A state and its global spin flip are then the same
 * point.
 * Edge order.  Edges are ordered by the strict total order key(a, b) = (d(a, b), min(a, b), max(a, b)), compared lexicographically.
 * Tree.  The tree is the unique minimum spanning tree of the complete graph on the M rows under that order.  Kruskal, Prim and Boruvka
 * all return it, so the result does not depend on the algorithm, grid or run.  It has M - 1 edges, reported in ascending key order:
 * edge e joins the rows edge_lo[e] < edge_hi[e] at distance edge_dist[e] (DEVICE, int32, M - 1 each; may be NULL when M < 2).
 * Nearest other row.  For row a it is the b != a that minimises (d(a, b), b): nn_index[a] = b, nn_dist[a] = d(a, b) (DEVICE, int32, M
 * each; both NULL or both given).  M = 1 writes nn_index = nn_dist = -1.  M <= 1 writes no edge.  M = 0 writes nothing but
 * rounds_out = 0.
 * rounds_out (DEVICE, one int32): the number of Boruvka rounds that did work, 1 <= rounds <= ceil(log2 M) for M >= 2, else 0; a
 * diagnostic (it does not depend on the grid either).
 * Asynchronous on `stream`, the host never synchronises: a fixed ceil(log2 M) rounds of ordinary launches are queued (a round at least
 * halves the components); once a device counter says one component is left the kernels of a round return at once.  No barrier across
 * workgroups and no spinning; integers only; the only atomics are 64-bit atomicMin on the best candidate of a row and on the best
 * edge of a component (the key d:16 | lo:24 | hi:24), and the counter of the edges.  The pair pass of a round walks the upper triangle
 * of the pair matrix in 64 x 64 blocks, as tn_pair_hist does, and offers every distance to both of its rows; TN_LINKAGE_WGS overrides
 * its grid as TN_PAIR_HIST_WGS does (read per call, and by tn_state_linkage_ws_bytes as by the call).
 * ws: 256-byte aligned, tn_state_linkage_ws_bytes (0 for a shape the call refuses and for M < 2, where ws may be NULL).
 * Limits: 0 <= M <= 2^24; 1 <= nbits <= 65534; ldr >= nwords; fold only with lanes16 = 0.
 * Errors: -1 argument (the message names the limit; a null operand; one of nn_index, nn_dist without the other), -3 workspace too small;
 * both before any launch, nothing is written. */
int64_t tn_state_linkage_ws_bytes(int64_t M, int64_t nbits, int lanes16);
int tn_state_linkage(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, int lanes16, int fold, int32_t* nn_index, int32_t* nn_dist,
                     int32_t* edge_lo, int32_t* edge_hi, int32_t* edge_dist, int32_t* rounds_out, void* ws, int64_t ws_bytes, void* stream);

/* ---- K17: exact heat bath and quench of whole lattice lines (no counterpart in the reference: tnac4o.relax_lines) -------------------
 * tn_line_sweep: `sweeps` sweeps of updates of whole rows and columns over M configurations, IN PLACE in states (DEVICE, M x Nx*Ny
 * int16, lattice order of this rotation).  cells, states, energy_out, the treatment of a state outside [0, q) as a neighbour and the
 * independence of a sample's result from M, the grid and the cut into calls are tn_cell_sweep's (K10).
 * The chain.  With the rows above and below given, row ny is a chain of cells x = 0 .. Nx-1 (B: the cell below; U from up_map and the
 * state above as in K10):
 *     side energy  a_x(s) = ((1.0 Es[s] + E4_x[s e4cols + U]) + B.E4[sb B.e4cols + (B.up_map ? B.up_map[s] : s)])
 *     coupling     E1_x[s_x e1cols + r_{x-1}(s_{x-1})],  r_{x-1}(s') = left_map_x ? left_map_x[s'] : s'
 * with these additions in this order, a term absent at a lattice edge.  A column is the same with (E1, left_map, nx) and (E4, up_map,
 * ny) exchanged.  A row pass updates the rows of even ny, then those of odd ny (one launch per parity); a column pass the columns of
 * even nx, then odd.  lines = 0: a sweep is one row pass (P = 1); 1: one column pass (P = 1); 2: a row pass, then a column pass (P = 2).
 * mode 0, heat bath at beta: the whole line is drawn from its conditional Boltzmann law by forward filtering and backward sampling in
 * the LINEAR domain: lambda_0(s) = w_0(s), lambda_x(s) = w_x(s) sum_r F_x[r] T_x[s, r] with w_x(s) = exp(-beta (a_x(s) - min_s a_x)),
 * T_x[s, r] = exp(-beta (E1_x[s, r] - min E1_x)) and the column messages F_x[r] = (sum of lambda_{x-1}(s') over r_{x-1}(s') = r) /
 * max_s lambda_{x-1}; cell Nx-1 is drawn from the weights lambda_{Nx-1}(s), then x = Nx-2 .. 0 from lambda_x(s) T_{x+1}[s_{x+1}, r_x(s)],
 * every draw by K10's rule (running sum in ascending s, t = u W, the first s with c_s >= t and w_s > 0, else the last s with w_s > 0).
 * uniforms (DEVICE): sweeps * P * Nx*Ny rows of ldu >= M doubles in [0, 1); the number of (sweep j, pass p, cell k, sample m) is
 * uniforms[((j P + p) Nx Ny + k) ldu + m].  The sums of the messages and of the running sum are not the bits of a host summation: a
 * draw closer to a boundary of the running sum than the rounding of these sums may differ from a reference.
 * Range guard (mode 0, sweeps > 0): beta (max - min) <= 300 for every chain table of the directions in use (E1 for rows, E4 for
 * columns).  Under it the largest lambda of a cell is at least 1e-131 after normalisation and nothing that underflows matters.  The
 * guard needs the tables, which live on the device: in mode 0 the call reduces their ranges, reads them back and WAITS for the stream
 * once, before any state is touched.  A call beyond the bound returns -1 with a message naming the range guard; it has then written
 * the head of ws (the table of the cells and the ranges) and nothing else.
 * mode 1, quench: the same recursion in (min, +): Lambda_0(s) = a_0(s), Lambda_x(s) = a_x(s) + min_r (mu_x[r] + E1_x[s, r]), mu_x[r] =
 * min of Lambda_{x-1}(s') over r_{x-1}(s') = r, E* = min_s Lambda_{Nx-1}(s).  The energy of the line as it stands is c_0 = a_0(s_0),
 * c_x = a_x(s_x) + (c_{x-1} + E1_x[s_x, r]), +inf when one of its cells holds a state outside its range.  The line moves only if
 * E* < c_{Nx-1} strictly, and then to the minimiser that is smallest in the lexicographic order of (s_{Nx-1}, .., s_0): from the far end,
 * the smallest state attaining min_s (Lambda_x(s) + E1_{x+1}[s_{x+1}, r_x(s)]).  No exponentials, no guard, the bits of the same
 * expressions in numpy; uniforms must be NULL; asynchronous, no host synchronisation.
 * Results (DEVICE): energy_out (M) as K10's (the same bits); moves_out / last_moves_out (M int32, may be NULL) = the number of CELLS
 * whose state changed over the call / in its last sweep.  sweeps = 0 updates nothing and only writes the outputs.
 * ws: tn_line_sweep_ws_bytes (0 for a shape the call refuses): the table of the cells, one flag per (cell, sample), the ranges, a
 * 32 MiB arena of transfer tables and a 16 MiB scratch of the workgroups that cannot keep their messages in LDS -- only the flags
 * depend on M.  T_x is computed once per call into the arena (transposed) for the tables that fit TN_LINE_SWEEP_TABLES bytes (read
 * per call; default and at most 33554432, 0: none); every other table evaluates the same expression where it is read: the same bits.
 * No barriers across workgroups and no atomics.  Limits: q <= 32767, M < 2^31, Nx Ny < 2^26, and q_max + the chain-table columns of
 * one line <= 2^21 (the vectors of one sample).
 * Errors: -1 argument (mode; lines; beta <= 0 or not finite in mode 0; uniforms NULL in mode 0 or not NULL in mode 1; ldu < M;
 * sweeps < 0; M; a null pointer; a bad cell; the range guard), -3 workspace too small; all but the range guard before any launch,
 * nothing is written. */
int64_t tn_line_sweep_ws_bytes(int64_t Nx, int64_t Ny, int64_t M);
int tn_line_sweep(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int16_t* states, int mode, int lines, double beta, int64_t sweeps,
                  const double* uniforms, int64_t ldu, double* energy_out, int32_t* moves_out, int32_t* last_moves_out, void* ws,
                  int64_t ws_bytes, void* stream);

/* ---- K18: per-row sums of the pairwise distances of a set of packed rows (no counterpart in the reference: the jackknife errors of the
 * overlap moments, tnac4o.calculate_overlap_errors) -------------------------------------------------------------------------------------
 * tn_pair_rowsums: the pair matrix of tn_pair_hist (K9) reduced per ROW instead of per distance bin.  Rows, lanes16, the masking of the
 * last word, ldr and weights (DEVICE, M uint32; NULL = all 1) are exactly those of tn_pair_hist.  out (DEVICE, 16-byte aligned, M x 6
 * entries of two uint64: lo, hi), row-major.  For row a, with d = dist(a, b) and the sum running over every b != a in 0 .. M-1:
 *     out[a][0] = sum w_b,   out[a][k] = sum w_b d^k for k = 1 .. 4,   out[a][5] = sum w_b |nbits - 2 d|,
 * each entry the exact integer lo + 2^64 hi.  The row's own weight does not enter its sums; a row of weight 0 still gets its sums.  A
 * row b != a with the same content has d = 0: it enters entries 0 and 5 only.  Every entry of every row is written: M = 1 gives six
 * zeros, M = 0 writes nothing.  An integer function of the inputs: bit-identical for every grid, split and run (no atomics and no
 * floating point: the full square of the pair matrix in 64 x 64 tiles, the sums of a row in registers, the 16 threads of a row added
 * with carry, one slab per segment of the columns in ws, summed with carry).
 * ws: 16-byte aligned, tn_pair_rowsums_ws_bytes (which reads TN_PAIR_ROWSUMS_WGS as the call does; 0 for a shape the call refuses).
 * Asynchronous on `stream`.  Limits: 0 <= M < 2^31 and 1 <= nbits <= 65535: then w d^2 < 2^64 and w d^4 < 2^96, so a row's sum stays
 * below 2^127.  Errors: -1 argument (the message names the limit), -3 workspace too small; both before any launch, nothing is written. */
int64_t tn_pair_rowsums_ws_bytes(int64_t M, int64_t nbits, int lanes16);
int tn_pair_rowsums(const uint64_t* rows, int64_t M, int64_t nbits, int64_t ldr, const uint32_t* weights, int lanes16, uint64_t* out, void* ws,
                    int64_t ws_bytes, void* stream);

/* ---- K19: one measurement of the overlap histograms of a tempering ladder (no counterpart in the reference: the measure= of
 * tnac4o.temper_samples) -----------------------------------------------------------------------------------------------------------------
 * tn_ladder_measure: ADDS one measurement to accumulators on the device.  states (DEVICE, M x Nx*Ny int16), slot (DEVICE, R x T int32,
 * R = M / T), cells (HOST) and bitcell (DEVICE, nbits x 2 int32) are those of tn_temper (K12) and are only read: the rows at temperature t
 * are slot[c][t], c = 0 .. R-1.  Every row is converted to nbits packed spin bits by tn_temper's own kernel (row bit = 1 - state bit, a
 * state outside its cell reads as 0, an entry of bitcell out of range leaves the bit 0).  For every t and every counted chain pair
 * ca < cb, with d = popcount(row_a XOR row_b):  spin_hist[t (nbits + 1) + d] += 1  (DEVICE, T x (nbits + 1) uint64).  With links (DEVICE,
 * nlinks x 2 int32 row positions) and link_hist (DEVICE, T x (nlinks + 1) uint64) the link row of a configuration has bit l = row bit
 * links[l][0] XOR row bit links[l][1] -- 0 when either entry lies outside [0, nbits) --, and with d_l the distance of two link rows
 * link_hist[t (nlinks + 1) + d_l] += 1 over the same pairs; link_hist NULL or nlinks = 0: no link overlap.
 * split = 0: every pair ca < cb is counted.  0 < split <= R: only the pairs with ca < split <= cb (two sets of chains, overlaps between
 * the sets); split = R counts nothing.  A slot entry outside [0, M) takes all pairs of that chain at that temperature out of the count.
 * energy (DEVICE, M doubles: tn_temper's energy_out) and esums (DEVICE, T x 3 doubles), both or neither used: one thread per
 * temperature forms s1 = sum E[slot[c][t]] and s2 = sum E^2 over c = 0 .. R-1 in ascending c (fp64, no contraction; a slot entry out
 * of range is skipped), then esums[3t] += 1, esums[3t+1] += s1, esums[3t+2] += s2.
 * Valid degenerate forms: R = 1, split = R and M = 0 count no pair; link_hist = NULL; energy or esums = NULL.  Only spin_hist, link_hist
 * and esums are written, inside their extents.  The counts are an integer function of the inputs: bit-identical for every grid and
 * every split of the pairs over workgroups (uint32 histograms in LDS with integer atomics, one slab per workgroup in ws, a reduce kernel
 * that adds the slabs into the 64-bit accumulators; TN_LADDER_WGS = the workgroups that share the pairs of one temperature, default
 * max(1, 1024 / T), never more than there are 16 x 16 tiles of pairs).  No floating-point atomics, no barrier across workgroups, no host
 * synchronisation.  ws: tn_ladder_measure_ws_bytes (which reads TN_LADDER_WGS as the call does; 0 for a shape the call refuses): the table
 * of the cells, the packed rows and link rows, the slabs.  Asynchronous on `stream`.
 * Limits: 0 <= M < 2^31, M a multiple of T >= 1, R <= 65536 (R (R - 1) / 2 < 2^32: no bin of a workgroup can wrap); 1 <= nbits <= 38815
 * and 0 <= nlinks <= 38815 (the histogram at 4 bytes per bin and 8576 bytes of staging must fit the 160 KiB of LDS); 0 <= split <= R;
 * cells as tn_cell_sweep's.  Errors: -1 argument (the message names the limit), -3 workspace too small; both before any launch, nothing
 * is written. */
int64_t tn_ladder_measure_ws_bytes(int64_t Nx, int64_t Ny, int64_t M, int64_t T, int64_t nbits, int64_t nlinks);
int tn_ladder_measure(int64_t Nx, int64_t Ny, const tn_beam_cell* cells, int64_t M, int64_t T, const int16_t* states, const int32_t* slot,
                      int64_t nbits, const int32_t* bitcell, const int32_t* links, int64_t nlinks, int64_t split, const double* energy,
                      uint64_t* spin_hist, uint64_t* link_hist, double* esums, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
