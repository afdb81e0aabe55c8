/*
 * nmgp_hip.h -- C ABI of libnmgp_hip.so, the MI355X (gfx950) kernels of the DSVI hot path of
 * Collaborative Nonstationary Multivariate GP inference (reference: code/nmgp_dsvi.py).
 *
 * Conventions:
 *   - plain pointers + sizes, no torch types; every buffer is caller-owned device memory;
 *   - every call only ENQUEUES work on the given hipStream_t (no implicit device sync, no
 *     allocation), so a caller may capture any sequence of calls into a hipGraph;
 *   - return 0 on success, <0 = index of the offending argument (argument error),
 *     NMGP_ERR_LAUNCH on a launch failure.  Numerical failures (non-PD matrix) are reported
 *     LAPACK-style through a device `info` array: info[b] = first failing column (1-based).
 *   - matrices are row-major; T = double (_f64) or float (_f32).
 *
 * Each entry point cites the reference interface it replaces.
 */
#ifndef NMGP_HIP_H
#define NMGP_HIP_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMGP_OK 0
#define NMGP_ERR_LAUNCH (-1000)

/* ------------------------------------------------------------------ library info */
int nmgp_version(void);

/* Device status word.  Kernels that hand data between workgroups of one launch wait on peers with
 * BOUNDED spins (a lost peer must not hang the GPU); a spin that gives up sets one of these bits
 * instead of failing silently.  nmgp_device_status() ORs the words of every kernel file into *out
 * (host memory) and clears them when `clear` != 0.  It synchronises with the device: call it at a
 * point where the caller syncs anyway (the Python layer does so with the Cholesky `info` check).
 * Any nonzero bit means the results of the launches since the last check are not trustworthy.     */
#define NMGP_STATUS_CHOL_SPIN  1u   /* two-role Cholesky: the inverse role lost its factor role    */
#define NMGP_STATUS_GEMM_SPIN  2u   /* grouped GEMM: a cooperative split-K chunk lost a peer       */
#define NMGP_STATUS_POTRF_SPIN 4u   /* blocked potrf step: the panel publisher never arrived       */
int nmgp_device_status(uint32_t* out, int clear);
/* sizeof of the descriptor structs below (host code checks its own layout against these) */
int64_t nmgp_sizeof_gemm_desc(void);
int64_t nmgp_sizeof_pairwise_desc(void);
int64_t nmgp_sizeof_pairwise_bwd_desc(void);
int64_t nmgp_sizeof_dsvi_args(void);
int64_t nmgp_sizeof_pair_desc(void);
int64_t nmgp_sizeof_chol_tp_args(void);

/* ------------------------------------------------------------------ grouped GEMM (MFMA)
 * C(i,j) = alpha * sum_k op(A)(i,k) * s(k) * op(B)(k,j) + beta*C(i,j) + gamma*rs(i)*E(i,j)
 *          (+ diag_add on i==j)
 * Operands are addressed through strides, which covers transposes, k-concatenated blocks
 * (A(i,k) = A[i*sA_i + (k%kbA)*sA_k + (k/kbA)*sA_kb]) and row / k ranges taken at run time from
 * a device segment table (row_seg / k_seg >= 0: rows or k in [seg[s], seg[s+1])).
 * Replaces every torch.matmul / torch.solve(...)-product in code/utils.py:117-157 and
 * code/nmgp_dsvi.py:172-177 (Sigma = tril(S) tril(S)^T).                                  */
enum {
  NMGP_A_LOWER = 1,      /* op(A)(i,k) = 0 for k > i     */
  NMGP_A_UPPER = 2,      /* op(A)(i,k) = 0 for k < i     */
  NMGP_B_LOWER = 4,      /* op(B)(k,j) = 0 for j > k     */
  NMGP_B_UPPER = 8,      /* op(B)(k,j) = 0 for j < k     */
  NMGP_OUT_LOWER = 16,   /* store only j <= i            */
  NMGP_OUT_TRIL = 32,    /* store j <= i, zero for j > i */
  NMGP_KSCALE = 64,      /* multiply by s(k) = kscale[k] */
  NMGP_EPI = 128,        /* + gamma * rs(i) * E(i,j)     */
  NMGP_EPI_E_LOWER = 256,/* E(i,j) = 0 for j > i         */
  NMGP_DIAG_ADD = 512,   /* + diag_add on i == j         */
  NMGP_EPI_RS_NEG = 1024,/* rs(i) taken with a minus sign */
  NMGP_LAT_COLPACK = 2048,/* latency kernel only (set by the host): a B_LOWER / B_UPPER problem with n == k ==
                          * 32 T, T <= 8, no other mask: tiles_n counts column-tile GROUPS -- {0}, {g, T-g}
                          * for g = 1..(T-1)/2 and {T/2} for even T (B_UPPER mirrored) -- whose k panels add up
                          * to <= 8, one group per workgroup                                                  */
};

typedef struct nmgp_gemm_desc {
  const void* A; const void* B; void* C;
  const void* kscale; const void* epi_E; const void* epi_rs;
  int64_t sA_i, sA_k, sA_kb;
  int64_t sB_k, sB_j, sB_kb;
  int64_t sC_i, sC_j;
  int64_t sE_i, sE_j;
  int32_t m, n, k, kbA, kbB, flags, row_seg, k_seg;
  double alpha, beta, gamma, diag_add;
  int32_t tiles_m, tiles_n, tile_start;
  int32_t seg_span;      /* row_seg / k_seg cover seg[s] .. seg[s + max(seg_span,1)] */
  /* split-K: ksplit > 1 cuts the k range into ksplit chunks; each chunk's 64x64 partial goes to
   * ws (tiles_m*tiles_n*ksplit*4096 elements) and the last-arriving chunk of a tile (counter in
   * `counters`, tiles_m*tiles_n zero-initialised int32, reset by the kernel) sums them in chunk
   * order -- deterministic -- and applies the epilogue.  tiles = tiles_m*tiles_n*ksplit.        */
  int32_t ksplit, pad2_;
  void* ws;
  int32_t* counters;
  /* batch (single-problem launches only): problem b uses A + b*sA_b, B + b*sB_b, C + b*sC_b;
   * batch <= 1 means one problem.  Split-K and batch are exclusive.                           */
  int64_t sA_b, sB_b, sC_b;
  int32_t batch, pad3_;
} nmgp_gemm_desc;

/* d_desc: device array of nprob descriptors (tiles_m/tiles_n/tile_start filled by the host,
 * tiles = ceil(m/64)*ceil(n/64)); total_tiles = sum of tiles; d_seg may be NULL if unused.  */
int nmgp_gemm_grouped_f64(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles,
                          const int32_t* d_seg, hipStream_t stream);
int nmgp_gemm_grouped_f32(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles,
                          const int32_t* d_seg, hipStream_t stream);
/* The same sized on device for this minibatch: a one-workgroup plan kernel turns the segment table
 * into per-problem first tiles (row-segmented problems get ceil(segment rows / 64) row tiles instead
 * of the static tiles_m), written to plan[0..nprob] (caller buffer of nprob + 1 int32), then `grid`
 * workgroups (<= total_tiles; <= 0: total_tiles) stride over the planned tiles.  Same results as the
 * static launch; no workgroups are dispatched for rows other outputs own (HCP: D=50 segments).   */
int nmgp_gemm_grouped_dyn_f64(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles, const int32_t* d_seg,
                              int32_t* plan, int grid, hipStream_t stream);
int nmgp_gemm_grouped_dyn_f32(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles, const int32_t* d_seg,
                              int32_t* plan, int grid, hipStream_t stream);
/* The same descriptors through the latency-oriented kernel (gemm_lat.hip) for groups of short-k
 * problems: 32x32 output tiles (tiles_m = ceil(m/32), tiles_n = ceil(n/32), tile_start in those
 * units, ksplit ignored), the k range of a tile split over the waves of its workgroup, operands
 * loaded straight into MFMA registers.  Requirements: non-negative strides, kbA / kbB either >= k
 * or a multiple of 64, operand extents below 2 GiB.  plan != NULL: sized on device as
 * nmgp_gemm_grouped_dyn_* (32-row tiles), `grid` workgroups (rounded up to a multiple of 8).
 * Same role in the step as nmgp_gemm_grouped_*: code/utils.py:117-146, code/nmgp_dsvi.py:172-258. */
int nmgp_gemm_grouped_lat_f64(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles, const int32_t* d_seg,
                              int32_t* plan, int grid, hipStream_t stream);
int nmgp_gemm_grouped_lat_f32(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles, const int32_t* d_seg,
                              int32_t* plan, int grid, hipStream_t stream);
/* Tile plans computed ahead (e.g. right after the minibatch gather, on another stream): the plan
 * kernels alone (64-row tiles for the tile kernel, 32-row for the latency kernel), and the grouped
 * launches that use such a plan as is.                                                         */
int nmgp_gemm_plan(const nmgp_gemm_desc* d_desc, int nprob, const int32_t* d_seg, int32_t* plan, hipStream_t stream);
int nmgp_gemm_plan_lat(const nmgp_gemm_desc* d_desc, int nprob, const int32_t* d_seg, int32_t* plan,
                       hipStream_t stream);
int nmgp_gemm_grouped_dyn_planned_f64(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles,
                                      const int32_t* d_seg, int32_t* plan, int grid, hipStream_t stream);
int nmgp_gemm_grouped_dyn_planned_f32(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles,
                                      const int32_t* d_seg, int32_t* plan, int grid, hipStream_t stream);
int nmgp_gemm_grouped_lat_planned_f64(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles,
                                      const int32_t* d_seg, int32_t* plan, int grid, hipStream_t stream);
int nmgp_gemm_grouped_lat_planned_f32(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles,
                                      const int32_t* d_seg, int32_t* plan, int grid, hipStream_t stream);
/* Persistent latency-kernel launch for groups with more tiles than one round of workgroups: one
 * workgroup per CU walks its tiles with the next tile's first operand panel loaded under the
 * current tile's MFMAs and reduction; results bit-identical to nmgp_gemm_grouped_lat_*.
 * plan != NULL: device tile plan (planned != 0: already computed by nmgp_gemm_plan_lat).       */
int nmgp_gemm_grouped_lat_pipe_f64(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles,
                                   const int32_t* d_seg, int32_t* plan, int planned, hipStream_t stream);
int nmgp_gemm_grouped_lat_pipe_f32(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles,
                                   const int32_t* d_seg, int32_t* plan, int planned, hipStream_t stream);
/* one problem passed by value (host descriptor; tiles fields are filled internally)          */
int nmgp_gemm_f64(const nmgp_gemm_desc* h_desc, const int32_t* d_seg, hipStream_t stream);
int nmgp_gemm_f32(const nmgp_gemm_desc* h_desc, const int32_t* d_seg, hipStream_t stream);

/* ------------------------------------------------------------------ batched Cholesky
 * In place lower Cholesky of `batch` n x n SPD matrices (A + b*strideA), upper triangle zeroed.
 * Replaces torch.cholesky in code/utils.py:46,54,276,347-348.  info[b] = 0 or the first
 * non-positive pivot column (1-based), as LAPACK potrf.                                     */
int nmgp_potrf_batched_f64(double* A, int64_t n, int64_t lda, int64_t strideA, int64_t batch,
                           int32_t* info, hipStream_t stream);
int nmgp_potrf_batched_f32(float* A, int64_t n, int64_t lda, int64_t strideA, int64_t batch,
                           int32_t* info, hipStream_t stream);
/* Out-of-place inverse of lower-triangular L: X = L^{-1} (upper triangle of X zeroed).
 * Used for K22^{-1} = L^{-T} L^{-1} (replaces torch.solve, code/utils.py:119) and the
 * Cholesky / log-det backward of KL_Gaussian (code/utils.py:332-351).                        */
int nmgp_trtri_batched_f64(const double* L, int64_t n, int64_t ldl, int64_t strideL,
                           double* X, int64_t ldx, int64_t strideX, int64_t batch, hipStream_t stream);
int nmgp_trtri_batched_f32(const float* L, int64_t n, int64_t ldl, int64_t strideL,
                           float* X, int64_t ldx, int64_t strideX, int64_t batch, hipStream_t stream);
/* Fused factor + inverse: A <- L = chol(A) in place (upper zeroed), X <- L^{-1}, info as potrf.
 * n <= 256 runs one register-resident kernel per matrix (the DSVI shapes: code/nmgp_dsvi.py:172-177
 * priors and variational covariances, whose inverses feed K12 K22^{-1} and the KL); larger n (HCP
 * M=512, ECoG M=1024, the M=4096 stress case) recurses on halves: leaves (up to 256 wide in f32, 128 in f64) use that kernel,
 * the panel / SYRK / inverse products are batched MFMA GEMMs of size ~n/2, n/4, ...  X's strictly
 * upper part is used as scratch and left zero.  batch <= 65535.                                */
int nmgp_chol_inv_batched_f64(double* A, int64_t n, int64_t lda, int64_t strideA, double* X, int64_t ldx,
                              int64_t strideX, int64_t batch, int32_t* info, hipStream_t stream);
int nmgp_chol_inv_batched_f32(float* A, int64_t n, int64_t lda, int64_t strideA, float* X, int64_t ldx,
                              int64_t strideX, int64_t batch, int32_t* info, hipStream_t stream);
/* The same with caller workspace for n > 256 (f32): the recursion's products then run split-K where
 * their 128x128 tile grid would not fill the chip (M=4096 stress case).  ws: at least
 * nmgp_chol_inv_workspace_size_f32(n, batch) bytes, zero-filled once before first use (the kernels
 * leave their counters zero again); ws == NULL runs without split-K.                           */
int64_t nmgp_chol_inv_workspace_size_f32(int64_t n, int64_t batch);
int nmgp_chol_inv_batched_ws_f32(float* A, int64_t n, int64_t lda, int64_t strideA, float* X, int64_t ldx,
                                 int64_t strideX, int64_t batch, int32_t* info, void* ws, int64_t ws_bytes,
                                 hipStream_t stream);
/* Round 6, the KL L-bar solve form (f32, n > 256): A <- L as above, but X holds only the inverses X11, X22 of the
 * top-level split's two diagonal blocks (n1 = nmgp_chol_split_point(n) rows / columns, then n - n1): the off-diagonal
 * block X21 = -X22 L21 X11 (two products of the recursion's top level) is not formed, and the factor's off-diagonal
 * block L21 is returned in X21's place (X rows n1.., columns 0..n1-1) -- A21 is left as scratch, A12 and X12 are not
 * written (no staging copy, no zeroing).  The caller applies L^-1 / L^-T blockwise (engine.py, kl_solve):
 * Sigma^-1 L_f = L^-T (L^-1 L_f) for the KL gradient of code/utils.py:339-351 without forming L^-1.           */
int64_t nmgp_chol_split_point(int64_t n);
int nmgp_chol_blockinv_batched_f32(float* A, int64_t n, int64_t lda, int64_t strideA, float* X, int64_t ldx,
                                   int64_t strideX, int64_t batch, int32_t* info, hipStream_t stream);

/* Fused GP-prior launch (round 6): up to 4 prior matrices of one DSVI step (A: K22 + jitter I, read) factored and
 * inverted as nmgp_chol_inv_batched_f64 does (A <- L, X <- L^-1, info), where a matrix with rows != 0 also gets its
 * minibatch products formed by extra workgroups of the same launch while the factorization runs (rows 1: K12 =
 * RBF(x, Z) rows, s2 exp(-(x_i/ls - z_j/ls)^2 / 2) with hyp = (log s2, log ls), code/utils.py:91-94; rows 2: first
 * the t-row sample of JGP_S -- ell_X = exp(P_t v + z_t sqrt(s2_t - ||T_t row||^2 + jitter)), code/utils.py:216-237
 * -- then K12 = Gibbs(x, Z, ell_X, ellZ) rows, code/utils.py:97-103): K12 (written out), T = K12 L^-T (right-looking,
 * from the published block columns of L) and P = T L^-1 = K12 (K22 + jitter I)^-1 (from the published rows of
 * X) -- the projections torch.solve forms in code/utils.py:117-120, 140-146, 228-232.
 * 128 <= n <= 256, 1 <= batch <= 4, B <= 4096; every output of row stride n.  The mats with rows != 0 need K12 /
 * T / P, x and Z; rows 2 needs Pt, Tt (B x n, the t prior's P and T), v, zt, hyp_t (log s2_t), ellX, var_t (B
 * outputs) and ellZ.                                                                                           */
typedef struct nmgp_chol_tp_mat {
  int32_t reserved;   /* 0 */
  int32_t rows;       /* 0: no minibatch products; 1: RBF K12 rows; 2: t-row + Gibbs K12 rows */
  const double* hyp;  /* rows 1: (log sigma2, log lengthscale) */
  double* K12;        /* B x n */
  double* T;          /* B x n */
  double* P;          /* B x n */
} nmgp_chol_tp_mat;
typedef struct nmgp_chol_tp_args {
  double* A;
  int64_t n, lda, strideA;
  double* X;
  int64_t ldx, strideX, batch;
  int32_t* info;
  double jitter;
  const double* Z;     /* n inducing inputs */
  const double* ellZ;  /* n Gibbs length scales (rows 2) */
  const double* x;     /* B minibatch inputs */
  int64_t B;
  const double* Pt;    /* rows 2: the t prior's P and T (B x n), the v sample (n), z_t (B), log s2_t */
  const double* Tt;
  const double* v;
  const double* zt;
  const double* hyp_t;
  double* ellX;        /* rows 2 outputs (B) */
  double* var_t;
  nmgp_chol_tp_mat mats[4];
  /* vg_wgs > 0 (round 6): mats[0] is Sigma_v (rows 0) and vg_wgs extra workgroups form, once L_v is factored,
   * v = vg_muv + L_v vg_z -> vg_v, exp(v) -> vg_ellZ and the Gibbs prior's K22 + jitter I (lower 16 x 16 tiles,
   * leading dimension n) -> vg_K22: nmgp_dsvi_vg22_*'s outputs from the same launch (code/utils.py:97-103,
   * code/nmgp_dsvi.py:198-215).  0: off.                                                                 */
  const double* vg_muv;
  const double* vg_z;
  double* vg_v;
  double* vg_ellZ;
  double* vg_K22;
  int64_t vg_wgs;
} nmgp_chol_tp_args;
int nmgp_chol_tp_f64(const nmgp_chol_tp_args* args, hipStream_t stream);
/* diagnostics (synchronous): the launch's per-workgroup phase stamps, recorded when NMGP_TP_DBG has bit 16 set
 * (8 x 64-bit wall-clock words per workgroup, tools/chol_tp_probe.py)                                  */
int nmgp_chol_tp_trace(uint64_t* out, int64_t n);

/* Single large SPD matrix (the M=4096 stress configuration, BASELINE.json configs[4]): blocked
 * right-looking Cholesky, A <- L in place (strictly upper part zeroed), info as potrf (first
 * non-positive pivot column, 1-based).  Replaces torch.cholesky / LAPACK potrf on one K_uu + jitter
 * (code/utils.py:32-40, 343-344; SIM_code/Utility/kernels.py:64 for the legacy kernels).
 * 128-wide fused leaves, panel GEMM against the leaf's inverse, one block column of lookahead, and the
 * trailing SYRK on a library-owned side stream joined back to `stream` through events (capturable
 * into a graph).  ws: nmgp_potrf_blocked_workspace_size_*(n) bytes, zero-filled once before first use
 * (the split-K counters are left zero again).                                                   */
int64_t nmgp_potrf_blocked_workspace_size_f32(int64_t n);
int64_t nmgp_potrf_blocked_workspace_size_f64(int64_t n);
int nmgp_potrf_blocked_f32(float* A, int64_t n, int64_t lda, int32_t* info, void* ws, int64_t ws_bytes,
                           hipStream_t stream);
int nmgp_potrf_blocked_f64(double* A, int64_t n, int64_t lda, int32_t* info, void* ws, int64_t ws_bytes,
                           hipStream_t stream);

/* ------------------------------------------------------------------ symmetric eigensolver
 * W[b] = eigenvalues of the symmetric A[b] (ascending, as torch.linalg.eigh / torch.symeig), V[b] =
 * eigenvectors as columns (V[i*ldv + j] = component i of vector j).  Replaces torch.symeig(B) /
 * torch.symeig(K) in kron_inv / kron_logdet (code/SIM_code/Utility/kronecker_operation.py:45,47,66,
 * 67) and multivariate_normal_logpdf0/1 (code/SIM_code/Utility/distributions.py:37,40,67,70).
 * Parallel cyclic Jacobi: n <= 64 one workgroup per matrix in LDS; larger n block Jacobi on 64x64
 * pair sub-problems with a device convergence flag (asynchronous, graph-capturable).  A is not
 * modified.  ws: nmgp_syevj_workspace_size_f64(n) bytes (no zero-fill needed).                  */
int64_t nmgp_syevj_workspace_size_f64(int64_t n);
int nmgp_syevj_batched_f64(const double* A, int64_t n, int64_t lda, int64_t strideA, int64_t batch, double* W,
                           int64_t strideW, double* V, int64_t ldv, int64_t strideV, void* ws, int64_t ws_bytes,
                           hipStream_t stream);

/* ------------------------------------------------------------------ large-tile f32 GEMM / SYRK
 * C(i,j) = alpha * sum_k A[i*lda + k] * op(B)(k,j) + beta * C[i*sCi + j*sCj], batched with strides
 * sAb/sBb/sCb; op(B)(k,j) = B[j*ldb + k] (b_kcontig = 1) or B[k*ldb + j] (0).  flags: NMGP_A_LOWER,
 * NMGP_B_UPPER, NMGP_B_LOWER (structural zeros: k ranges trimmed, diagonal k-tiles masked) and
 * NMGP_OUT_LOWER (m == n: only the lower triangle is computed and stored -- SYRK).  128x128 tiles on
 * v_mfma_f32_32x32x2_f32.  The trailing update / panel / inverse products of the recursive
 * Cholesky (the torch.cholesky of code/utils.py:46,276,347 at M >= 512).  ws as above
 * (nmgp_gemm_big_workspace_size bytes) or NULL.                                                */
int64_t nmgp_gemm_big_workspace_size(void);
int nmgp_gemm_big_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int b_kcontig, float* C,
                      int64_t sCi, int64_t sCj, int m, int n, int k, int flags, double alpha, double beta,
                      int64_t sAb, int64_t sBb, int64_t sCb, int batch, void* ws, hipStream_t stream);
/* The same for `batch` problems at arbitrary element offsets (device int64 arrays offA/offB/offC:
 * problem b uses A + offA[b], B + offB[b], C + offC[b]) -- the D + Q variational factors of the
 * engine, which sit at non-uniform offsets of the parameter vector (the live i >= j blocks of the dense
 * D x D Sigma_U layout).  NMGP_OUT_TRIL stores zeros above the diagonal; diag_add is added to C(i,i)
 * (Sigma_f = tril(S_f) tril(S_f)^T + jitter I, code/nmgp_dsvi.py:172-177, code/utils.py:343-344).  */
int nmgp_gemm_big_offsets_f32(const float* A, int64_t lda, const float* B, int64_t ldb, int b_kcontig, float* C,
                              int64_t sCi, int64_t sCj, int m, int n, int k, int flags, double alpha, double beta,
                              double diag_add, const int64_t* offA, const int64_t* offB, const int64_t* offC,
                              int batch, void* ws, hipStream_t stream);
/* General form: op(A)(i,k) = A[i*lda + k] (a_kcontig = 1) or A[k*lda + i] (0), NMGP_A_UPPER allowed,
 * and with NMGP_EPI (+ NMGP_EPI_E_LOWER) the epilogue adds gamma * RS_b[i] * E_b(i, j), E_b = E + offE[b]
 * with strides (sEi, sEj), RS_b = RS + offRS[b]: the KL L-bar of every variational factor,
 * -C^-T (C^-1 L) + diag(1/C_ii^2) L (code/utils.py:339-351 and its autograd), for all D + Q + 1
 * factors in one launch.  kseg != NULL: problem b sums k over [seg[kseg[b]], seg[kseg[b] + kspan[b]])
 * of the device segment table (A and B advanced to that k), the rows of the outputs it covers -- the
 * L-bar products P^T W of the quadratic forms (code/nmgp_dsvi.py:227-258 and their autograd).
 * All nmgp_gemm_big_* forms: every problem's A, B, C and E span must stay below 2 GiB (32-bit buffer
 * offsets; -40 otherwise), output strides are non-negative, and E must not alias C (a tile's C and E
 * values are read before its stores).                                                               */
int nmgp_gemm_big_offsets_epi_f32(const float* A, int64_t lda, int a_kcontig, const float* B, int64_t ldb,
                                  int b_kcontig, float* C, int64_t sCi, int64_t sCj, int m, int n, int k, int flags,
                                  double alpha, double beta, double diag_add, const int64_t* offA,
                                  const int64_t* offB, const int64_t* offC, const float* E, const int64_t* offE,
                                  int64_t sEi, int64_t sEj, const float* RS, const int64_t* offRS, double gamma,
                                  const int32_t* seg, const int32_t* kseg, const int32_t* kspan, int batch,
                                  void* ws, hipStream_t stream);
/* ... and with per-problem ROW ranges (rseg != NULL): problem b's rows are [seg[rseg[b]], seg[rseg[b] +
 * rspan[b]]) of A, C (and E, RS), at most m -- the quadratic-form factors W = P L and the P-bar products
 * W-hat L^T on the rows of the outputs each latent / pair factor serves (code/nmgp_dsvi.py:227-258), on the
 * 128x128 kernel for the fp32 M >= 512 shapes.  Not with NMGP_OUT_LOWER.                                  */
int nmgp_gemm_big_offsets_seg_f32(const float* A, int64_t lda, int a_kcontig, const float* B, int64_t ldb,
                                  int b_kcontig, float* C, int64_t sCi, int64_t sCj, int m, int n, int k, int flags,
                                  double alpha, double beta, double diag_add, const int64_t* offA,
                                  const int64_t* offB, const int64_t* offC, const float* E, const int64_t* offE,
                                  int64_t sEi, int64_t sEj, const float* RS, const int64_t* offRS, double gamma,
                                  const int32_t* seg, const int32_t* kseg, const int32_t* kspan, const int32_t* rseg,
                                  const int32_t* rspan, int batch, void* ws, hipStream_t stream);
/* NMGP_EPI product (offsets, no OUT_LOWER / OUT_TRIL, no split-K) that also stores the raw product
 * acc(i, j) = sum_k op(A)(i,k) op(B)(k,j) to D_b(i, j) = D[offD[b] + i*sDi + j] (sDi >= n) besides
 * C = alpha acc + beta C + gamma RS E: the KL L-bar solve form's G21 = X22^T W21, added to the gradient rows and
 * needed again for G11 = X11^T (W11 - L21^T G21).  a_kcontig 0 or 1, b_kcontig 0.                       */
int nmgp_gemm_big_offsets_dual_f32(const float* A, int64_t lda, int a_kcontig, const float* B, int64_t ldb,
                                   int b_kcontig, float* C, int64_t sCi, int64_t sCj, int m, int n, int k, int flags,
                                   double alpha, double beta, const int64_t* offA, const int64_t* offB,
                                   const int64_t* offC, const float* E, const int64_t* offE, int64_t sEi, int64_t sEj,
                                   const float* RS, const int64_t* offRS, double gamma, float* D, const int64_t* offD,
                                   int64_t sDi, int batch, hipStream_t stream);

/* ------------------------------------------------------------------ pairwise kernel builder
 * mode RBF:   K = scale2 * exp(-0.5 * ||x/ls - z/ls||^2)          (code/utils.py:91-94)
 *             EXPAND distance: ||x||^2+||z||^2-2x.z on x/ls, z/ls (SIM_code/Utility/kernels.py:24-43)
 * mode GIBBS: K = scale2 * [sigX sigZ] * sqrt(2 lx lz / (lx^2+lz^2)) * exp(-r2/(lx^2+lz^2))
 *             (code/utils.py:97-103; SIM_code/Utility/kernels.py:46-73 with sigma, EXPAND)
 * + diag_add on i == j (the 1e-4 / 1e-6 jitters).                                            */
enum { NMGP_RBF = 0, NMGP_GIBBS = 1 };
enum { NMGP_DIST_DIFF = 0, NMGP_DIST_EXPAND = 1 };
enum { NMGP_HYP_LOG = 1 };     /* hyp[] holds log(scale2), log(ls): exponentiate on device */

typedef struct nmgp_pairwise_desc {
  const void* X; const void* Z;          /* (n x p), (m x p) row-major                  */
  const void* ellX; const void* ellZ;    /* GIBBS per-point length scales               */
  const void* sigX; const void* sigZ;    /* optional per-point sigma (legacy), or NULL  */
  const void* hyp;                       /* device [scale2, ls] (RBF) / [scale2] (GIBBS), or NULL */
  void* K;
  int64_t ldk;
  int32_t n, m, p, mode, dist, flags;
  double scale2, length_scale, diag_add;
  int32_t tiles, tile_start;   /* tiles = ceil(n/8) * ceil(m/64) (8-row x 64-column output tiles)           */
} nmgp_pairwise_desc;

int nmgp_pairwise_f64(const nmgp_pairwise_desc* d_desc, int ndesc, int total_tiles, hipStream_t stream);
int nmgp_pairwise_f32(const nmgp_pairwise_desc* d_desc, int ndesc, int total_tiles, hipStream_t stream);
int nmgp_pairwise_single_f64(const nmgp_pairwise_desc* h_desc, hipStream_t stream);
int nmgp_pairwise_single_f32(const nmgp_pairwise_desc* h_desc, hipStream_t stream);

/* Backward of the builder for Kbar = Rbar - rowcoef(i) * Pm (Pm / rowcoef optional):
 *   RBF:   scal_part[t*2+0] += sum Kbar*K, scal_part[t*2+1] += sum Kbar*K*r2   (per tile t)
 *   GIBBS: row_part[ct*n + i] = sum_j Kbar*K*dlogK/dlx_i over column tile ct,
 *          col_part[rt*m + j] = sum_i Kbar*K*dlogK/dlz_j over row tile rt,
 *          scal_part[t*2+0]  = sum Kbar*K
 * Tiles are 8 rows x 64 columns (tiles = ceil(n/8) * ceil(m/64)); partial sums are deterministic.   */
typedef struct nmgp_pairwise_bwd_desc {
  const void* X; const void* Z; const void* ellX; const void* ellZ; const void* hyp;
  const void* K; const void* Rbar; const void* Pm; const void* rowcoef;
  void* row_part; void* col_part; void* scal_part;
  int64_t ld;
  int32_t n, m, p, mode, flags, tiles, tile_start, pad_;
  double scale2, length_scale;
} nmgp_pairwise_bwd_desc;

int nmgp_pairwise_bwd_f64(const nmgp_pairwise_bwd_desc* d_desc, int ndesc, int total_tiles, hipStream_t stream);
int nmgp_pairwise_bwd_f32(const nmgp_pairwise_bwd_desc* d_desc, int ndesc, int total_tiles, hipStream_t stream);
int nmgp_pairwise_bwd_single_f64(const nmgp_pairwise_bwd_desc* h_desc, hipStream_t stream);
int nmgp_pairwise_bwd_single_f32(const nmgp_pairwise_bwd_desc* h_desc, hipStream_t stream);

/* Deterministic column sums of a (rows x cols) row-major array: out[j] = beta*out[j] + sum_i a[i*cols+j] */
int nmgp_colsum_f64(const double* a, int64_t rows, int64_t cols, double beta, double* out, hipStream_t stream);
int nmgp_colsum_f32(const float* a, int64_t rows, int64_t cols, double beta, float* out, hipStream_t stream);

/* ------------------------------------------------------------------ Kronecker kernels
 * kronecker_product (SIM_code/Utility/kronecker_operation.py:5-22): out[(i*r2+k)*(c1*c2)+j*c2+l] =
 *   t1[i,j]*t2[k,l]  (one multiply per element: bit-exact)
 * kronecker_product_diag (:25-33): out[i*n2+k] = d1[i]*d2[k]
 * kron_mv (:72-85): out = (B kron K) y, B (P1 x P2), K (N1 x N2), y (P2*N2) -> (P1*N1).  P2 <= 8: one
 *   fused launch streaming K once (work unused, may be NULL); otherwise two GEMMs through work (N1*P2). */
int nmgp_kron_product_f64(const double* t1, int64_t r1, int64_t c1, const double* t2, int64_t r2, int64_t c2,
                          double* out, hipStream_t stream);
int nmgp_kron_product_diag_f64(const double* d1, int64_t n1, const double* d2, int64_t n2, double* out,
                               hipStream_t stream);
int nmgp_kron_mv_f64(const double* B, int64_t P1, int64_t P2, const double* K, int64_t N1, int64_t N2,
                     const double* y, double* out, double* work, hipStream_t stream);
int nmgp_kron_product_f32(const float* t1, int64_t r1, int64_t c1, const float* t2, int64_t r2, int64_t c2,
                          float* out, hipStream_t stream);
int nmgp_kron_product_diag_f32(const float* d1, int64_t n1, const float* d2, int64_t n2, float* out,
                               hipStream_t stream);
int nmgp_kron_mv_f32(const float* B, int64_t P1, int64_t P2, const float* K, int64_t N1, int64_t N2,
                     const float* y, float* out, float* work, hipStream_t stream);

/* ------------------------------------------------------------------ DSVI step kernels
 * The fused, closed-form DSVI objective and gradients (NMGP.forward + autograd backward,
 * code/nmgp_dsvi.py:157-301) are assembled by the host from the primitives above plus the
 * row / reduction kernels below, all reading one argument block.  See DESIGN.md §4.       */
typedef struct nmgp_dsvi_args {
  /* sizes */
  int32_t D, M, B, Q, NF, elbo_mode, frozen_mask;
  int32_t pair_packed;         /* 0: mu_U (D,D,M), sqrt_U (D,D,M,M) as the reference; 1: (Q,M), (Q,M,M) */
  double N_over_B, jitter;
  /* parameters: flat theta in the registration order of code/nmgp_dsvi.py:117-155 */
  const void* theta; void* grad;
  int64_t off_muW, off_sW, off_muv, off_sv, off_muU, off_sU, off_hyp;
  /* minibatch: rows grouped by output; seg[o]..seg[o+1] = rows of output o */
  const void* x; const void* y; const int32_t* row_out; const int32_t* seg; const void* Z;
  const void* noise;          /* z_v (M) | z_t (B) | z_pairs (Q x B), reference call order */
  /* factor storage (see DESIGN.md §3 for the layout) */
  void* Afac;                 /* (NF+4, M, M): A1 -> C1 (variational), then priors t,0,1,G -> C2 */
  void* Cinv;                 /* (NF+4, M, M) inverses of the factors                          */
  void* Ainv;                 /* (4, M, M) prior inverses t,0,1,G                              */
  void* K12; void* P; void* Pbar; void* R;   /* (4, B, M) each, order t,0,1,G           */
  void* Abar;                 /* (4, M, M) prior adjoints                                      */
  void* WG; void* WP;         /* (D, B, M) quadratic-form factors                              */
  void* Y;                    /* Ainv * mu : G (D x M) | t (1 x M) | 0 (D*D x M) | 1 (D*D x M)   */
  void* Xs;                   /* (NF, M, M) scratch: Cinv_f * L_f                              */
  void* v; void* vbar; void* ellZ; void* ellX; void* var_t;   /* (M),(M),(M),(B),(B)          */
  void* rowbuf;               /* (2D+5, B) per-row adjoints                                     */
  void* facbuf;               /* KL (NF) | delta (4,M) | wvec (4,M) | sel (4,D*D) | e (NF,M)   */
  void* red;                  /* per-block partial sums                                        */
  void* out;                  /* [0] loss [1] SELBO_R [2] KL_W [3] KL_v [4] KL_U  (16 entries;  */
                              /* [8..14] training-step pre-sums of nmgp_dsvi_prefinal_*)      */
  void* gib_row; void* gib_col; void* scal_part; void* phi;
  int32_t* info;
  int32_t n_ct, n_rt, n_rt22, nblk_rows;
  int64_t scal_off[8];        /* tile offsets of the RBF backward problems L0_12,L0_22,L1_12,L1_22,t12,t22 */
  void* T;                    /* (4, B, M) K12 C2^-T per prior (t,0,1,G): the Nystrom variance
                                 rowsum(P o K12) is formed as ||T_row||^2 (no cancellation-prone
                                 explicit-inverse product) and P = T C2^-1                       */
  /* pair sharding (SURVEY §8e axis 3; 0 / D / 1 = the whole model): the packed pairs this rank holds
     are [pair_q0, pair_q0 + Q) -- the pairs (i, j <= i) of a contiguous range of outputs, blocks of
     mu_U / sqrt_U / Y / noise numbered from pair_q0; n_wfac = number of W factors in the factor list
     (D on the rank that owns KL_W, else 0); kl_v = 1 on the rank that owns KL_v                   */
  int32_t pair_q0, n_wfac, kl_v, pair_pad;
  /* fp32 engines (round 3): (4, B, M) fp64 K12 C2^-T per prior, formed from fp64 kernel matrices and fp64
     prior factors; when set, the Nystrom variances k11 - ||T_row||^2 are taken from it in fp64 (the fp32
     T is not read).  NULL: use T */
  const void* T64;
  /* KL factor range (round 3, compute_ELBO with the KL sharded over ranks): only the variational factors
     f in [kl_f0, kl_f1) of the W | pairs list (and the v factor when kl_v) are given a KL term; the whole
     model is [0, NF - 1) */
  int32_t kl_f0, kl_f1;
  /* fp64 sample / hyper-gradient path of fp32 engines (round 3; all NULL otherwise):
     v64     (M, M) fp64 lower Cholesky factor of Sigma_v + 1e-4 I: the v sample mu_v + C z is formed in
             fp64 (ell_Z = exp(v) amplifies its absolute error), written to v / ellZ (fp32) and ellZ64;
     ellZ64  (M) fp64 ell_Z;
     K12_64  (4, B, M) fp64 K12 of the priors (slot 0 = t);
     t64     fp64 t-prior adjoint workspace: [P-bar_t (B x M) | varbar (B) | per-4-row varbar partials]
             written by the t-row backward (the t-prior builder backward and hyper-parameter partials then
             run in fp64 from it: K12 - P K22 cancels to ~1e-4 P, cond ~1e7 at the ECoG length scales);
     scal64  fp64 hyper-parameter partials of the t-prior builders (t12 tiles, then t22 tiles), summed
             by the finalize kernel in fp64 (sigma2_tildeell_log / length_scales_tildeell_log)          */
  const void* v64;
  void* ellZ64;
  const void* K12_64;
  void* t64;
  void* scal64;
  /* round 6: when non-NULL, the training step's finalize kernel advances this optimizer step counter by one at its
     end (the captured step then runs nmgp_adam_lower_advanced_*, which reads the advanced counter: one launch fewer
     at the step's tail).  NULL: untouched.                                                                      */
  int64_t* adam_step;
} nmgp_dsvi_args;

int nmgp_dsvi_hyper_f64(const nmgp_dsvi_args* a, hipStream_t s);      /* hyper values + v sample   */
int nmgp_dsvi_vg22_f64(const nmgp_dsvi_args* a, hipStream_t s);       /* v sample + K_G22 + jitter I (fused priors) */
int nmgp_dsvi_trow_f64(const nmgp_dsvi_args* a, hipStream_t s);       /* t-row forward             */
int nmgp_dsvi_recon_f64(const nmgp_dsvi_args* a, hipStream_t s);      /* recon + per-row adjoints  */
int nmgp_dsvi_kl_f64(const nmgp_dsvi_args* a, hipStream_t s);         /* KL per factor + e-vectors */
int nmgp_dsvi_delta_f64(const nmgp_dsvi_args* a, hipStream_t s);      /* prior diag adjoints delta, w */
int nmgp_dsvi_tbwd_f64(const nmgp_dsvi_args* a, hipStream_t s);       /* t-row backward            */
int nmgp_dsvi_vbwd_f64(const nmgp_dsvi_args* a, hipStream_t s);       /* v backward -> Phi         */
int nmgp_dsvi_finalize_f64(const nmgp_dsvi_args* a, hipStream_t s);   /* loss + scalar gradients   */
int nmgp_dsvi_mugrad_f64(const nmgp_dsvi_args* a, hipStream_t s);     /* KL mean gradients of mu_W / mu_v / mu_U */
/* Training steps: nmgp_dsvi_finalize_* adds the KL mean gradients itself when D M + M + (pair columns) M is at most
 * NMGP_MUGRAD_IN_FINALIZE_MAX; larger engines launch nmgp_dsvi_mugrad_* (after the L-bar and v backward, before
 * finalize).                                                                                                   */
#define NMGP_MUGRAD_IN_FINALIZE_MAX 65536
int nmgp_dsvi_prefinal_f64(const nmgp_dsvi_args* a, hipStream_t s);   /* training step: recon + KL sums -> out[8..14] */
/* fp32 twins (HCP / ECoG-shaped configurations): same arguments, every buffer float */
int nmgp_dsvi_hyper_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_vg22_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_trow_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_recon_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_kl_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_delta_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_tbwd_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_vbwd_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_finalize_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_mugrad_f32(const nmgp_dsvi_args* a, hipStream_t s);
int nmgp_dsvi_prefinal_f32(const nmgp_dsvi_args* a, hipStream_t s);

/* ------------------------------------------------------------------ optimiser / RNG
 * torch.optim.Adam update (code/nmgp_dsvi.py:777,854) on a flat parameter vector; step is a
 * device counter (incremented by the kernel's last block) so the call can be graph-replayed.  */
int nmgp_adam_f64(double* theta, const double* grad, double* m, double* v, int64_t n,
                  int64_t* step, double lr, double beta1, double beta2, double eps, hipStream_t stream);
int nmgp_adam_f32(float* theta, const float* grad, float* m, float* v, int64_t n,
                  int64_t* step, double lr, double beta1, double beta2, double eps, hipStream_t stream);
/* The same update where the ranges tri[2k] .. tri[2k] + tri[2k+1] M^2 of the vector are lower-triangular M x M
 * blocks (sqrt_W, sqrt_v, sqrt_U: their strictly upper triangles never receive a gradient, code/utils.py:68-72 --
 * torch's Adam leaves them unchanged): only the 16-byte vectors holding lower-triangle elements are read and
 * written there (bit-identical to nmgp_adam_*); ranges ascending and disjoint, 16-byte aligned, M % (16 / size) == 0.
 * tri is a HOST array of ntri (offset, blocks) pairs.  One step-counter increment.                          */
int nmgp_adam_lower_f64(double* theta, const double* grad, double* m, double* v, int64_t n, const int64_t* tri,
                        int ntri, int M, int64_t* step, double lr, double beta1, double beta2, double eps,
                        hipStream_t stream);
int nmgp_adam_lower_f32(float* theta, const float* grad, float* m, float* v, int64_t n, const int64_t* tri, int ntri,
                        int M, int64_t* step, double lr, double beta1, double beta2, double eps, hipStream_t stream);
/* The same update for a step counter that was ALREADY advanced for this step (by the finalize kernel, adam_step
 * above): the bias corrections use step[0] itself and the counter is not advanced again.  One launch; needs the
 * aligned single-launch form (16-byte pointers, M and every range offset multiples of 16 / size, ntri <= 4), else
 * -12.                                                                                                          */
int nmgp_adam_lower_advanced_f64(double* theta, const double* grad, double* m, double* v, int64_t n,
                                 const int64_t* tri, int ntri, int M, const int64_t* step, double lr, double beta1,
                                 double beta2, double eps, hipStream_t stream);
int nmgp_adam_lower_advanced_f32(float* theta, const float* grad, float* m, float* v, int64_t n, const int64_t* tri,
                                 int ntri, int M, const int64_t* step, double lr, double beta1, double beta2,
                                 double eps, hipStream_t stream);
/* Counter-based Philox4x32-10 standard normals: out[0:n] = the first n elements of the stream with key `seed`
 * and base = *counter + offset (counter == NULL reads as 0): so (counter = c, offset = o) and (counter = c + o,
 * offset = 0) are the same stream, and a shorter call is a prefix of a longer one.  Quad t = i / 4 runs Philox
 * on the counter words (t_lo, t_hi, base_lo, base_hi) with key (seed_lo, seed_hi); its four words c_q give
 * u_q = (c_q + 0.5) * 2^-32 and, by Box-Muller in float64, out[4t .. 4t+3] = (r0 cos 2 pi u1, r0 sin 2 pi u1,
 * r1 cos 2 pi u3, r1 sin 2 pi u3), r0 = sqrt(-2 ln u0), r1 = sqrt(-2 ln u2), rounded to the output type.
 * base does NOT shift the element index: streams of different bases share no quad.               */
int nmgp_normal_f64(double* out, int64_t n, uint64_t seed, const int64_t* counter, int64_t offset,
                    hipStream_t stream);
int nmgp_normal_f32(float* out, int64_t n, uint64_t seed, const int64_t* counter, int64_t offset,
                    hipStream_t stream);
int nmgp_counter_add(int64_t* counter, int64_t inc, hipStream_t stream);
/* Element-wise precision conversion dst[i] = (dst type) src[i] (round to nearest for f64 -> f32).
 * fp32 engines (HCP / ECoG shapes) factor the four GP priors K22 + 1e-4 I in fp64: the fp32
 * explicit-inverse projections K12 (K22 + 1e-4 I)^-1 of code/utils.py:117-119 otherwise lose
 * ~cond(K22) * eps.                                                            */
/* P-bar_G of the DSVI backward (autograd of code/nmgp_dsvi.py:227-238 through utils.MGP_mu_sigma2,
 * code/utils.py:128-146): for every row r of output i (rows grouped by output, seg[0..D]),
 * P[r, :] += Z[0][r, :] + Z[1][r, :] + ... + Z[i][r, :] in that order, where Z[d] = W-hat_d L_d^T (stride sZ
 * elements between factors, row stride M) was formed for the rows of outputs >= d.  0 or -(argument). */
int nmgp_pbar_reduce_f64(const double* Z, int64_t sZ, double* P, int64_t ldp, const int32_t* seg, int D, int B, int M,
                         hipStream_t stream);
int nmgp_pbar_reduce_f32(const float* Z, int64_t sZ, float* P, int64_t ldp, const int32_t* seg, int D, int B, int M,
                         hipStream_t stream);
/* ------------------------------------------------------------------ pair-block streaming products (round 5)
 * The per-pair products of the DSVI step when each output owns few minibatch rows (ECoG: ~4 of B = 512 per
 * output, Q = 8256 pairs of M = 1024): one problem per coefficient pair (i, j), rows r in [seg[s], seg[s+1]).
 * Each streams its M x M lower-triangular block once (HBM-bound) with the rows' operands on chip; row r of an
 * operand at base + offset + r * M (row stride M), blocks row-major with leading dimension M.
 *   quad : C[r] = A[r] L              (A at a_off, L at l_off, C at c_off)  -- code/utils.py:115-120 (MGP_d),
 *                                      the quadratic-form factors W = P L_ij of code/nmgp_dsvi.py:227-237
 *   dot  : Z[r] = W[r] L^T            (W at a_off, L at l_off, Z at c_off)  -- their P-bar (autograd)
 *   rank : G[k][c] += sum_r P[r][k] W[r][c] for c <= k  (P at a_off, G at l_off, W at c_off; the strictly
 *          upper part of G is not touched)                                -- the pair's L-bar (autograd)
 *   mv   : C[c] += sum_r A[r][c] x[r] over the problem's rows (A at a_off, x at l_off, C at c_off; any M)
 *          -- the pair's mu-bar (autograd of mu_ij in W = mu + L eps), round 6
 *   pair_pbar_reduce: row r of output i (i0 <= i < i1): P1[r] += Z_i[r], P0[r] += Z_0[r] + ... + Z_{i-1}[r]
 *          in j order (Z_j at Z + j sZ) -- the L1 / L0 prior P-bars of code/nmgp_dsvi.py:227-237
 * M must be a multiple of 4 (f32) / 2 (f64); quad needs M <= 2048 (f32) / 3072 (f64), dot and rank M <= 1024.
 * Deterministic (fixed summation order).  0 or -(argument index).                                       */
typedef struct nmgp_pair_desc {
  int64_t a_off, l_off, c_off;   /* element offsets of the three operands */
  int32_t seg;                   /* segment index s: the problem's rows are seg[s] .. seg[s+1]-1 */
  int32_t pad;
} nmgp_pair_desc;
int nmgp_pair_quad_f64(const double* A, const double* L, double* C, const nmgp_pair_desc* descs, int nprob,
                       const int32_t* seg, int M, hipStream_t stream);
int nmgp_pair_quad_f32(const float* A, const float* L, float* C, const nmgp_pair_desc* descs, int nprob,
                       const int32_t* seg, int M, hipStream_t stream);
int nmgp_pair_dot_f64(const double* W, const double* L, double* Z, const nmgp_pair_desc* descs, int nprob,
                      const int32_t* seg, int M, hipStream_t stream);
int nmgp_pair_dot_f32(const float* W, const float* L, float* Z, const nmgp_pair_desc* descs, int nprob,
                      const int32_t* seg, int M, hipStream_t stream);
int nmgp_pair_rank_f64(const double* P, double* G, const double* W, const nmgp_pair_desc* descs, int nprob,
                       const int32_t* seg, int M, hipStream_t stream);
int nmgp_pair_rank_f32(const float* P, float* G, const float* W, const nmgp_pair_desc* descs, int nprob,
                       const int32_t* seg, int M, hipStream_t stream);
int nmgp_pair_mv_f64(const double* A, const double* x, double* C, const nmgp_pair_desc* descs, int nprob,
                     const int32_t* seg, int M, hipStream_t stream);
int nmgp_pair_mv_f32(const float* A, const float* x, float* C, const nmgp_pair_desc* descs, int nprob,
                     const int32_t* seg, int M, hipStream_t stream);
int nmgp_pair_pbar_reduce_f64(const double* Z, int64_t sZ, double* P0, double* P1, int64_t ldp, const int32_t* seg,
                              int D, int i0, int i1, int B, int M, hipStream_t stream);
int nmgp_pair_pbar_reduce_f32(const float* Z, int64_t sZ, float* P0, float* P1, int64_t ldp, const int32_t* seg,
                              int D, int i0, int i1, int B, int M, hipStream_t stream);
/* L-bar / mu-bar of the latent factors in the DSVI backward (autograd of code/nmgp_dsvi.py:198-215, W = mu + L eps
 * and MGP_d's L-products): factor d's gradient collects Y_{i,d} = P_G[rows of i]^T W-hat_d[rows of i] over outputs
 * i = d .. D-1.  Slot (i, d) is Y + (first(d) + i - d) * sY, first(d) = sum_{d' < d} (D - d'): an M x M matrix, then an
 * M-vector at offset M * M.  Adds, in i order, the matrices' lower triangles onto gA + d * sA (upper triangle set to
 * 0) and the vectors onto gB + d * sB.  0 or -(argument).                                                          */
int nmgp_lbar_reduce_f64(const double* Y, int64_t sY, double* gA, int64_t sA, double* gB, int64_t sB, int D, int M,
                         hipStream_t stream);
int nmgp_lbar_reduce_f32(const float* Y, int64_t sY, float* gA, int64_t sA, float* gB, int64_t sB, int D, int M,
                         hipStream_t stream);
int nmgp_convert_f32_to_f64(const float* src, double* dst, int64_t n, hipStream_t stream);
int nmgp_convert_f64_to_f32(const double* src, float* dst, int64_t n, hipStream_t stream);
/* On-device minibatch pipeline (replaces the host DataLoader + vec2list split of
 * code/nmgp_dsvi.py:816-837 for a dataset resident in HBM): copies minibatch
 * b = (*batch_counter) % nbatch of pre-split, output-grouped batches (Xb/Yb (nbatch,B) f64, Ib
 * (nbatch,B) int32 row->output, Sb (nbatch,nseg) int32 segment table) into the engine's inputs
 * and then advances *batch_counter -- one launch, graph-capturable, no host work per step.      */
/* Start of one training step in a single launch: the minibatch gather of nmgp_batch_gather_* (batch
 * (*bctr) % nbatch, bctr advanced), nnoise Philox normals exactly as nmgp_normal_*(noise, nnoise, seed,
 * nctr, 0) with *nctr advanced by one afterwards, and grad[0:ngrad] = 0 -- the DataLoader draw
 * (code/nmgp_dsvi.py:829-837), optimizer.zero_grad() (:830) and the step's torch.randn draws
 * (code/utils.py:123, 226, 234).  done: one int32, zero before first use (left zero).            */
int nmgp_step_begin_f64(const double* Xb, const double* Yb, const int32_t* Ib, const int32_t* Sb, int64_t B,
                        int64_t nseg, int64_t nbatch, int64_t* bctr, double* x, double* y, int32_t* row_out,
                        int32_t* seg, double* noise, int64_t nnoise, uint64_t seed, int64_t* nctr, int32_t* done,
                        double* grad, int64_t ngrad, hipStream_t stream);
int nmgp_step_begin_f32(const float* Xb, const float* Yb, const int32_t* Ib, const int32_t* Sb, int64_t B,
                        int64_t nseg, int64_t nbatch, int64_t* bctr, float* x, float* y, int32_t* row_out,
                        int32_t* seg, float* noise, int64_t nnoise, uint64_t seed, int64_t* nctr, int32_t* done,
                        float* grad, int64_t ngrad, hipStream_t stream);
/* The same start of a step together with two theta-only launches of the fused-prior schedule, in ONE launch: the
 * pairwise group pw (npd descriptors, pw_tiles tiles: the RBF K22 + lam I; as nmgp_pairwise_*) and the grouped GEMM gd
 * (ngd descriptors, lat_tiles tiles, laid out for nmgp_gemm_grouped_lat_* WITHOUT a device tile plan: Sigma_v + lam I;
 * lat_seg: its segment table or NULL) run as further workgroups of the grid, each exactly as in its own launch.
 * Neither may read what the begin part writes (minibatch, noise, gradient).  Error codes as nmgp_step_begin_*, then
 * -20 pw / npd / pw_tiles, -23 gd / ngd / lat_tiles missing or not positive.                                      */
int nmgp_step_head_f64(const double* Xb, const double* Yb, const int32_t* Ib, const int32_t* Sb, int64_t B,
                       int64_t nseg, int64_t nbatch, int64_t* bctr, double* x, double* y, int32_t* row_out,
                       int32_t* seg, double* noise, int64_t nnoise, uint64_t seed, int64_t* nctr, int32_t* done,
                       double* grad, int64_t ngrad, const nmgp_pairwise_desc* pw, int npd, int pw_tiles,
                       const nmgp_gemm_desc* gd, int ngd, int lat_tiles, const int32_t* lat_seg, hipStream_t stream);
int nmgp_step_head_f32(const float* Xb, const float* Yb, const int32_t* Ib, const int32_t* Sb, int64_t B,
                       int64_t nseg, int64_t nbatch, int64_t* bctr, float* x, float* y, int32_t* row_out,
                       int32_t* seg, float* noise, int64_t nnoise, uint64_t seed, int64_t* nctr, int32_t* done,
                       float* grad, int64_t ngrad, const nmgp_pairwise_desc* pw, int npd, int pw_tiles,
                       const nmgp_gemm_desc* gd, int ngd, int lat_tiles, const int32_t* lat_seg, hipStream_t stream);
int nmgp_batch_gather_f64(const double* Xb, const double* Yb, const int32_t* Ib, const int32_t* Sb, int64_t B,
                          int64_t nseg, int64_t nbatch, int64_t* batch_counter, double* x, double* y,
                          int32_t* row_out, int32_t* seg, hipStream_t stream);
int nmgp_batch_gather_f32(const float* Xb, const float* Yb, const int32_t* Ib, const int32_t* Sb, int64_t B,
                          int64_t nseg, int64_t nbatch, int64_t* batch_counter, float* x, float* y,
                          int32_t* row_out, int32_t* seg, hipStream_t stream);

/* Fused posterior summaries of NMGP.sample_FY (code/nmgp_dsvi.py:492-580, whose (S, N, D, D) correlation tensor the
 * reference's drivers only ever average, NMGP_ECoG_full.py:329-332).  fp64.  For every sample s < S and input n < N,
 * with q running over the pairs (i, j <= i) in row order (q = i (i + 1) / 2 + j):
 *   l_q = pair_mu[q * ld_pair + n] + pair_sd[q * ld_pair + n] * z_p[s * z_stride + q * N + n],
 *   L_ii = exp(l), L_ij = l (j < i);
 *   Y[(s * N + n) * D + i] = sum_{j <= i} L_ij G[(s * D + j) * N + n] + sd_err * z_f[s * z_stride + n * D + i];
 *   cov = L L^T (v_mfma_f64_16x16x4_f64), corr_ij = cov_ij * sqrt(1 / cov_ii) * sqrt(1 / cov_jj)  (:567-569),
 *   corr_ii = 1 exactly where the expression is finite (its rounding noise on the diagonal would show as 1e-8 in
 *   the sd); where cov_ii is 0, inf or NaN the expression's NaN is kept;
 *   corr_sum[(n * D + i) * D + j] += corr_ij, corr_sq[...] += corr_ij^2   (full symmetric D x D).
 * corr_sum / corr_sq ACCUMULATE (the caller zeroes them once; the chunks of one summary add up); Y is overwritten.
 * z_p and z_f point into one noise block with a per-sample stride of z_stride elements.  When N alone cannot fill
 * the chip the samples are cut into slices whose partial sums go through `ws` (nmgp_fy_workspace_size bytes, 0 when
 * unsliced) and are added in slice order: no floating-point atomics, the same call gives the same bits.  All
 * indexing is 64-bit.  Returns 0 (nothing launched when S == 0 or N == 0), NMGP_ERR_FY_ARG when D is outside
 * 1..128, S or N is negative, a pointer is NULL, ld_pair < N, or the workspace is missing / too small; nothing is
 * launched then either.                                                                                          */
#define NMGP_ERR_FY_ARG (-60)
int64_t nmgp_fy_workspace_size(int D, int N, int S);
int nmgp_fy_accum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* G,
                      const double* z_p, const double* z_f, int64_t z_stride, double sd_err, int D, int N, int S,
                      double* Y, double* corr_sum, double* corr_sq, void* ws, int64_t ws_bytes, hipStream_t stream);

/* Fused held-out summaries of NMGP.sample_Y (code/nmgp_dsvi.py:406-490; the drivers keep a mean curve, a band and an
 * RMSE of its samples, NMGP_ECoG_pred.py:277-299).  fp64.  Input n belongs to output i = I[n]; for every sample
 * s < S and input n < N, with j = 0..i in ascending order and q = i (i + 1) / 2 + j:
 *   l_j = fma(pair_sd[q * ld_pair + n], z_p[s * z_stride + q * N + n], pair_mu[q * ld_pair + n]),  l_i = exp(l_i);
 *   F[s * N + n] = sum_j l_j G[(s * D + j) * N + n]   (one fma per j, chained in j order);
 *   Y[s * N + n] = F + sd_err * z_f[s * z_stride + n];
 *   F_sum[n] += F, F_sq[n] += F^2;  L_sum[n * D + j] += l_j, L_sq[...] += l_j^2 for j <= i (row I_n of L; the
 *   columns j > i are not touched);  G_sum[j * N + n] += G, G_sq[...] += G^2 for every j < D;
 *   with y: a = -0.5 log(2 pi v) - (y[n] - F)^2 / (2 v), v = sd_err^2, folded into the running log-sum-exp
 *   (lse_max[n], lse_sum[n]) -- log sum_s exp(a_s) = lse_max + log(lse_sum) -- by M = max(m1, m2),
 *   r = r1 exp(m1 - M) + r2 exp(m2 - M); the caller starts it at (-inf, 0), two empty states stay (-inf, 0), a NaN
 *   y[n] makes both words NaN at that n only, y[n] = +-inf leaves the state as it was.
 * Only the I_n + 1 pairs of row I_n are read at input n; no (S, D, D, N) tensor exists.  The sums and the
 * log-sum-exp state ACCUMULATE over calls (the caller initialises them once), in sample order; Y and F are
 * overwritten.  y may be NULL: lse_max / lse_sum are then neither required nor touched.  An I[n] outside 0..D-1
 * indexes nothing: Y, F, F_sum, F_sq, the whole row n of L_sum / L_sq and the log-sum-exp state get NaN at that n
 * (G_sum / G_sq do not depend on I).  z_p and z_f point into one noise block with a per-sample stride of z_stride
 * elements.  When ceil(N / 64) (D + 1) waves cannot fill the chip the samples are cut into slices whose sums go
 * through `ws` (nmgp_y_workspace_size bytes, 0 when unsliced, non-decreasing in S) and are added in slice order:
 * no floating-point atomics, the same call gives the same bits.  All indexing is 64-bit.  Returns 0 (nothing
 * launched when S == 0 or N == 0), NMGP_ERR_Y_ARG when D < 1, S or N is negative, a required pointer is NULL
 * (lse_max / lse_sum count when y is given), ld_pair < N, z_stride < 0, S > 262140 or D > 262139 (grid limits), or
 * the workspace is missing / too small; nothing is launched then either.                                         */
#define NMGP_ERR_Y_ARG (-61)
int64_t nmgp_y_workspace_size(int D, int N, int S);
int nmgp_y_accum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* G,
                     const double* z_p, const double* z_f, int64_t z_stride, const int64_t* I, const double* y,
                     double sd_err, int D, int N, int S, double* Y, double* F, double* F_sum, double* F_sq,
                     double* L_sum, double* L_sq, double* G_sum, double* G_sq, double* lse_max, double* lse_sum,
                     void* ws, int64_t ws_bytes, hipStream_t stream);

/* Credible bands of the output correlations (code/utils.py:354-366, plot_corrs: np.quantile(sampled_corrs[:, :, i, j],
 * (0.025, 0.975), axis=0) of NMGP.sample_FY's samples) without the (S, N, D, D) tensor.  fp64, two steps.
 *
 * nmgp_corr_collect_f64: per-sample correlations of a list of P output pairs (i, j) = (pi[p], pj[p]) (device int32
 * arrays).  For every p < P, input n < N and sample s < S of this chunk, with q = a (a + 1) / 2 + b:
 *   l_q = pair_mu[q * ld_pair + n] + pair_sd[q * ld_pair + n] * z_p[s * z_stride + q * N + n],
 *   L_aa = exp(l), L_ab = l (b < a);  cov_ab = sum_{k <= min(a, b)} L_ak L_bk;
 *   C[(p * N + n) * ld_c + s_off + s] = cov_ij * sqrt(1 / cov_ii) * sqrt(1 / cov_jj)   (code/nmgp_dsvi.py:567-569)
 * -- the definitions and the normalisation order of nmgp_fy_accum_f64, so C holds the very samples whose mean is
 * corr_mean.  i < j is allowed and gives the same bits as (j, i); a duplicate pair gives the same bits again;
 * i == j gives exactly 1 where the expression is finite and NaN where it is not (cov_ii 0, inf or NaN).  L is zero
 * above its diagonal and the reference multiplies the full matrices, so a non-finite cov_ii or cov_jj makes the
 * pair NaN at that (n, s) (inf * 0), and only there.  pi / pj outside 0..D-1 cannot be validated on the host: that
 * pair's P-slice of C is NaN, the other pairs are not affected.  C is WRITTEN, never accumulated, every element
 * once: calls over disjoint sample ranges (s_off) give the same bits as one call.  The layout of C -- samples
 * innermost, rows (p, n) -- is what nmgp_quantile_rows_f64 reads: rows = P * N, ld = ld_c.  All indexing is 64-bit.
 *
 * nmgp_quantile_rows_f64: exact order-statistic quantiles of `rows` rows of S values, row r at C + r * ld; elements
 * past S are not read and C is not modified.  qs is a HOST array of nq quantiles in [0, 1] (passed to the kernel by
 * value).  Each row is sorted inside LDS (bitonic network on S padded with +inf); with pos = q (S - 1),
 * lo = floor(pos), a = x_(lo), b = x_(min(lo + 1, S - 1)), w = pos - lo:
 *   out[k * rows + r] = a when w == 0, a + (b - a) w when w < 0.5, else b - (b - a) (1 - w)
 * (torch.lerp; np.quantile's linear method).  A row with a NaN gives NaN for every quantile; +-inf sort as values.
 * Rows of up to 128 values get a wave each, longer rows 128 or 256 threads; one workgroup sorts at most
 * nmgp_quantile_rows_max_S() = 16384 values (128 KiB of the 160 KiB of LDS), a larger S is refused.  No atomics: the
 * same call gives the same bits.
 *
 * Both return 0 and launch nothing when a count is 0, and NMGP_ERR_CORRQ_ARG before any launch when D is outside
 * 1..128, a count or s_off is negative, a pointer is NULL, ld_pair < N, z_stride < 0, ld_c < s_off + S, ld < S,
 * S > nmgp_quantile_rows_max_S(), or a quantile is outside [0, 1] (NaN included).                                 */
#define NMGP_ERR_CORRQ_ARG (-62)
int nmgp_quantile_rows_max_S(void);
int nmgp_corr_collect_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                          int64_t z_stride, const int32_t* pi, const int32_t* pj, int P, int D, int N, int S,
                          double* C, int64_t ld_c, int64_t s_off, hipStream_t stream);
int nmgp_quantile_rows_f64(const double* C, int64_t rows, int S, int64_t ld, const double* qs, int nq, double* out,
                           hipStream_t stream);

/* Partial correlations of the outputs, the companion of the correlations of nmgp_fy_accum_f64: the correlation of
 * outputs i and j given all the others, i.e. the normalised precision matrix.  The reference has no such code; the
 * quantity is a function of NMGP.sample_FY's covariance L L^T (code/nmgp_dsvi.py:567-569) and is scale invariant.
 * fp64.  For every sample s < S and input n < N, with L built from the pair samples exactly as in
 * nmgp_fy_accum_f64 (l_q = pair_mu[q * ld_pair + n] + pair_sd[q * ld_pair + n] * z_p[s * z_stride + q * N + n],
 * L_ii = exp(l), L_ij = l for j < i):
 *   W = L^-1 (lower triangular: 16 x 16 diagonal tiles by substitution, the tiles below them tile row by tile row
 *   on v_mfma_f64_16x16x4_f64),  Omega = W^T W = (L L^T)^-1 (lower triangle, matrix cores),
 *   pcorr_ij = -Omega_ij * sqrt(1 / Omega_ii) * sqrt(1 / Omega_jj) for i != j,  pcorr_ii = 1 exactly;
 *   if any L_kk of that sample at that input is 0, inf or NaN (an exp that under- or overflowed), EVERY pcorr_ij of
 *   that sample at that input is NaN, the diagonal included; other inputs and samples are not affected;
 *   pc_sum[(n * D + i) * D + j] += pcorr_ij, pc_sq[...] += pcorr_ij^2   (full symmetric D x D);
 *   with a pair list (P > 0; pi / pj device int32): C[(p * N + n) * ld_c + s_off + s] = pcorr_{pi[p], pj[p]}.
 * pc_sum / pc_sq ACCUMULATE (the caller zeroes them once; the chunks of one summary add up); both NULL = collect
 * only: the same C bits are written and no sum (and no workspace) is touched.  C is WRITTEN, every element once, in
 * the layout nmgp_quantile_rows_f64 reads (rows = P * N, ld = ld_c); (i, j) and (j, i) give the same bits, a
 * duplicate pair the same bits again, i == j the diagonal value (1, or NaN by the rule above); pi / pj outside
 * 0..D-1 cannot be validated on the host: that pair's slice of C is NaN.  The samples are cut into slices by the rule
 * of nmgp_fy_accum_f64 (none when N >= 256); the slices' partial sums go through `ws` (nmgp_pcorr_workspace_size
 * bytes, 0 when unsliced) and are added in slice order: no floating-point atomics, the same call gives the same
 * bits.  L and W share one workgroup's LDS (2 x 72 KiB at D = 128).  All indexing is 64-bit.  Returns 0 (nothing
 * launched when S == 0 or N == 0), NMGP_ERR_PCORR_ARG before any launch when D is outside 1..128, a count or s_off
 * is negative, ld_pair < N, z_stride < 0, pair_mu / pair_sd / z_p is NULL, exactly one of pc_sum / pc_sq is NULL,
 * the sums and the pair list are both absent, P > 0 and pi, pj or C is NULL or ld_c < s_off + S, or the sums are
 * given and the workspace is missing / too small.                                                              */
#define NMGP_ERR_PCORR_ARG (-63)
int64_t nmgp_pcorr_workspace_size(int D, int N, int S);
int nmgp_pcorr_accum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                         int64_t z_stride, int D, int N, int S, double* pc_sum, double* pc_sq, const int32_t* pi,
                         const int32_t* pj, int P, double* C, int64_t ld_c, int64_t s_off, void* ws, int64_t ws_bytes,
                         hipStream_t stream);

/* Group means of the output correlations (reference NMGP_ECoG_full.py:456-544, "Post analysis": the correlations
 * averaged over the neighbour and distance groups of the electrode grid) and of the partial correlations, per
 * sample, without the (S, N, D, D) tensor and without per-pair samples.  fp64.
 *
 * The group table is a CSR in DEVICE memory (a launch can be captured): goff, K + 1 int32 offsets into the entries
 * (goff[0] = 0, goff[K] = E), and gent, E int32 entries (max(i, j) << 16) | min(i, j).  Order and duplicates count
 * (a pair listed twice weighs twice), groups may overlap, (i, i) is the diagonal value.  The table cannot be
 * validated on the host, and it cannot make the kernel leave its buffers: offsets are clamped to 0..E and made
 * monotone (a group left empty is 0 / 0 = NaN), an entry outside 0..D-1 is NaN and so is its group, the other
 * groups are not affected.
 *
 * nmgp_corr_group_f64: for every group k < K, input n < N and sample s < S of this chunk, with corr the correlation
 * of nmgp_fy_accum_f64 (the same L, the same MFMA order, the same normalisation acc * isi * isj, the diagonal
 * exactly 1 where finite, non-finite values kept: a group of one pair is that correlation bit for bit),
 *   C[(k * N + n) * ld_c + s_off + s] = (sum_{e in group k} corr[s, n, i_e, j_e]) / |group k|.
 * A group with a NaN correlation at (s, n) is NaN at (s, n).  The sum is taken in float64 in an order that is a
 * function of the group alone -- up to 256 entries: lane l of one wave adds the entries l, l + 64, ..., then a xor
 * butterfly over the lanes; longer: thread t of the workgroup adds the entries t, t + 256, ..., a butterfly per
 * wave, the 4 wave sums added in wave order -- so C does not depend on the other groups of the call, on how the
 * samples are split over calls (s_off) or over slices, nor on the run: no atomics, no workspace, every element of the
 * addressed columns written exactly once, the other columns of a wider C left alone.  One workgroup per (input,
 * slice of samples) with L and the normalised triangle in LDS (2 x 72 KiB + 1 KiB at D = 128).  Returns 0 and
 * launches nothing when K, N or S is 0, NMGP_ERR_CGROUP_ARG before any launch when D is outside 1..128, N, S, K or
 * s_off is negative, a pointer is NULL, E < K, ld_pair < N, z_stride < 0 or ld_c < s_off + S.
 *
 * nmgp_pcorr_accum_groups_f64: nmgp_pcorr_accum_f64 with a third, independent output next to the sums and the pair
 * list: Cg[(k * N + n) * ld_cg + sg_off + s] = the group means of that sample's partial correlations (the values
 * the pair list collects; NaN everywhere where the sample is NaN), by the same reduction.  K = 0 is
 * nmgp_pcorr_accum_f64 exactly (which forwards here); sums and C have the same bits with and without groups, Cg
 * the same bits with and without sums and pair list.  Refused (NMGP_ERR_PCORR_ARG) as nmgp_pcorr_accum_f64, and
 * when sums, pair list and groups are all absent, K or sg_off is negative, or K > 0 and goff, gent or Cg is NULL,
 * E < K or ld_cg < sg_off + S.                                                                                  */
#define NMGP_ERR_CGROUP_ARG (-64)
int nmgp_corr_group_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                        int64_t z_stride, int D, int N, int S, const int32_t* goff, const int32_t* gent, int K,
                        int E, double* C, int64_t ld_c, int64_t s_off, hipStream_t stream);
int nmgp_pcorr_accum_groups_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                                int64_t z_stride, int D, int N, int S, double* pc_sum, double* pc_sq,
                                const int32_t* pi, const int32_t* pj, int P, double* C, int64_t ld_c, int64_t s_off,
                                const int32_t* goff, const int32_t* gent, int K, int E, double* Cg, int64_t ld_cg,
                                int64_t sg_off, void* ws, int64_t ws_bytes, hipStream_t stream);

/* Conditional prediction of the missing outputs at an input from the outputs observed at the same input, per
 * posterior sample, fused (csrc/ycond.hip).  The reference has no such code; the quantity is a function of what
 * NMGP.sample_FY samples (code/nmgp_dsvi.py:519-569).  fp64.  For every sample s < S and input n < N, with L built
 * from the pair samples exactly as in nmgp_pcorr_accum_f64, mu_g / var_g (S, N, D) contiguous the marginals of the
 * latent G of that sample, V = diag(var_g + 1e-4) and s2 the noise variance (jitter included):
 *   y(x_n) ~ N(L mu_g, L V L^T + s2 I).  Row n of Y_obs (N, D contiguous) has observed (finite) and missing
 *   (non-finite) entries;  A = V^-1 + L^T diag(w) L with w_o = 1 / s2 where observed and 0 elsewhere,
 *   b = V^-1 mu_g + L^T (w o y),  A = R R^T (tiled Cholesky on v_mfma_f64_16x16x4_f64),  c = R^-1 b,
 *   w_h = R^-1 l_h (l_h = row h of L as a column),  mu = w_h^T c,  v = |w_h|^2 + s2  for every missing h.
 * The missing entries of Y_obs in (n, d) row-major order are the E entries; e_off (N + 1 device int32) is the
 * prefix sum of the rows' missing counts (e_off[0] = 0, e_off[N] = E) and must agree with the mask of Y_obs: a
 * table that does not cannot make the kernel leave its buffers (its offsets are clamped to 0..E and made monotone,
 * a row's count is clipped to the mask's), but the entries it misplaces are undefined.  A row without a missing entry does no work.
 *   mu_sum[e] += mu,  y2_sum[e] += v + mu^2,  f2_sum[e] += v - s2 + mu^2   (ACCUMULATED: the caller zeroes them);
 *   with y_true (E, NULL = none): (lse_max[e], lse_sum[e]) <- the running log-sum-exp state of
 *   log N(y_true[e] | mu, v) over the samples, combined as in nmgp_y_accum_f64 (the caller starts it at (-inf, 0));
 *   a non-finite y_true[e] leaves its state untouched;
 *   with Mu / Var (both or neither; ld rows of E): Mu[(s_off + s) * E + e] = mu, Var[...] = v, every addressed
 *   element written once, the other rows left alone.
 * A sample whose L_kk is 0, inf or NaN at input n, or whose var_g + 1e-4 is not finite and positive there, gives
 * NaN mu and v at every entry of that input (and NaN sums); other inputs are not affected.  Slicing, workspace
 * (nmgp_ycond_workspace_size bytes, 0 when unsliced) and determinism as nmgp_pcorr_accum_f64: no floating-point
 * atomics, the same call gives the same bits.  L and A share one workgroup's LDS (149.5 KiB at D = 128).  Returns
 * 0 (nothing launched when S, N or E is 0), NMGP_ERR_YCOND_ARG before any launch when D is outside 1..128, a
 * count or s_off is negative, E > N D, s2 is not positive, ld_pair < N, z_stride < 0, an input or a sum is NULL,
 * exactly one of Mu / Var is NULL or ld < s_off + S, y_true is given without lse_max / lse_sum, or the workspace is
 * missing / too small.                                                                                          */
#define NMGP_ERR_YCOND_ARG (-65)
int64_t nmgp_ycond_workspace_size(int D, int N, int S);
int nmgp_ycond_accum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                         int64_t z_stride, const double* mu_g, const double* var_g, const double* Y_obs, double s2,
                         int D, int N, int S, const int32_t* e_off, int E, double* mu_sum, double* y2_sum,
                         double* f2_sum, const double* y_true, double* lse_max, double* lse_sum, double* Mu,
                         double* Var, int64_t ld, int64_t s_off, void* ws, int64_t ws_bytes, hipStream_t stream);

/* Eigenvalues of the sample's output correlation matrix, per posterior sample and input, fused (csrc/spectrum.hip):
 * how many independent modes the outputs have and how strong the common mode is.  The reference has no such code;
 * the quantity is a function of NMGP.sample_FY's correlation (code/nmgp_dsvi.py:567-569).  fp64.  For every sample
 * s < S and input n < N, with L built from the pair samples exactly as in nmgp_fy_accum_f64 and
 * Is_i = sqrt(1 / |row i of L|^2) as in nmgp_corr_group_f64:  G = diag(Is) L,  R = G G^T (trace D), and
 * lambda_1 >= ... >= lambda_D the eigenvalues of R, found by one-sided Jacobi rotations of the column pairs of G in
 * one workgroup's LDS (136 KiB at D = 128) until every pair has |g_p . g_q| <= sqrt(max(D, 4)) 2^-53 |g_p| |g_q|
 * (LAPACK's dgesvj criterion; 2^-52 up to D = 4 -- at 2^-52 for every D about one random matrix in 50000 cycles
 * between two roundings and never ends), at most 30 sweeps;
 * then lambda_j = |g_j|^2 and u_j = g_j / |g_j|, sorted descending (ties by column).  Where not a single pair
 * needed a rotation R is the identity (the diagonal of a correlation is exactly 1 in this family) and every
 * lambda is exactly 1; so it is for D = 1.
 *   E[(r * N + n) * ld_e + s_off + s] = lambda_{r+1} for r < k,
 *   E[(k * N + n) * ld_e + s_off + s] = D^2 / sum_{j <= D} lambda_j^2   (the effective dimension, over all D),
 *   with load2_sum (N, k, D contiguous; NULL = none): load2_sum[(n * k + r) * D + d] += u_{r+1,d}^2  (ACCUMULATED:
 *   the caller zeroes it; sign-free, each mode's D values sum to 1).
 * E is WRITTEN, every addressed element once, the other columns of a wider E left alone.  If some L_ii of the sample
 * at n is 0, inf or NaN (or an Is is not finite and positive), every row of E at (s, n) is NaN and NaN is added to
 * the loadings of n; other inputs and samples are not affected.  A finite input that has not converged after 30
 * sweeps is NaN in the same way and adds 1 to *unconverged (device int32, required, never reset here).  E comes from
 * the one workgroup that owns (s, n), from that sample alone: no floating-point atomics, the same bits in every run
 * and however the samples are split over calls (s_off) or slices.  The samples are cut into slices by the rule of
 * nmgp_fy_accum_f64 (none when N >= 256); the slices' loading sums go through `ws`
 * (nmgp_corr_spectrum_workspace_bytes, 0 when unsliced or without loadings) and are added to load2_sum in slice
 * order.  All indexing is 64-bit.  Returns 0 (nothing launched when N == 0 or S == 0), NMGP_ERR_SPECTRUM_ARG before
 * any launch when D is outside 1..128, k outside 1..D, N, S, s_off or ws_bytes is negative, pair_mu, pair_sd, z_p,
 * E or unconverged is NULL, ld_pair < N, z_stride < 0, ld_e < s_off + S, or load2_sum is given, the samples are
 * sliced and the workspace is missing / too small.                                                              */
#define NMGP_ERR_SPECTRUM_ARG (-66)
int64_t nmgp_corr_spectrum_workspace_bytes(int D, int N, int S, int k);
int nmgp_corr_spectrum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                           int64_t z_stride, int D, int N, int S, int k, double* E, int64_t ld_e, int64_t s_off,
                           double* load2_sum, void* ws, int64_t ws_bytes, int32_t* unconverged, hipStream_t stream);

/* Exact scores of equal-weight Gaussian mixtures (csrc/mixscore.hip): CRPS, PIT and quantiles of the predictives of
 * nmgp_y_accum_f64 (components N(F_sn, s2)) and nmgp_ycond_accum_f64 (components N(mu_se, v_se)).  The reference has
 * no such code.  fp64, no matrix cores.  Entry e < E has the S components mu_s = Mu[s * ld_mu + e] and
 * v_s = Var[s * ld_var + e] (the component axis is the slow one, as the collected buffers lie; ld >= E, so Mu / Var
 * may be column ranges of wider buffers), or v_s = var_scalar for every s and e when Var is NULL (a compile-time
 * variant of the kernels with sigma and the pair sigma hoisted).  With sigma_s = sqrt(v_s), Phi the normal CDF and
 *   A(m, v) = m erf(m / sqrt(2 v)) + sqrt(2 v / pi) exp(-m^2 / (2 v)):
 *   pit[e]    = (1/S) sum_s Phi((y[e] - mu_s) / sigma_s)                                  (needs y),
 *   spread[e] = t2 = (sum_{t<s} A(mu_s - mu_t, v_s + v_t) + sum_s sigma_s / sqrt(pi)) / S^2
 *             = (1 / (2 S^2)) sum_s sum_t A(mu_s - mu_t, v_s + v_t),
 *   crps[e]   = (1/S) sum_s A(y[e] - mu_s, v_s) - t2                                      (needs y),
 *   quantiles[k * ld_q + e] = the root q of (1/S) sum_s Phi((q - mu_s) / sigma_s) = p[k], bisected from
 *     [min_s, max_s](mu_s + z_p[k] sigma_s), widened by 1e-12 max_s(|mu_s| + |z_p[k]| sigma_s), until no double lies
 *     strictly between the ends; the end with the smaller |F - p| is returned.  z_p[k] = Phi^-1(p[k]) comes from the
 *     caller; p and z_p are HOST arrays of nq <= 16 values (passed to the kernel by value), p strictly inside (0, 1).
 *     A quantile not down to adjacent doubles after 200 steps is NaN and adds 1 to *unconverged (device int32,
 *     required with nq > 0, never reset here).
 * Every output is optional (NULL = not computed) and WRITTEN at its E addressed elements only; y (E, contiguous) is
 * required by pit and crps.  An entry with a non-finite mu_s, or a v_s that is non-finite or <= 0, is NaN in every
 * output (and not counted in *unconverged); a non-finite y[e] makes pit[e] and crps[e] NaN, spread and quantiles
 * are still computed; other entries are not affected.  A workgroup serves 8 adjacent entries (64-byte row segments
 * of Mu / Var).  The S (S - 1) / 2 pair terms of an entry are cut into min(T (T + 1) / 2, 64) slices of tile pairs,
 * T = ceil(S / 128): a function of S alone.  The slices' partial sums go through `ws` (nmgp_mix_score_workspace_size
 * bytes; needed for crps / spread only, 0 at S = 1) and are added in slice order, every reduction inside a workgroup
 * in a fixed order: no floating-point atomics, the same call gives the same bits, and an entry's bits do not
 * depend on which other entries share the call.  All indexing is 64-bit.  Returns 0 (nothing launched when E == 0),
 * NMGP_ERR_MIX_ARG before any launch when S is outside 1..2^20, E or nq is negative, nq > 16, E > 8 (2^31 - 1), Mu
 * is NULL, ld_mu < E, Var is given with ld_var < E or is NULL with a var_scalar that is not finite and positive, pit
 * or crps is asked for without y, no output is asked for, nq > 0 and z_p, p, quantiles or unconverged is NULL or
 * ld_q < E, a p[k] is not strictly inside (0, 1), a z_p[k] is not finite, or crps / spread is asked for and the
 * workspace is missing / too small.                                                                              */
#define NMGP_ERR_MIX_ARG (-67)
int64_t nmgp_mix_score_workspace_size(int S, int64_t E);
int nmgp_mix_score_f64(const double* Mu, int64_t ld_mu, const double* Var, int64_t ld_var, double var_scalar, int S,
                       int64_t E, const double* y, const double* z_p, const double* p, int nq, double* pit,
                       double* crps, double* spread, double* quantiles, int64_t ld_q, int32_t* unconverged, void* ws,
                       int64_t ws_bytes, hipStream_t stream);

/* Local stationary fits around the inducing points, fused (csrc/preest.hip): the reference's pre_estimation_partial
 * (code/pre_nmgp.py:102-125), one workgroup per inducing point, fp64, no matrix cores.  x (N inputs of the complete
 * rows, element stride x_stride >= 1), Yrot = Y V_B (N rows of D, row stride ld_y >= D), mu (D, the eigenvalues of
 * B = Y^T Y / (N - 1) = V_B diag(mu) V_B^T), z (M inducing inputs, element stride z_stride >= 1).  Window m holds the
 * P rows with the smallest |x_n - z_m| (ties to the lower row), written in ascending row order to
 * neighbours[m * P + p] (optional).  Its likelihood is vec(Y_loc) ~ N(0, K(ell) (x) B + s I), evaluated as
 *   nll = 1/2 sum_pd [log G_pd + E_pd / G_pd] + 1/2 P D log 2 pi,  G_pd = lam_p mu_d + s,  E = (V_K^T Yrot_loc)^2,
 * K = V_K diag(lam) V_K^T the RBF kernel of the window inputs (divide by ell, then difference; ell < 1e-8 clamped).
 * nmgp_pre_estimate_f64 minimises it over the box log ell in [log(delta / 4), log(16 span)] (delta the smallest
 * positive gap of the sorted window inputs, span their range), log s in log(mean mu) + [-14, 2], by the fixed search
 * described in csrc/preest.hip, and writes log_ell[m], log_s[m], nll[m], flags[m] and (optional) box[m * 4 + 0..3] =
 * the four box ends in that order.  Flag bits: 1 / 2 log ell at its lower / upper end, 4 / 8 log s at its lower /
 * upper end, 16 a Jacobi solve did not converge in 30 sweeps, 32 degenerate window (span 0 or fewer than P finite
 * inputs: the results are NaN).  nmgp_pre_loglik_f64 evaluates nll[m * E + e] at the caller's pairs
 * pars[(m * E + e) * 2 + 0 / 1] = (log s, log ell) on the same windows (flags: bits 16 and 32 only).  Only the
 * addressed elements are written.  Every loop is bounded and every sum has a fixed order: the same call gives the
 * same bits, and a window's bits do not depend on the other windows of the call.  Both return 0 (nothing launched at
 * M == 0) and NMGP_ERR_PREEST_ARG before any launch when P is outside 3..32, D outside 1..128, N < P, M or E is
 * negative, a required pointer is NULL, a stride is below 1, ld_y < D, or an element offset ((N - 1) x_stride,
 * N ld_y, (M - 1) z_stride, M P) passes 2^31 - 1.                                                              */
#define NMGP_ERR_PREEST_ARG (-68)
int nmgp_pre_estimate_f64(const double* x, int64_t x_stride, const double* Yrot, int64_t ld_y, const double* mu,
                          const double* z, int64_t z_stride, int N, int D, int M, int P, double* log_ell,
                          double* log_s, double* nll, int32_t* flags, int32_t* neighbours, double* box,
                          hipStream_t stream);
int nmgp_pre_loglik_f64(const double* x, int64_t x_stride, const double* Yrot, int64_t ld_y, const double* mu,
                        const double* z, int64_t z_stride, int N, int D, int M, int P, const double* pars, int E,
                        double* nll, int32_t* flags, int32_t* neighbours, hipStream_t stream);

/* The same search and evaluation on windows handed over as data (code/pre_nmgp.py:64-100: the coefficient factor
 * differs from window to window, so every window has its own eigenbasis): xs[m * P + p] the window inputs,
 * Yrot_loc[(m * P + p) * D + d] = (Y_loc V_m), mu[m * D + d] the eigenvalues of that window's B_m = V_m diag(mu_m)
 * V_m^T.  The kernel body, the search, the flags and the results are those of the two entries above; a window with a
 * non-finite input is flagged degenerate.  window_flags (optional, M): a window with a non-zero entry (the flags of
 * nmgp_pre_local_factor_f64) is not fitted, its results are NaN and its flags that entry.  NMGP_ERR_PREEST_ARG before any launch when P is outside 3..32, D outside
 * 1..128, M or E is negative, a required pointer is NULL or M P D passes 2^31 - 1.                              */
int nmgp_pre_estimate_windows_f64(const double* xs, const double* Yrot_loc, const double* mu, int M, int D, int P,
                                  const int32_t* window_flags, double* log_ell, double* log_s, double* nll,
                                  int32_t* flags, double* box, hipStream_t stream);
int nmgp_pre_loglik_windows_f64(const double* xs, const double* Yrot_loc, const double* mu, int M, int D, int P,
                                const int32_t* window_flags, const double* pars, int E, double* nll, int32_t* flags,
                                hipStream_t stream);

/* Local coefficient factors around the inducing points, fused (csrc/prelocal.hip): what the reference's
 * pre_estimation_all (code/pre_nmgp.py:64-100) set out to estimate per window, one workgroup per inducing point.
 * The rows with a finite |x_n - z_m| are ordered by (|x_n - z_m|, n); the fit window is the first P rows (the window
 * of nmgp_pre_estimate_f64), the covariance window the next cov_rows rows (holdout = 1) or the first cov_rows rows
 * (holdout = 0).  B_local[m] = w (Y_w^T Y_w) + alpha B (D x D, symmetric bit for bit; Y_w the covariance rows, summed
 * in ascending row order on the fp64 matrix cores; B (D x D, row stride ld_b) the global matrix), L[m] its lower
 * Cholesky factor (upper triangle 0, no jitter).  Also written: neighbours[m * P + p] and cov_neighbours[m * cov_rows
 * + c] in ascending row order, xs[m * P + p] and Yloc[(m * P + p) * D + d] the fit rows, flags[m]: 32 fewer than
 * P holdout + cov_rows finite inputs (tables -1, the rest NaN), NMGP_PRE_FLAG_FACTOR a pivot of B_local[m] was not
 * positive (L[m] is NaN; the other windows are unaffected).  The same call gives the same bits, and a window's bits
 * do not depend on the other windows.  Returns NMGP_ERR_PRELOCAL_ARG before any launch when P is outside 3..32,
 * D outside 1..128, cov_rows outside P..1024, P holdout + cov_rows > N, alpha outside [0, 1], w negative or not
 * finite, holdout not 0 / 1, a pointer is NULL, a stride is below 1, ld_y or ld_b < D, or an element offset passes
 * 2^31 - 1.                                                                                                  */
#define NMGP_ERR_PRELOCAL_ARG (-69)
#define NMGP_PRE_FLAG_FACTOR 64
int nmgp_pre_local_factor_f64(const double* x, int64_t x_stride, const double* Y, int64_t ld_y, const double* B,
                              int64_t ld_b, const double* z, int64_t z_stride, int N, int D, int M, int P,
                              int cov_rows, int holdout, double w, double alpha, double* B_local, double* L,
                              int32_t* neighbours, int32_t* cov_neighbours, double* xs, double* Yloc, int32_t* flags,
                              hipStream_t stream);

/* Whole-step HIP graphs (the reference runs its step eagerly, code/nmgp_dsvi.py:829-854; the build captures
 * noise -> forward -> backward -> Adam once and replays it).  Capture goes straight through the HIP runtime:
 * begin on `stream` (thread-local mode; other streams join through event waits and must join back before
 * the end), end + instantiate into an executable graph handle, launch it on a stream, destroy it.  The body
 * must not allocate or synchronise.  Returns NMGP_ERR_LAUNCH on a runtime failure; a failed end of capture
 * leaves nothing behind.                                                                                  */
int nmgp_graph_begin(hipStream_t stream);
int nmgp_graph_end(hipStream_t stream, void** exec_out);
int nmgp_graph_launch(void* exec, hipStream_t stream);
int nmgp_graph_destroy(void* exec);

/* Events a captured step graph records as EXTERNAL event nodes (hipEventRecordWithFlags(...,
 * hipEventRecordExternal)): a stream outside the graph can wait on a point INSIDE a replayed step -- the
 * data-parallel step starts the all-reduce of the gradient rows that are final at that point (the sqrt_W /
 * sqrt_U rows after the L-bar products) while the rest of the backward still runs (SURVEY §8e axis 2; the
 * reference's loss.backward(); optimizer.step(), code/nmgp_dsvi.py:847-854, has no such overlap).  Outside a
 * capture the record is a plain event record.  Handles are opaque (hipEvent_t, timing disabled).         */
int nmgp_event_create(void** event_out);
int nmgp_event_destroy(void* event);
int nmgp_event_record_external(void* event, hipStream_t stream);
int nmgp_stream_wait_event(hipStream_t stream, void* event);

#ifdef __cplusplus
}
#endif
#endif /* NMGP_HIP_H */
