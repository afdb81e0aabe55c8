// Eigenvalues of the output correlation matrix of NMGP.sample_FY, per posterior sample and input: how many
// independent modes the D outputs have at x and how strong the common mode is.  The reference has no such code; the
// quantity is a function of the sample's correlation R = diag(Is) L L^T diag(Is) (code/nmgp_dsvi.py:567-569).  Per
// sample s and input n the top k eigenvalues go to E[r, n, s_off + s], the effective dimension D^2 / sum_j lambda_j^2
// to E[k, n, s_off + s], and the squared loadings u_jd^2 of the top k modes are summed over the samples.  The
// (S, N, D, D) tensor is never stored.
//
// Method: one-sided (Hestenes) Jacobi on the columns of G = diag(Is) L, in place in LDS.  R = G G^T has the
// eigenvalues of G^T G; rotating column pairs (p, q) from the right until every pair is orthogonal leaves
// lambda_j = |g_j|^2 and u_j = g_j / |g_j|, an eigenvector of R -- no second (eigenvector) matrix, so D = 128 fits:
// G is D rows of ld doubles, 128 x 136 x 8 B = 136 KiB under the CU's 160 KiB (a two-sided solver with vectors needs
// twice that; eig.hip stops at 64 rows).  L is formed by the expressions of fy_load_L and Is by those of
// fy_row_sums / cgroup.hip (two threads per row, columns of one parity each), in this kernel's row-major layout.
//
// A round rotates the ceil(D / 2) disjoint pairs of the circle ordering of eig.hip (pair k of round r is
// ((r + k) mod m, (r - k) mod m), pair 0 (r, m), m = np - 1, np = D rounded up to even; without eig.hip's swap to
// p < q, which a one-sided rotation does not need).  A pair is owned for the round by LS consecutive lanes (4 at
// D > 64, 8 / 16 / 32 at D <= 64 / 32 / 16): lane `sub` of the set holds the rows sub, sub + LS, ... of both columns
// in registers, the three dot products reduce by a xor butterfly inside the set (every lane gets the same bits), the
// rotation is applied from the registers and written back -- no barrier inside a round, one after it.  A pair is
// rotated when |g_p . g_q| > tol |g_p| |g_q|, tol = sqrt(max(D, 4)) 2^-53 (2^-52 up to D = 4; the criterion of
// LAPACK's dgesvj); a sweep (m rounds) without a rotation ends the solve, 30 sweeps cap it.  With tol = 2^-52 at
// every D a few random matrices never end (1 of the 64800 of tools/spectrum_probe.py at D = 50, 1 of 32000 at
// D = 128, 5 of 200000 at D = 17 in a host emulation): the angle that would cancel a dot product of
// 1.04 x 2^-52 |g_p| |g_q| is below the resolution of the columns' elements, the rotation overshoots to
// -1.04 x 2^-52 and the next sweep rotates back, a cycle of two; every other matrix ends in 5 to 18 sweeps.  The
// rounding of the D-term dot product itself is of the order sqrt(D) 2^-53, so the larger tolerance asks for what
// can be computed.  For odd D the pad index m only ever meets pair 0, which is then skipped: the pad column is not
// stored.
//
// LDS banks: G is row-major with ld = the smallest value >= np with ld mod 32 == 32 / LS.  The 32 lanes of a
// half-wave are 32 / LS pairs x LS rows; consecutive pairs have consecutive columns a (descending b), so the
// ds_read_b64 of column a hits double-bank (sub * ld + a) mod 32 = sub * 32 / LS + a0 + k: all 32 distinct, except in
// the round where the column index wraps around m.  The ds_write_b64 (banked modulo 16 doubles per 16 lanes) is
// 2-way with this ld; not measured against the alternative (ld mod 32 == 16 / LS: writes free, reads 2-way).
//
// After convergence: column norms, a rank sort descending inside LDS (ties by column index), the stores.  Where no
// pair was rotated at all, G's columns were orthogonal from the start, G is diagonal and R is the identity in the
// family's convention (diagonal exactly 1 where finite): every eigenvalue is then exactly 1 (so is D = 1).  A sample
// whose L has a zero or non-finite diagonal entry at n (or a non-finite, zero Is) is NaN in every row of E at (s, n)
// and adds NaN to the loadings of n; its sweep loop ends after one sweep, since a NaN comparison rotates nothing.  A
// finite input that has not converged after 30 sweeps is NaN likewise and counted in *unconverged (one plain vector
// atomic add).  Everything of (s, n) comes from the one workgroup that owns it, from that sample alone: E does not
// depend on the run, on the slices or on how the samples are split over calls (s_off).
//
// Loadings: with k D up to 16384 sums per input there is neither LDS (D = 128) nor registers to hold them over the
// slice, so the workgroup keeps them in its own (slice, n) block of the workspace -- written by the slice's first
// sample, then read, added to and written by the same thread -- and spectrum_reduce_kernel adds the slices in slice
// order onto the caller's (N, k, D) sums.  Unsliced (N >= 256), the block is the caller's sum itself.
#include "fy_tiles.hpp"

namespace nmgp {

constexpr int kSpecSweeps = 30;
constexpr double kSpecTolUnit = 0x1p-53;               // tol = sqrt(max(D, 4)) of it

// Lanes per column pair, rows per lane and the largest D of an instantiation.
__host__ __device__ constexpr int spec_max_d(int LS) { return 512 / LS > kFyMaxD ? kFyMaxD : 512 / LS; }
__host__ __device__ constexpr int spec_rows(int LS) { return (spec_max_d(LS) + LS - 1) / LS; }
// Row stride of G: the smallest ld >= np with ld mod 32 == 32 / LS.
__host__ __device__ constexpr int spec_ld(int np, int LS) {
  const int ld = (np / 32) * 32 + 32 / LS;
  return ld < np ? ld + 32 : ld;
}

template <int LS>
__global__ __launch_bounds__(kFyThreads) void corr_spectrum_kernel(
    const double* __restrict__ pair_mu, const double* __restrict__ pair_sd, int64_t ld_pair,
    const double* __restrict__ z_p, int64_t z_stride, int D, int N, int S, int per, int k, double* __restrict__ E,
    int64_t ld_e, int64_t s_off, double* __restrict__ load2, int64_t slice_stride, int first_writes,
    int* __restrict__ unconverged, int n_blocks) {
  constexpr int R = spec_rows(LS);
  extern __shared__ __attribute__((aligned(16))) double sp_smem[];
  double* Gs = sp_smem;                                 // D rows of ld
  __shared__ double lam[kFyMaxD], nrm[kFyMaxD], Is[kFyMaxD];
  __shared__ int ord[kFyMaxD];
  __shared__ int bad;

  const int n = fy_block_input(n_blocks);
  if (n >= N) return;
  const int slice = blockIdx.y;
  const int s0 = slice * per, s1 = min(S, s0 + per);
  const int tid = threadIdx.x;
  const int np = D + (D & 1), H = np >> 1, m = np - 1, ld = spec_ld(np, LS);
  const int pk = tid / LS, sub = tid % LS;
  const int64_t k_stride = (int64_t)N * ld_e;
  const double nan = __builtin_nan("");
  const double tol = sqrt((double)max(D, 4)) * kSpecTolUnit;

  if (tid < kFyMaxD) ord[tid] = 0;

  for (int s = s0; s < s1; ++s) {
    if (tid == 0) bad = 0;
    __syncthreads();

    // ---- pair samples -> L (the expressions of fy_load_L), zero above the diagonal
    {
      const double* zp = z_p + (int64_t)s * z_stride + n;
#pragma unroll 1
      for (int e = tid; e < D * np; e += kFyThreads) {
        const int i = e / np, j = e - i * np;
        double l = 0.0;
        if (j <= i) {
          const int64_t q = i * (i + 1) / 2 + j;
          l = pair_mu[q * ld_pair + n] + pair_sd[q * ld_pair + n] * zp[q * N];
          if (i == j) {
            l = exp(l);
            if (!(__builtin_isfinite(l) && l != 0.0)) bad = 1;
          }
        }
        Gs[i * ld + j] = l;
      }
    }
    __syncthreads();

    // ---- Is = sqrt(1 / |row i of L|^2), the summation order of fy_row_sums
    {
      const int frow = tid >> 1, fhalf = tid & 1;
      double c = 0.0;
      if (frow < D) {
        for (int j = fhalf; j <= frow; j += 2) {
          const double v = Gs[frow * ld + j];
          c = fma(v, v, c);
        }
      }
      c = c + __shfl_xor(c, 1, 64);
      if (frow < D && fhalf == 0) {
        const double is = sqrt(1.0 / c);
        Is[frow] = is;
        if (!(__builtin_isfinite(is) && is > 0.0)) bad = 1;
      }
    }
    __syncthreads();

    // ---- G = diag(Is) L
#pragma unroll 1
    for (int e = tid; e < D * np; e += kFyThreads) {
      const int i = e / np, j = e - i * np;
      if (j <= i) Gs[i * ld + j] *= Is[i];
    }
    __syncthreads();

    // ---- the sweeps
    bool conv = false, any_rot = false;
    for (int sweep = 0; sweep < kSpecSweeps; ++sweep) {
      int rotated = 0;
      for (int r = 0; r < m; ++r) {
        int a, b;
        if (pk == 0) {
          a = r;
          b = m;
        } else {
          a = r + pk;
          if (a >= m) a -= m;
          b = r - pk;
          if (b < 0) b += m;
        }
        const bool act = pk < H && b < D;               // b == D: the pad column of an odd D
        double p[R], q[R];
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int t = 0; t < R; ++t) {
          const int i = sub + t * LS;
          p[t] = 0.0;
          q[t] = 0.0;
          if (act && i < D) {
            p[t] = Gs[i * ld + a];
            q[t] = Gs[i * ld + b];
          }
          alpha = fma(p[t], p[t], alpha);
          beta = fma(q[t], q[t], beta);
          gamma = fma(p[t], q[t], gamma);
        }
#pragma unroll
        for (int o = 1; o < LS; o <<= 1) {
          alpha += __shfl_xor(alpha, o, 64);
          beta += __shfl_xor(beta, o, 64);
          gamma += __shfl_xor(gamma, o, 64);
        }
        if (act && fabs(gamma) > tol * sqrt(alpha * beta)) {
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + tt * tt);
          const double sn = tt * c;
          // Rutishauser's form of c p - s q and s p + c q: with tau = s / (1 + c), 1 - s tau = c, and a small angle
          // changes a column by a small term instead of scaling it by a rounded c (one ulp per rotation otherwise,
          // which the leading column of nearly equicorrelated outputs collects D times a sweep)
          const double tau = sn / (1.0 + c);
#pragma unroll
          for (int t = 0; t < R; ++t) {
            const int i = sub + t * LS;
            if (i < D) {
              Gs[i * ld + a] = fma(-sn, fma(tau, p[t], q[t]), p[t]);
              Gs[i * ld + b] = fma(sn, fma(-tau, q[t], p[t]), q[t]);
            }
          }
          rotated = 1;
        }
        __syncthreads();
      }
      if (!__syncthreads_or(rotated)) {
        conv = true;
        break;
      }
      any_rot = true;
    }

    // ---- column norms, rank sort descending
    if (tid < D) {
      double c = 0.0;
      for (int i = 0; i < D; ++i) {
        const double v = Gs[i * ld + tid];
        c = fma(v, v, c);
      }
      nrm[tid] = c;
    }
    __syncthreads();
    const bool ok = conv && bad == 0;
    if (tid < D && ok) {
      const double x = nrm[tid];
      int rank = 0;
      for (int l = 0; l < D; ++l) {
        const double y = nrm[l];
        rank += (y > x || (y == x && l < tid)) ? 1 : 0;
      }
      ord[rank] = tid;
      lam[rank] = any_rot ? x : 1.0;
    }
    __syncthreads();

    // ---- the stores of this sample
    double* Eo = E + (int64_t)n * ld_e + s_off + s;
    if (tid < k) Eo[tid * k_stride] = ok ? lam[tid] : nan;
    if (tid == kFyThreads - 1) {
      double s2 = 0.0;
      if (ok)
        for (int j = 0; j < D; ++j) s2 = fma(lam[j], lam[j], s2);
      Eo[k * k_stride] = ok ? (double)D * (double)D / s2 : nan;
      if (!conv && bad == 0) atomicAdd(unconverged, 1);
    }
    if (load2) {
      double* dst = load2 + (int64_t)slice * slice_stride + (int64_t)n * k * D;
      const bool wr = first_writes && s == s0;
      for (int e = tid; e < k * D; e += kFyThreads) {
        const int r = e / D, d = e - r * D;
        double v = nan;
        if (ok) {
          const int j = min(ord[r], D - 1);
          const double g = Gs[d * ld + j];
          v = g * g / nrm[j];
        }
        dst[e] = wr ? v : dst[e] + v;
      }
    }
    __syncthreads();
  }
}

// out (N, k, D) += the nsl slices' sums in the workspace, in slice order.
__global__ void spectrum_reduce_kernel(const double* __restrict__ ws, int nsl, int64_t total, double* __restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    double a = out[e];
    for (int sl = 0; sl < nsl; ++sl) a += ws[(int64_t)sl * total + e];
    out[e] = a;
  }
}

template <int LS, class... Args>
static int spectrum_launch(int D, int N, int nsl, hipStream_t s, Args... args) {
  constexpr int dmax = spec_max_d(LS);
  allow_dynamic_lds<corr_spectrum_kernel<LS>>(dmax * spec_ld(dmax, LS) * sizeof(double));
  const size_t smem = (size_t)D * spec_ld(D + (D & 1), LS) * sizeof(double);
  const int n_blocks = (N + kFyXcds - 1) / kFyXcds * kFyXcds;
  hipLaunchKernelGGL(corr_spectrum_kernel<LS>, dim3((unsigned)n_blocks, (unsigned)nsl), dim3(kFyThreads), smem, s,
                     args..., n_blocks);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int64_t nmgp_corr_spectrum_workspace_bytes(int D, int N, int S, int k) {
  if (D < 1 || D > kFyMaxD || k < 1 || k > D || N <= 0 || S <= 0) return 0;
  int nsl, per;
  fy_slicing(N, S, &nsl, &per);
  return nsl == 1 ? 0 : (int64_t)nsl * N * k * D * (int64_t)sizeof(double);
}

int nmgp_corr_spectrum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                           int64_t z_stride, int D, int N, int S, int k, double* E, int64_t ld_e, int64_t s_off,
                           double* load2_sum, void* ws, int64_t ws_bytes, int32_t* unconverged, hipStream_t stream) {
  if (D < 1 || D > kFyMaxD || k < 1 || k > D || N < 0 || S < 0 || s_off < 0 || ws_bytes < 0)
    return NMGP_ERR_SPECTRUM_ARG;
  if (N == 0 || S == 0) return NMGP_OK;
  if (!pair_mu || !pair_sd || !z_p || !E || !unconverged) return NMGP_ERR_SPECTRUM_ARG;
  if (ld_pair < N || z_stride < 0 || ld_e < s_off + S || N > 0x7fffffff - kFyXcds) return NMGP_ERR_SPECTRUM_ARG;
  int nsl, per;
  fy_slicing(N, S, &nsl, &per);
  const int64_t total = (int64_t)N * k * D;
  const bool sliced = load2_sum && nsl > 1;
  if (sliced && (!ws || ws_bytes < nsl * total * (int64_t)sizeof(double))) return NMGP_ERR_SPECTRUM_ARG;
  double* dst = sliced ? (double*)ws : load2_sum;
  const int H = (D + 1) / 2;
  int rc;
#define NMGP_SPEC_GO(LS)                                                                                          \
  rc = spectrum_launch<LS>(D, N, nsl, stream, pair_mu, pair_sd, ld_pair, z_p, z_stride, D, N, S, per, k, E, ld_e, \
                           s_off, dst, sliced ? total : (int64_t)0, sliced ? 1 : 0, (int*)unconverged)
  if (H <= 8) NMGP_SPEC_GO(32);
  else if (H <= 16) NMGP_SPEC_GO(16);
  else if (H <= 32) NMGP_SPEC_GO(8);
  else NMGP_SPEC_GO(4);
#undef NMGP_SPEC_GO
  if (rc != NMGP_OK || !sliced) return rc;
  const int blocks = (int)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
  hipLaunchKernelGGL(spectrum_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, (const double*)ws, nsl,
                     total, load2_sum);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

}  // extern "C"
