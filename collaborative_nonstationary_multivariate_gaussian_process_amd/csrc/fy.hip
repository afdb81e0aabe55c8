// Fused posterior summaries of NMGP.sample_FY (reference code/nmgp_dsvi.py:492-580): per sample s and input n the
// pair samples -> L, Y = L G + noise, corr = D^-1/2 (L L^T) D^-1/2, accumulated over the samples on the device, so
// that the (S, N, D, D) correlation tensor is never stored.
//
// One workgroup (4 waves) per (input n, slice of samples).  L lives in LDS as its lower-triangular 16 x 16 tiles
// (tile (ti, tj <= ti) at slot ti (ti + 1) / 2 + tj, 2 KiB each: 72 KiB at D = 128), zero above the diagonal and in
// the rows past D.  Inside a tile element (r, c) sits at r * 16 + (c ^ ((r >> 1) << 1)): an MFMA operand read (16
// rows x 2 columns per 32-lane half, 8 bytes each) then touches 32 different 8-byte bank pairs, without padding.
// cov tile (ti, tj) = sum_{kt <= tj} L(ti, kt) L(tj, kt)^T on v_mfma_f64_16x16x4_f64, tiles above the diagonal of L
// skipped; the lower-triangular cov tiles are dealt round-robin to the waves, and each wave keeps the running
// sum and sum of squares of its tiles' correlations in registers across the slice's samples.  The sums leave the
// workgroup once: straight onto corr_sum / corr_sq when the samples are not sliced (this workgroup owns input n),
// else into a per-slice workspace that a second kernel adds up in slice order (no floating-point atomics).
#include "fy_tiles.hpp"

namespace nmgp {

template <int NT>
__global__ __launch_bounds__(kFyThreads) void fy_accum_kernel(
    const double* __restrict__ pair_mu, const double* __restrict__ pair_sd, int64_t ld_pair,
    const double* __restrict__ G, const double* __restrict__ z_p, const double* __restrict__ z_f, int64_t z_stride,
    double sd_err, int D, int N, int S, int per, double* __restrict__ Y, double* __restrict__ corr_sum,
    double* __restrict__ corr_sq, double* __restrict__ ws, int n_blocks) {
  constexpr int T = NT * (NT + 1) / 2;                  // lower-triangular tiles
  constexpr int KMAX = (T + kFyWaves - 1) / kFyWaves;   // cov tiles of one wave
  extern __shared__ __attribute__((aligned(16))) double fy_smem[];
  double* Lt = fy_smem;                                 // T tiles
  double* Gs = Lt + T * kFyTileElems;                   // NT * 16
  double* Is = Gs + NT * kFyTile;                       // NT * 16: sqrt(1 / cov_ii), 0 past D

  const int n = fy_block_input(n_blocks);
  if (n >= N) return;
  const int slice = blockIdx.y;
  const int s0 = slice * per, s1 = min(S, s0 + per);
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform32(tid >> 6);
  const int Q = D * (D + 1) / 2;

  for (int e = tid; e < T * kFyTileElems + 2 * NT * kFyTile; e += kFyThreads) fy_smem[e] = 0.0;

  f64x4 sum[KMAX], sq[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) sum[k] = sq[k] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int ar = lane & 15, ak = lane >> 4;             // MFMA operand row / k of this lane
  __syncthreads();

  for (int s = s0; s < s1; ++s) {
    // ---- pair samples -> L tiles; G column -> LDS
    fy_load_L<false>(Lt, pair_mu, pair_sd, ld_pair, z_p + (int64_t)s * z_stride + n, n, N, Q, tid, nullptr);
    if (tid < D) Gs[tid] = G[((int64_t)s * D + tid) * N + n];
    __syncthreads();

    // ---- Y row and the diagonal of cov
    {
      const int frow = tid >> 1;
      double f;
      const double c = fy_row_sums<true>(Lt, Gs, D, tid, &f);
      if (frow < D && (tid & 1) == 0) {
        const int64_t o = ((int64_t)s * N + n) * D + frow;
        Y[o] = f + sd_err * z_f[(int64_t)s * z_stride + (int64_t)n * D + frow];
        Is[frow] = sqrt(1.0 / c);
      }
    }
    __syncthreads();

    // ---- cov tiles on the matrix cores, normalised and accumulated
    // the tile coordinates are worked out again for every sample (a few scalar operations per tile): hoisted out
    // of the sample loop, the KMAX tiles' rows, columns and LDS bases stay live together and, at D > 96, no
    // longer fit the scalar registers
    int tw = wave;
    asm volatile("" : "+s"(tw));
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int t = tw + k * kFyWaves;
      if (t < T) {
        const int ti = uniform32(fy_tri_row(t));
        const int tj = t - fy_ntiles(ti);
        const double* At = Lt + fy_ntiles(ti) * kFyTileElems;
        const double* Bt = Lt + fy_ntiles(tj) * kFyTileElems;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int kt = 0; kt <= tj; ++kt) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const int o = kt * kFyTileElems + fy_tile_off(ar, kk * 4 + ak);
            acc = Mfma<double>::mma(At[o], Bt[o], acc);
          }
        }
        const double isj = Is[tj * kFyTile + (lane & 15)];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = Mfma<double>::row(lane, r);
          const double isi = Is[ti * kFyTile + row];
          // rows or columns past D: Is = 0.  The diagonal is 1, not 1 +- an ulp of rounding noise, which
          // E[c^2] - mean^2 would turn into a standard deviation of 1e-8 where it is 0 -- unless the
          // expression is not finite there (cov_ii 0, inf or NaN after an exp under / overflow): that stays.
          double c = acc[r] * isi * isj;
          if (ti == tj && row == (lane & 15) && __builtin_isfinite(c)) c = 1.0;
          sum[k][r] += c;
          sq[k][r] = fma(c, c, sq[k][r]);
        }
      }
    }
    __syncthreads();
  }

  // ---- the slice's sums leave the workgroup: lower triangle held, both triangles written
  const int64_t dd = (int64_t)D * D;
  const bool direct = gridDim.y == 1;
  double* o_sum = direct ? corr_sum + (int64_t)n * dd : ws + (((int64_t)slice * N + n) * 2) * dd;
  double* o_sq = direct ? corr_sq + (int64_t)n * dd : o_sum + dd;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int t = wave + k * kFyWaves;
    if (t < T) {
      const int ti = uniform32(fy_tri_row(t));
      const int tj = t - fy_ntiles(ti);
      const int j = tj * kFyTile + (lane & 15);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti * kFyTile + Mfma<double>::row(lane, r);
        if (i < D && j <= i) {
          const int64_t a = (int64_t)i * D + j, b = (int64_t)j * D + i;
          if (direct) {
            o_sum[a] += sum[k][r];
            o_sq[a] += sq[k][r];
            if (j < i) {
              o_sum[b] += sum[k][r];
              o_sq[b] += sq[k][r];
            }
          } else {
            o_sum[a] = sum[k][r];
            o_sq[a] = sq[k][r];
          }
        }
      }
    }
  }
}

// out_sum / out_sq += the slices' partial sums, in slice order; one thread per (n, i, j), the partials hold the
// lower triangle only.
__global__ __launch_bounds__(256) void fy_tri_reduce_kernel(const double* __restrict__ ws, int nsl, int D, int N,
                                                             double* __restrict__ out_sum,
                                                             double* __restrict__ out_sq) {
  const int64_t dd = (int64_t)D * D;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)N * dd) return;
  const int64_t n = e / dd;
  const int ij = (int)(e - n * dd), i = ij / D, j = ij - i * D;
  const int64_t src = (int64_t)max(i, j) * D + min(i, j);
  double a = 0.0, b = 0.0;
  for (int sl = 0; sl < nsl; ++sl) {
    const double* p = ws + (((int64_t)sl * N + n) * 2) * dd + src;
    a += p[0];
    b += p[dd];
  }
  out_sum[e] += a;
  out_sq[e] += b;
}

int fy_tri_reduce(const double* ws, int nsl, int D, int N, double* out_sum, double* out_sq, hipStream_t stream) {
  const int64_t total = (int64_t)N * D * D;
  hipLaunchKernelGGL(fy_tri_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ws, nsl, D, N,
                     out_sum, out_sq);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int64_t nmgp_fy_workspace_size(int D, int N, int S) { return fy_tri_workspace_bytes(D, N, S); }

int nmgp_fy_accum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* G,
                      const double* z_p, const double* z_f, int64_t z_stride, double sd_err, int D, int N, int S,
                      double* Y, double* corr_sum, double* corr_sq, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (D < 1 || D > kFyMaxD || N < 0 || S < 0) return NMGP_ERR_FY_ARG;
  if (N == 0 || S == 0) return NMGP_OK;
  if (!pair_mu || !pair_sd || !G || !z_p || !z_f || !Y || !corr_sum || !corr_sq) return NMGP_ERR_FY_ARG;
  if (ld_pair < N || z_stride < 0 || N > 0x7fffffff - kFyXcds) return NMGP_ERR_FY_ARG;
  int nsl, per;
  fy_slicing(N, S, &nsl, &per);
  if (!ws_covers(fy_tri_workspace_bytes(D, N, S), ws, ws_bytes)) return NMGP_ERR_FY_ARG;
  const int rc = fy_dispatch_nt((D + kFyTile - 1) / kFyTile, NMGP_ERR_FY_ARG, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    const size_t smem = (size_t)(fy_ntiles(NT) * kFyTileElems + 2 * NT * kFyTile) * sizeof(double);
    return fy_launch<fy_accum_kernel<NT>>(smem, N, nsl, stream, pair_mu, pair_sd, ld_pair, G, z_p, z_f, z_stride,
                                          sd_err, D, N, S, per, Y, corr_sum, corr_sq, (double*)ws);
  });
  if (rc != NMGP_OK || nsl == 1) return rc;
  return fy_tri_reduce((const double*)ws, nsl, D, N, corr_sum, corr_sq, stream);
}

}  // extern "C"
