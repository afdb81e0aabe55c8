// Fused held-out summaries of NMGP.sample_Y (reference code/nmgp_dsvi.py:406-490): input n belongs to one output
// I_n, so a sample needs only row I_n of L -- the I_n + 1 pairs q = I_n (I_n + 1) / 2 + j, j <= I_n -- and the
// (S, D, D, N) tensor of all pairs that predict.sample_Y fills and then gathers one row from is never built.
//
// Every operand ((Q, N) pair marginals, (S, Q N) pair noise, (S, D, N) G, (S, N) F) is unit-stride in n, so lanes
// run along n everywhere: a wave reads 512 contiguous bytes per load.  Two passes on the stream:
//   rows     one thread per (input n, sample s), 64 inputs x 4 samples per workgroup: the fma chain over j <= I_n
//            -> F[s, n], Y[s, n].  Four independent loads per j, nothing carried but the chain itself.
//   moments  one thread per (input n, row r), 64 inputs x 4 rows per workgroup, looping over the samples in order
//            with its sums in registers: r < D gives G_sum / G_sq [r, n] and, where r <= I_n, L_sum / L_sq [n, r]
//            (the pair sample is formed again: two loads and one fma); r == D reads the F the first pass wrote
//            and gives F_sum / F_sq [n] and the running log-sum-exp of the log densities of y_n.
// A thread owns its outputs, so the sums are added in place without atomics and in sample order.  When
// ceil(N / 64) (D + 1) waves cannot fill the chip the samples are cut into slices (grid z); a slice's sums go to
// the workspace and a third kernel adds them up in slice order onto the outputs.
#include <math.h>

#include "common.hpp"
#include "lse_state.hpp"

namespace nmgp {

constexpr int kYLanes = 64;      // inputs per workgroup: one wave along n
constexpr int kYRows = 4;        // waves per workgroup: samples (rows pass) or rows of the moments
constexpr int kYFill = 1024;     // waves the moments pass wants in flight: one per SIMD
constexpr int kYMaxGridY = 65535;

// Sample slices of the moments pass: none once the (input tile, row) waves alone pass half the fill, else as many
// as reach it, at most one per sample.  Non-decreasing in S, so the workspace of a full chunk covers a shorter one.
static int y_slices(int D, int N, int S) {
  const int64_t waves = (int64_t)((N + kYLanes - 1) / kYLanes) * ((int64_t)D + 1);
  int64_t want = waves > kYFill / 2 ? 1 : kYFill / waves;
  if (want > S) want = S;
  return (int)(want < 1 ? 1 : want);
}

__global__ __launch_bounds__(kYLanes* kYRows) void y_rows_kernel(
    const double* __restrict__ pair_mu, const double* __restrict__ pair_sd, int64_t ld_pair,
    const double* __restrict__ G, const double* __restrict__ z_p, const double* __restrict__ z_f, int64_t z_stride,
    const int64_t* __restrict__ I, double sd_err, int D, int N, int S, double* __restrict__ Y,
    double* __restrict__ F) {
  const int64_t n = (int64_t)blockIdx.x * kYLanes + threadIdx.x;
  const int64_t s = (int64_t)blockIdx.y * kYRows + threadIdx.y;
  if (n >= N || s >= S) return;
  const int64_t i = I[n];
  double f = __builtin_nan(""), y = f;                  // an id outside 0..D-1 indexes nothing
  if (i >= 0 && i < D) {
    const int64_t q0 = i * (i + 1) / 2;
    const double* mu = pair_mu + q0 * ld_pair + n;
    const double* sd = pair_sd + q0 * ld_pair + n;
    const double* zp = z_p + s * z_stride + q0 * N + n;
    const double* g = G + s * D * N + n;
    f = 0.0;
#pragma unroll 4
    for (int64_t j = 0; j < i; ++j) f = fma(fma(sd[j * ld_pair], zp[j * N], mu[j * ld_pair]), g[j * N], f);
    f = fma(exp(fma(sd[i * ld_pair], zp[i * N], mu[i * ld_pair])), g[i * N], f);
    y = fma(sd_err, z_f[s * z_stride + n], f);
  }
  F[s * N + n] = f;
  Y[s * N + n] = y;
}

struct YOut {
  double *F_sum, *F_sq, *L_sum, *L_sq, *G_sum, *G_sq, *lse_max, *lse_sum;
};

// The four sums of thread (n, row) over some samples, added onto the outputs.  row < D: (G_sum, G_sq, L_sum,
// L_sq), the L pair only where row <= I_n (or NaN where I_n is no id); row == D: (F_sum, F_sq, lse max, lse sum).
__device__ inline void y_emit(const YOut& o, bool scored, int64_t n, int row, int D, int N, bool l_row, double v0,
                              double v1, double v2, double v3) {
  if (row < D) {
    o.G_sum[(int64_t)row * N + n] += v0;
    o.G_sq[(int64_t)row * N + n] += v1;
    if (l_row) {
      o.L_sum[n * D + row] += v2;
      o.L_sq[n * D + row] += v3;
    }
  } else {
    o.F_sum[n] += v0;
    o.F_sq[n] += v1;
    if (scored) {
      double m, r;
      y_lse_combine(o.lse_max[n], o.lse_sum[n], v2, v3, &m, &r);
      o.lse_max[n] = m;
      o.lse_sum[n] = r;
    }
  }
}

__global__ __launch_bounds__(kYLanes* kYRows) void y_moments_kernel(
    const double* __restrict__ pair_mu, const double* __restrict__ pair_sd, int64_t ld_pair,
    const double* __restrict__ G, const double* __restrict__ z_p, int64_t z_stride, const int64_t* __restrict__ I,
    const double* __restrict__ y, const double* __restrict__ F, double v, double c0, int D, int N, int S, YOut o,
    double* __restrict__ ws) {
  const int64_t n = (int64_t)blockIdx.x * kYLanes + threadIdx.x;
  const int row = blockIdx.y * kYRows + threadIdx.y;
  if (n >= N || row > D) return;
  const int nsl = gridDim.z, slice = blockIdx.z;
  const int64_t s0 = (int64_t)slice * S / nsl, s1 = (int64_t)(slice + 1) * S / nsl;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  bool l_row = false;
  if (row < D) {
    const int64_t i = I[n];
    const bool bad = i < 0 || i >= D, act = !bad && row <= i;
    l_row = bad || act;
    const double* g = G + (int64_t)row * N + n;
    const int64_t g_stride = (int64_t)D * N;
    if (act) {
      const int64_t q = i * (i + 1) / 2 + row;
      const double mu = pair_mu[q * ld_pair + n], sd = pair_sd[q * ld_pair + n];
      const double* zp = z_p + q * N + n;
      const bool diag = row == i;
#pragma unroll 4
      for (int64_t s = s0; s < s1; ++s) {
        const double gv = g[s * g_stride];
        double l = fma(sd, zp[s * z_stride], mu);
        if (diag) l = exp(l);
        v0 += gv;
        v1 = fma(gv, gv, v1);
        v2 += l;
        v3 = fma(l, l, v3);
      }
    } else {
#pragma unroll 8
      for (int64_t s = s0; s < s1; ++s) {
        const double gv = g[s * g_stride];
        v0 += gv;
        v1 = fma(gv, gv, v1);
      }
      if (bad) v2 = v3 = __builtin_nan("");
    }
  } else {
    const bool scored = y != nullptr;
    const double yn = scored ? y[n] : 0.0;
    v2 = -INFINITY;                                      // (v2, v3): the slice's own log-sum-exp state
#pragma unroll 4
    for (int64_t s = s0; s < s1; ++s) {
      const double fv = F[s * N + n];
      v0 += fv;
      v1 = fma(fv, fv, v1);
      if (scored) {
        const double d = yn - fv;
        const double a = c0 - d * d / (2.0 * v);
        if (a != a || v2 != v2) {
          v2 = v3 = __builtin_nan("");
        } else if (a > v2) {
          v3 = v3 * exp(v2 - a) + 1.0;
          v2 = a;
        } else if (a != -INFINITY) {
          v3 += exp(a - v2);
        }
      }
    }
  }
  if (nsl == 1) {
    y_emit(o, y != nullptr, n, row, D, N, l_row, v0, v1, v2, v3);
  } else {
    const int64_t plane = ((int64_t)D + 1) * N;
    double* w = ws + (int64_t)slice * 4 * plane + (int64_t)row * N + n;
    w[0] = v0;
    w[plane] = v1;
    w[2 * plane] = v2;
    w[3 * plane] = v3;
  }
}

// outputs += the slices' sums, in slice order; thread (n, row) as in the moments pass.
__global__ __launch_bounds__(kYLanes* kYRows) void y_combine_kernel(const double* __restrict__ ws, int nsl,
                                                                    const int64_t* __restrict__ I, bool scored,
                                                                    int D, int N, YOut o) {
  const int64_t n = (int64_t)blockIdx.x * kYLanes + threadIdx.x;
  const int row = blockIdx.y * kYRows + threadIdx.y;
  if (n >= N || row > D) return;
  const int64_t plane = ((int64_t)D + 1) * N;
  const double* w = ws + (int64_t)row * N + n;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  bool l_row = false;
  if (row < D) {
    const int64_t i = I[n];
    l_row = i < 0 || i >= D || row <= i;
  } else {
    v2 = -INFINITY;
  }
  for (int sl = 0; sl < nsl; ++sl, w += 4 * plane) {
    v0 += w[0];
    v1 += w[plane];
    if (row < D) {
      v2 += w[2 * plane];
      v3 += w[3 * plane];
    } else if (scored) {
      y_lse_combine(v2, v3, w[2 * plane], w[3 * plane], &v2, &v3);
    }
  }
  y_emit(o, scored, n, row, D, N, l_row, v0, v1, v2, v3);
}

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int64_t nmgp_y_workspace_size(int D, int N, int S) {
  if (D < 1 || N <= 0 || S <= 0) return 0;
  const int nsl = y_slices(D, N, S);
  return nsl == 1 ? 0 : (int64_t)nsl * 4 * ((int64_t)D + 1) * N * (int64_t)sizeof(double);
}

int nmgp_y_accum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* G,
                     const double* z_p, const double* z_f, int64_t z_stride, const int64_t* I, const double* y,
                     double sd_err, int D, int N, int S, double* Y, double* F, double* F_sum, double* F_sq,
                     double* L_sum, double* L_sq, double* G_sum, double* G_sq, double* lse_max, double* lse_sum,
                     void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (D < 1 || N < 0 || S < 0) return NMGP_ERR_Y_ARG;
  if (N == 0 || S == 0) return NMGP_OK;
  if (!pair_mu || !pair_sd || !G || !z_p || !z_f || !I || !Y || !F || !F_sum || !F_sq || !L_sum || !L_sq ||
      !G_sum || !G_sq)
    return NMGP_ERR_Y_ARG;
  if (y && (!lse_max || !lse_sum)) return NMGP_ERR_Y_ARG;
  if (ld_pair < N || z_stride < 0) return NMGP_ERR_Y_ARG;
  // the samples (rows pass) and the D + 1 rows (moments pass) are dealt four to a workgroup along grid y
  if (S > kYRows * kYMaxGridY || D > kYRows * kYMaxGridY - 1) return NMGP_ERR_Y_ARG;
  const int nsl = y_slices(D, N, S);
  if (!ws_covers(nmgp_y_workspace_size(D, N, S), ws, ws_bytes)) return NMGP_ERR_Y_ARG;

  const dim3 block(kYLanes, kYRows);
  const unsigned tiles = (unsigned)((N + kYLanes - 1) / kYLanes);
  hipLaunchKernelGGL(y_rows_kernel, dim3(tiles, (unsigned)((S + kYRows - 1) / kYRows)), block, 0, stream, pair_mu,
                     pair_sd, ld_pair, G, z_p, z_f, z_stride, I, sd_err, D, N, S, Y, F);
  NMGP_CHECK_LAUNCH();
  const YOut o = {F_sum, F_sq, L_sum, L_sq, G_sum, G_sq, lse_max, lse_sum};
  const double v = sd_err * sd_err;
  const double c0 = -0.5 * log(2.0 * M_PI * v);
  const unsigned row_blocks = (unsigned)((D + 1 + kYRows - 1) / kYRows);
  hipLaunchKernelGGL(y_moments_kernel, dim3(tiles, row_blocks, (unsigned)nsl), block, 0, stream, pair_mu, pair_sd,
                     ld_pair, G, z_p, z_stride, I, y, (const double*)F, v, c0, D, N, S, o, (double*)ws);
  NMGP_CHECK_LAUNCH();
  if (nsl > 1) {
    hipLaunchKernelGGL(y_combine_kernel, dim3(tiles, row_blocks), block, 0, stream, (const double*)ws, nsl, I,
                       y != nullptr, D, N, o);
    NMGP_CHECK_LAUNCH();
  }
  return NMGP_OK;
}

}  // extern "C"
