// Credible bands of the output correlations of NMGP.sample_FY (reference code/utils.py:354-366, plot_corrs: the mean
// curve and np.quantile(sampled_corrs[:, :, i, j], (0.025, 0.975), axis=0)), without the (S, N, D, D) tensor: the
// per-sample correlations of a LIST of output pairs are collected into C (P, N, ld_c), samples innermost, and the
// quantiles of every row of C are taken by an exact sort inside LDS.
//
// corr_collect: one workgroup (256 threads) per tile of 16 inputs x 16 samples and a run of the pair list.  In the
// load / compute phase thread t works on (sample t >> 4, input t & 15): the 16 lanes of a sample read 16
// consecutive inputs of one pair row, a whole 128-byte line of pair_mu / pair_sd / z_p.  The result goes through a
// 16 x 17 LDS tile (two of them, one barrier per pair) and leaves with thread t on (input t >> 4, sample t & 15):
// 16 lanes store a 128-byte run along s.  A correlation is three dot products over the rows i and j of L, at most
// D terms each; consecutive pairs of the list that share their larger index keep its cov_ii in a register (every
// pair of "all", which is in row order).  No matrix cores, no atomics: every element of C is written once.
//
// quantile_rows: a row of S values is copied into LDS, padded with +inf to a power of two P2, sorted by a bitonic
// network and interpolated.  A team of 64 (P2 <= 128), 128 (P2 = 256) or 256 threads (P2 >= 512) owns a row, so a
// workgroup of 256 threads sorts 4, 2 or 1 rows; one workgroup holds at most 16384 doubles = 128 KiB of the CU's
// 160 KiB of LDS (nmgp_quantile_rows_max_S).  NaN sorts as +inf and marks its row: all its quantiles are NaN.
#include "common.hpp"

namespace nmgp {

constexpr int kCqThreads = 256;
constexpr int kCqTile = 16;                  // inputs and samples per workgroup
constexpr int kCqMaxD = 128;
constexpr int kCqBlocksWanted = 2048;        // the pair list is cut until the grid has about this many workgroups
constexpr int kQrThreads = 256;
constexpr int kQrMaxS = 16384;
constexpr int kQrMaxQ = 32;                  // quantiles per launch (passed by value)

// pos = q (S - 1) is split on the host into lo = floor(pos) and w = pos - lo: on the device the product and
// the subtraction would contract into one fma, whose w differs from the rounded product's by up to an ulp of pos
struct QrQs {
  double w[kQrMaxQ];
  int lo[kQrMaxQ];
};

__global__ __launch_bounds__(kCqThreads) void corr_collect_kernel(
    const double* __restrict__ pair_mu, const double* __restrict__ pair_sd, int64_t ld_pair,
    const double* __restrict__ z_p, int64_t z_stride, const int32_t* __restrict__ pi,
    const int32_t* __restrict__ pj, int P, int per_chunk, int D, int N, int S, int tiles_n, double* __restrict__ C,
    int64_t ld_c, int64_t s_off) {
  __shared__ double tile[2][kCqTile][kCqTile + 1];
  const int tid = threadIdx.x;
  const int tn = blockIdx.x % tiles_n, ts = blockIdx.x / tiles_n;
  const int p0 = blockIdx.y * per_chunk, p1 = min(P, p0 + per_chunk);
  // load / compute role: lanes along n.  Inputs and samples past the end are clamped (their loads stay in
  // bounds) and never stored.
  const int nl = tid & 15, sl = tid >> 4;
  const int n = min(tn * kCqTile + nl, N - 1), s = min(ts * kCqTile + sl, S - 1);
  const double* mu = pair_mu + n;
  const double* sd = pair_sd + n;
  const double* z = z_p + (int64_t)s * z_stride + n;
  // store role: lanes along s
  const int sn = tn * kCqTile + (tid >> 4), ss = ts * kCqTile + (tid & 15);
  const bool st_ok = sn < N && ss < S;

  int held = -1;                             // the row whose cov_ii / sqrt(1 / cov_ii) are in registers
  double ca = 0.0, isa = 0.0;
  for (int p = p0; p < p1; ++p) {
    const int i = uniform32(pi[p]), j = uniform32(pj[p]);
    const int a = max(i, j), b = min(i, j);  // (i, j) and (j, i) are the same computation
    double c = __builtin_nan("");
    if (b >= 0 && a < D) {
      if (a != held) {
        const int64_t qa = (int64_t)a * (a + 1) / 2;
        ca = 0.0;
        for (int k = 0; k < a; ++k) {
          const int64_t q = qa + k;
          const double l = mu[q * ld_pair] + sd[q * ld_pair] * z[q * N];
          ca = fma(l, l, ca);
        }
        const int64_t q = qa + a;
        const double l = exp(mu[q * ld_pair] + sd[q * ld_pair] * z[q * N]);
        ca = fma(l, l, ca);
        isa = sqrt(1.0 / ca);
        held = a;
      }
      if (a == b) {
        // exactly 1 where the expression is finite; cov_ii 0, inf or NaN keeps its NaN (as fy.hip)
        c = ca * isa * isa;
        if (__builtin_isfinite(c)) c = 1.0;
      } else {
        const int64_t qa = (int64_t)a * (a + 1) / 2, qb = (int64_t)b * (b + 1) / 2;
        double cb = 0.0, cab = 0.0;
        for (int k = 0; k < b; ++k) {
          const int64_t q1 = qa + k, q2 = qb + k;
          const double la = mu[q1 * ld_pair] + sd[q1 * ld_pair] * z[q1 * N];
          const double lb = mu[q2 * ld_pair] + sd[q2 * ld_pair] * z[q2 * N];
          cb = fma(lb, lb, cb);
          cab = fma(la, lb, cab);
        }
        const int64_t q1 = qa + b, q2 = qb + b;
        const double la = mu[q1 * ld_pair] + sd[q1 * ld_pair] * z[q1 * N];
        const double lb = exp(mu[q2 * ld_pair] + sd[q2 * ld_pair] * z[q2 * N]);
        cb = fma(lb, lb, cb);
        cab = fma(la, lb, cab);
        c = cab * isa * sqrt(1.0 / cb);
        // L is zero above its diagonal, and the reference multiplies the full matrices: a non-finite L_aa or
        // L_bb meets those zeros (inf * 0) in every pair that touches its row
        if (!(__builtin_isfinite(ca) && __builtin_isfinite(cb))) c = __builtin_nan("");
      }
    }
    double(*t)[kCqTile + 1] = tile[p & 1];
    t[nl][sl] = c;
    lds_barrier();
    if (st_ok) C[((int64_t)p * N + sn) * ld_c + s_off + ss] = t[tid >> 4][tid & 15];
  }
}

// T threads per row, R = 256 / T rows per workgroup, P2 = the padded row length.
__global__ __launch_bounds__(kQrThreads) void quantile_rows_kernel(const double* __restrict__ C, int64_t rows, int S,
                                                                   int64_t ld, QrQs qs, int nq, int P2, int T,
                                                                   double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double qr_smem[];
  __shared__ int has_nan[kQrThreads / kWave];
  const int tid = threadIdx.x, R = kQrThreads / T;
  const int team = tid / T, t = tid - team * T;
  const int64_t row = (int64_t)blockIdx.x * R + team;
  const bool live = row < rows;
  double* x = qr_smem + (size_t)team * P2;
  if (t == 0) has_nan[team] = 0;
  __syncthreads();
  const double inf = __builtin_inf();
  bool bad = false;
  for (int e = t; e < P2; e += T) {
    double v = inf;
    if (live && e < S) {
      v = C[row * ld + e];
      if (v != v) {
        bad = true;
        v = inf;
      }
    }
    x[e] = v;
  }
  if (bad) has_nan[team] = 1;
  __syncthreads();
  for (int k = 2; k <= P2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int u = t; u < (P2 >> 1); u += T) {
        const int lo = ((u & ~(j - 1)) << 1) | (u & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const double a = x[lo], b = x[hi];
        if ((a > b) == up) {
          x[lo] = b;
          x[hi] = a;
        }
      }
      __syncthreads();
    }
  }
  if (live) {
    const bool nan_row = has_nan[team] != 0;
    for (int qi = t; qi < nq; qi += T) {
      const int lo = qs.lo[qi], hi = min(lo + 1, S - 1);
      const double w = qs.w[qi], a = x[lo], b = x[hi];
      double r = w < 0.5 ? a + (b - a) * w : b - (b - a) * (1.0 - w);
      if (w == 0.0) r = a;                   // an order statistic is returned as it is (also +-inf)
      if (nan_row) r = __builtin_nan("");
      out[(int64_t)qi * rows + row] = r;
    }
  }
}

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int nmgp_quantile_rows_max_S(void) { return kQrMaxS; }

int nmgp_corr_collect_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                          int64_t z_stride, const int32_t* pi, const int32_t* pj, int P, int D, int N, int S,
                          double* C, int64_t ld_c, int64_t s_off, hipStream_t stream) {
  if (D < 1 || D > kCqMaxD || P < 0 || N < 0 || S < 0 || s_off < 0) return NMGP_ERR_CORRQ_ARG;
  if (P == 0 || N == 0 || S == 0) return NMGP_OK;
  if (!pair_mu || !pair_sd || !z_p || !pi || !pj || !C) return NMGP_ERR_CORRQ_ARG;
  if (ld_pair < N || z_stride < 0 || ld_c < s_off + S) return NMGP_ERR_CORRQ_ARG;
  const int tiles_n = (N + kCqTile - 1) / kCqTile, tiles_s = (S + kCqTile - 1) / kCqTile;
  const int64_t tiles = (int64_t)tiles_n * tiles_s;
  if (tiles > 0x7fffffffLL) return NMGP_ERR_CORRQ_ARG;
  // cut the pair list only while the tiles alone leave the chip idle: a cut ends the reuse of a held row
  int64_t chunks = (kCqBlocksWanted + tiles - 1) / tiles;
  if (chunks > P) chunks = P;
  if (chunks > 65535) chunks = 65535;
  if (chunks < 1) chunks = 1;
  const int per_chunk = (int)((P + chunks - 1) / chunks);
  chunks = (P + per_chunk - 1) / per_chunk;
  hipLaunchKernelGGL(corr_collect_kernel, dim3((unsigned)tiles, (unsigned)chunks), dim3(kCqThreads), 0, stream,
                     pair_mu, pair_sd, ld_pair, z_p, z_stride, pi, pj, P, per_chunk, D, N, S, tiles_n, C, ld_c, s_off);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

int nmgp_quantile_rows_f64(const double* C, int64_t rows, int S, int64_t ld, const double* qs, int nq, double* out,
                           hipStream_t stream) {
  if (rows < 0 || S < 0 || nq < 0 || S > kQrMaxS) return NMGP_ERR_CORRQ_ARG;
  if (rows == 0 || S == 0 || nq == 0) return NMGP_OK;
  if (!C || !qs || !out || ld < S) return NMGP_ERR_CORRQ_ARG;
  for (int i = 0; i < nq; ++i)
    if (!(qs[i] >= 0.0 && qs[i] <= 1.0)) return NMGP_ERR_CORRQ_ARG;
  int P2 = 2;
  while (P2 < S) P2 <<= 1;
  const int T = P2 <= 128 ? 64 : (P2 == 256 ? 128 : 256);
  const int R = kQrThreads / T;
  const int64_t blocks = (rows + R - 1) / R;
  if (blocks > 0x7fffffffLL) return NMGP_ERR_CORRQ_ARG;
  const size_t smem = (size_t)R * P2 * sizeof(double);
  allow_dynamic_lds<quantile_rows_kernel>(kQrMaxS * sizeof(double));
  for (int q0 = 0; q0 < nq; q0 += kQrMaxQ) {
    QrQs h;
    const int cnt = nq - q0 < kQrMaxQ ? nq - q0 : kQrMaxQ;
    for (int i = 0; i < kQrMaxQ; ++i) {
      const volatile double pos = i < cnt ? qs[q0 + i] * (double)(S - 1) : 0.0;
      int lo = (int)floor(pos);
      lo = lo < 0 ? 0 : (lo > S - 1 ? S - 1 : lo);
      h.lo[i] = lo;
      h.w[i] = pos - (double)lo;
    }
    hipLaunchKernelGGL(quantile_rows_kernel, dim3((unsigned)blocks), dim3(kQrThreads), smem, stream, C, rows, S, ld,
                       h, cnt, P2, T, out + (int64_t)q0 * rows);
    NMGP_CHECK_LAUNCH();
  }
  return NMGP_OK;
}

}  // extern "C"
