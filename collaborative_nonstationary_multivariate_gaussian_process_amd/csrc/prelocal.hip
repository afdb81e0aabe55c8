// Local coefficient factors around the inducing points: what the reference's pre_estimation_all (code/pre_nmgp.py:64-100)
// set out to give mu_U, as one launch, one workgroup of 4 waves per inducing point z_m.
//
// Order of the rows with a finite |x_n - z_m|: the key (|x_n - z_m|, n) ascending (ties to the lower row).  The fit
// window is the first P rows of the order (bit for bit the window of preest.hip), the covariance window the next Pc
// rows (hold-out) or the first Pc rows; both are written in ascending row order.
//
// Selection: distances are non-negative doubles, so their bit patterns order as unsigned integers.  The k-th smallest
// bit pattern T is found exactly by a search over its 63 bits from the top (one workgroup count of "key < candidate"
// per bit); the rows with key < T are all in, and of the rows with key == T the lowest k - count(key < T).  One more
// pass compacts the chosen rows in ascending row order (wave ballots, the four wave counts through LDS).  The first
// selection runs over the N inputs in global memory with k = P holdout + Pc, the second over the chosen rows in LDS
// with k = P and splits them into the two windows.  Nothing is kept per thread, so the window may hold 1024 rows.
//
// Covariance: S = Y_w^T Y_w of the Pc covariance rows on v_mfma_f64_16x16x4_f64.  The rows are staged through LDS in
// ascending row order, 32 at a time and zero padded, and taken four per MFMA step; the lower 16 x 16 tiles of S are
// dealt to the waves round-robin (36 tiles at D = 128: 9 accumulators of 8 VGPRs a wave) and stay in registers for
// the whole window.  The order is fixed: a window's bits do not depend on the launch or on the other windows.
// B_m = w S + alpha B (one multiply each, one fused add) is taken from the lower triangle and stored symmetric.
//
// Factor: a right-looking column Cholesky on the packed lower triangle in LDS (fp64 VALU, stored l_ij used in every
// update, so |L L^T - B_m| <= gamma_{D+1} |L| |L^T| holds as for the textbook algorithm; no inverted diagonal tile).
// A pivot that is not positive sets the factor flag: L of that window is NaN, the other windows are unaffected.
//
// LDS: the packed triangle (<= 8256 doubles, 64.5 KiB) next to the row staging (32 x <= 144 doubles, 36 KiB), both
// dynamic; the selected rows' keys and indices and the two windows (static, 17 KiB).
#include <math.h>

#include "fy_tiles.hpp"

namespace nmgp {

constexpr int kPlThreads = 256, kPlWaves = kPlThreads / kWave, kPlMinP = 3, kPlMaxP = 32, kPlMaxD = 128;
constexpr int kPlMaxCov = 1024, kPlMaxSel = kPlMaxCov + kPlMaxP, kPlChunk = 32, kPlSlots = 9;
constexpr int kPlFlagDegenerate = 32, kPlFlagFactor = 64;
constexpr unsigned long long kPlInfBits = 0x7ff0000000000000ull;
static_assert(kPlSlots * kPlWaves >= (kPlMaxD / 16) * (kPlMaxD / 16 + 1) / 2, "every lower tile has a slot");

struct PlShared {
  unsigned long long skey[kPlMaxSel];
  int sidx[kPlMaxSel];
  int cov[kPlMaxCov];
  int fit[kPlMaxP];
  int wa[kPlWaves], wb[kPlWaves];
};

__host__ __device__ inline int pl_stage_ld(int Dp) { return (Dp & 31) == 16 ? Dp : Dp + 16; }
__host__ __device__ inline int pl_packed(int D) { return (D * (D + 1) / 2 + 1) & ~1; }

__device__ inline int pl_block_count(PlShared& s, int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s.wa[threadIdx.x >> 6] = v;
  __syncthreads();
  return s.wa[0] + s.wa[1] + s.wa[2] + s.wa[3];
}

// The k smallest of the n keys key(i) (ties to the lower i): emit(i, key, chosen, pos) for every i, pos the number of
// chosen entries before i.  False, and nothing emitted, when fewer than k keys are finite.
template <class KeyFn, class Emit>
__device__ bool pl_select(PlShared& s, int n, int k, KeyFn key, Emit emit) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  auto below = [&](unsigned long long t) {
    int c = 0;
    for (int i = tid; i < n; i += kPlThreads) c += key(i) < t ? 1 : 0;
    return pl_block_count(s, c);
  };
  if (below(kPlInfBits) < k) return false;
  unsigned long long T = 0;                                     // the largest T with fewer than k keys below it
  for (int bit = 62; bit >= 0; --bit) {
    const unsigned long long cand = T | (1ull << bit);
    if (below(cand) < k) T = cand;
  }
  const int need = k - below(T);                                // of the keys equal to T, the first `need`
  __syncthreads();
  const unsigned long long lower = (1ull << lane) - 1ull;
  int tie_base = 0, sel_base = 0;
  for (int base = 0; base < n; base += kPlThreads) {
    const int i = base + tid;
    const unsigned long long kk = i < n ? key(i) : ~0ull;
    const bool lt = kk < T, eq = kk == T;
    const unsigned long long be = __ballot(eq);
    if (lane == 0) s.wa[w] = __popcll(be);
    __syncthreads();
    int tr = tie_base + __popcll(be & lower);
    for (int q = 0; q < w; ++q) tr += s.wa[q];
    tie_base += s.wa[0] + s.wa[1] + s.wa[2] + s.wa[3];
    const bool chosen = lt || (eq && tr < need);
    const unsigned long long bs = __ballot(chosen);
    if (lane == 0) s.wb[w] = __popcll(bs);
    __syncthreads();
    int pos = sel_base + __popcll(bs & lower);
    for (int q = 0; q < w; ++q) pos += s.wb[q];
    sel_base += s.wb[0] + s.wb[1] + s.wb[2] + s.wb[3];
    if (i < n) emit(i, kk, chosen, pos);
  }
  __syncthreads();
  return true;
}

struct PlOut {
  double *B_local, *L, *xs, *Yloc;
  int *nbr, *cov, *flags;
};

__global__ __launch_bounds__(kPlThreads) void prelocal_kernel(
    const double* __restrict__ x, int64_t x_stride, const double* __restrict__ Y, int64_t ld_y,
    const double* __restrict__ B, int64_t ld_b, const double* __restrict__ z, int64_t z_stride, int N, int D, int P,
    int Pc, int holdout, double w, double alpha, PlOut o) {
  extern __shared__ __attribute__((aligned(16))) double pl_smem[];
  __shared__ PlShared s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ar = lane & 15, ak = lane >> 4;
  const int mwin = blockIdx.x, DD = D * D;
  const int nt = (D + kFyTile - 1) / kFyTile, Dp = nt * kFyTile, ldS = pl_stage_ld(Dp), T = fy_ntiles(nt);
  double* Lp = pl_smem;                                         // packed lower triangle: (i, j) at i (i + 1) / 2 + j
  double* stage = Lp + pl_packed(D);                            // kPlChunk rows of ldS
  const double nan = __builtin_nan("");
  const double zm = z[(int64_t)mwin * z_stride];
  const int K = (holdout ? P : 0) + Pc;
  double* oB = o.B_local + (int64_t)mwin * DD;
  double* oL = o.L + (int64_t)mwin * DD;
  double* oY = o.Yloc + (int64_t)mwin * P * D;

  // ---- 1. the first K rows of the order, ascending by row, then the two windows
  const bool enough = pl_select(
      s, N, K,
      [&](int i) {
        const double d = fabs(x[(int64_t)i * x_stride] - zm);
        return d < INFINITY ? (unsigned long long)__double_as_longlong(d) : kPlInfBits;
      },
      [&](int i, unsigned long long kk, bool chosen, int pos) {
        if (chosen && pos < K) {
          s.sidx[pos] = i;
          s.skey[pos] = kk;
        }
      });
  if (!enough) {
    for (int e = tid; e < DD; e += kPlThreads) {
      oB[e] = nan;
      oL[e] = nan;
    }
    for (int e = tid; e < P * D; e += kPlThreads) oY[e] = nan;
    if (tid < P) {
      o.nbr[(int64_t)mwin * P + tid] = -1;
      o.xs[(int64_t)mwin * P + tid] = nan;
    }
    for (int e = tid; e < Pc; e += kPlThreads) o.cov[(int64_t)mwin * Pc + e] = -1;
    if (tid == 0) o.flags[mwin] = kPlFlagDegenerate;
    return;
  }
  pl_select(
      s, K, P, [&](int i) { return s.skey[i]; },
      [&](int i, unsigned long long, bool chosen, int pos) {
        if (chosen) {
          if (pos < P) s.fit[pos] = s.sidx[i];
          if (!holdout) s.cov[i] = s.sidx[i];
        } else if (holdout) {
          if (i - pos < Pc) s.cov[i - pos] = s.sidx[i];
        } else {
          s.cov[i] = s.sidx[i];
        }
      });
  if (tid < P) {
    o.nbr[(int64_t)mwin * P + tid] = s.fit[tid];
    o.xs[(int64_t)mwin * P + tid] = x[(int64_t)s.fit[tid] * x_stride];
  }
  for (int e = tid; e < Pc; e += kPlThreads) o.cov[(int64_t)mwin * Pc + e] = s.cov[e];
  for (int e = tid; e < P * D; e += kPlThreads) {
    const int p = e / D, d = e - p * D;
    oY[e] = Y[(int64_t)s.fit[p] * ld_y + d];
  }

  // ---- 2. the lower tiles of Y_w^T Y_w on the matrix cores, accumulators in registers
  f64x4 acc[kPlSlots];
  int ti[kPlSlots], tj[kPlSlots];
#pragma unroll
  for (int k = 0; k < kPlSlots; ++k) {
    acc[k] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int t = min(wave + k * kPlWaves, T - 1);
    ti[k] = uniform32(fy_tri_row(t));
    tj[k] = uniform32(t - fy_ntiles(ti[k]));
  }
  for (int c0 = 0; c0 < Pc; c0 += kPlChunk) {
    const int rows = min(kPlChunk, Pc - c0), rows4 = (rows + 3) & ~3;
    __syncthreads();                                            // the last chunk has been read
    for (int e = tid; e < rows4 * Dp; e += kPlThreads) {
      const int r = e / Dp, d = e - r * Dp;
      double v = 0.0;
      if (r < rows && d < D) v = Y[(int64_t)s.cov[c0 + r] * ld_y + d];
      stage[r * ldS + d] = v;
    }
    __syncthreads();
    for (int k4 = 0; k4 < rows4; k4 += 4) {
      const double* rowp = stage + (k4 + ak) * ldS + ar;        // A[i][k] = Y[k][16 ti + i], B[k][j] = Y[k][16 tj + j]
#pragma unroll
      for (int k = 0; k < kPlSlots; ++k)
        if (wave + k * kPlWaves < T)
          acc[k] = Mfma<double>::mma(rowp[ti[k] * kFyTile], rowp[tj[k] * kFyTile], acc[k]);
    }
  }

  // ---- 3. B_m = w S + alpha B from the lower triangle, stored symmetric; its packed copy for the factorization
#pragma unroll
  for (int k = 0; k < kPlSlots; ++k) {
    if (wave + k * kPlWaves < T) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = ti[k] * kFyTile + Mfma<double>::row(lane, r), j = tj[k] * kFyTile + ar;
        if (i < D && j <= i) {
          const double b = fma(w, acc[k][r], __dmul_rn(alpha, B[(int64_t)i * ld_b + j]));
          Lp[i * (i + 1) / 2 + j] = b;
          oB[i * D + j] = b;
          oB[j * D + i] = b;
        }
      }
    }
  }

  // ---- 4. right-looking Cholesky of the packed triangle
  bool bad = false;
  for (int j = 0; j < D; ++j) {
    __syncthreads();
    const int cj = j * (j + 1) / 2 + j;
    const double piv = Lp[cj];
    if (!(piv > 0.0 && piv < INFINITY)) {
      bad = true;
      break;
    }
    const double rt = sqrt(piv);
    __syncthreads();                                            // everybody holds the pivot
    for (int i = j + tid; i < D; i += kPlThreads) {
      const int q = i * (i + 1) / 2 + j;
      Lp[q] = i == j ? rt : Lp[q] / rt;
    }
    __syncthreads();
    const int rem = D - 1 - j, tot = rem * (rem + 1) / 2;
    for (int q = tid; q < tot; q += kPlThreads) {
      const int a = fy_tri_row(q), c = q - a * (a + 1) / 2;
      const int i = j + 1 + a, cc = j + 1 + c, ri = i * (i + 1) / 2;
      Lp[ri + cc] = fma(-Lp[ri + j], Lp[cc * (cc + 1) / 2 + j], Lp[ri + cc]);
    }
  }
  __syncthreads();
  for (int e = tid; e < DD; e += kPlThreads) {
    const int i = e / D, j = e - i * D;
    oL[e] = bad ? nan : (j <= i ? Lp[i * (i + 1) / 2 + j] : 0.0);
  }
  if (tid == 0) o.flags[mwin] = bad ? kPlFlagFactor : 0;
}

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int nmgp_pre_local_factor_f64(const double* x, int64_t x_stride, const double* Y, int64_t ld_y, const double* B,
                              int64_t ld_b, const double* z, int64_t z_stride, int N, int D, int M, int P,
                              int cov_rows, int holdout, double w, double alpha, double* B_local, double* L,
                              int32_t* neighbours, int32_t* cov_neighbours, double* xs, double* Yloc, int32_t* flags,
                              hipStream_t stream) {
  if (P < kPlMinP || P > kPlMaxP || D < 1 || D > kPlMaxD || M < 0) return NMGP_ERR_PRELOCAL_ARG;
  if (cov_rows < P || cov_rows > kPlMaxCov || (holdout != 0 && holdout != 1)) return NMGP_ERR_PRELOCAL_ARG;
  if ((int64_t)P * holdout + cov_rows > (int64_t)N) return NMGP_ERR_PRELOCAL_ARG;
  if (!(alpha >= 0.0 && alpha <= 1.0) || !(w >= 0.0 && w < INFINITY)) return NMGP_ERR_PRELOCAL_ARG;
  if (!x || !Y || !B || !z || !B_local || !L || !neighbours || !cov_neighbours || !xs || !Yloc || !flags)
    return NMGP_ERR_PRELOCAL_ARG;
  if (x_stride < 1 || z_stride < 1 || ld_y < D || ld_b < D) return NMGP_ERR_PRELOCAL_ARG;
  const int64_t lim = 0x7fffffffLL;
  if ((int64_t)(N - 1) * x_stride > lim || (int64_t)N * ld_y > lim || (int64_t)M * cov_rows > lim ||
      (int64_t)M * D * D > lim || (int64_t)M * P * D > lim)
    return NMGP_ERR_PRELOCAL_ARG;
  if (M > 0 && (int64_t)(M - 1) * z_stride > lim) return NMGP_ERR_PRELOCAL_ARG;
  if (M == 0) return NMGP_OK;
  allow_dynamic_lds<prelocal_kernel>(
      (size_t)(pl_packed(kPlMaxD) + kPlChunk * pl_stage_ld(kPlMaxD)) * sizeof(double));
  const int Dp = (D + kFyTile - 1) / kFyTile * kFyTile;
  const size_t smem = (size_t)(pl_packed(D) + kPlChunk * pl_stage_ld(Dp)) * sizeof(double);
  PlOut o{B_local, L, xs, Yloc, (int*)neighbours, (int*)cov_neighbours, (int*)flags};
  hipLaunchKernelGGL(prelocal_kernel, dim3((unsigned)M), dim3(kPlThreads), smem, stream, x, x_stride, Y, ld_y, B, ld_b,
                     z, z_stride, N, D, P, cov_rows, holdout, w, alpha, o);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

}  // extern "C"
