// Conditional prediction of the missing outputs at an input from the outputs observed there, per posterior sample,
// fused like the partial correlations of pcorr.hip: the (S, N, D, D) tensor is never stored.  The reference has no
// such code; the quantity is a pure function of what NMGP.sample_FY samples (reference code/nmgp_dsvi.py:519-569).
//
// Given the sample, y(x_n) ~ N(L mu_g, L V L^T + s2 I) with V = diag(var_g + 1e-4): the latent G is integrated out.
// Row n of Y_obs has observed (finite) and missing entries.  In the latent space
//   A = V^-1 + L^T diag(w) L  (w_o = 1 / s2 where observed, else 0),  b = V^-1 mu_g + L^T (w o y),
//   A = R R^T,  c = R^-1 b,  w_h = R^-1 l_h  (l_h = row h of L as a column),  mu_h = w_h^T c,  v_h = |w_h|^2 + s2
// for every missing h.  A is D x D and positive definite whatever the mask, so the mask is a row weight only.
//
// One workgroup (4 waves) per (input n, slice of samples), L and A side by side in LDS in the tile layout of
// fy_tiles.hpp (2 x 72 KiB at D = 128) plus five D-vectors and the list of missing outputs (5.5 KiB): 149.5 KiB of
// the CU's 160 KiB at D = 128.  A row without a missing entry returns at once.  Per sample:
//   1. pair samples -> L tiles (fy_load_L with its bad-diagonal flag), V^-1 and mu_g -> LDS.
//   2. A's lower tiles on v_mfma_f64_16x16x4_f64, tile (ti, tj <= ti) = sum_{kt >= ti} L(kt, ti)^T diag(w) L(kt, tj)
//      with w folded into the A operand (the operand pattern of Omega in pcorr.hip), tiles dealt round-robin; V^-1
//      on the diagonal, 1 on the diagonal past D; b by two threads per column.
//   3. Tiled Cholesky in place, left-looking, column block k: wave 0 updates the diagonal tile, factors it in
//      registers (lane = row of the full symmetric tile, the pivot row read with v_readlane), inverts the factor by
//      substitution (lane = column) and writes the INVERSE W_kk over the tile; waves 1-3 meanwhile form the updated
//      transposed tiles T^T = A(i, k)^T - sum_{m < k} R(k, m) R(i, m)^T in accumulator registers; after a barrier
//      they multiply, R(i, k)^T = W_kk T^T, the accumulator registers fed back as the B operand (k order of the C
//      layout, as pcorr.hip), and store R(i, k).  Two barriers per column block.
//   4. Forward solves: right-hand sides in blocks of 16 columns, 15 rows l_h and b as the 16th column of EVERY
//      block, so that c sits in lane 15 of each 16-lane group and mu = w_h^T c needs shuffles only.  A block lives
//      in one wave's accumulator registers (NT tiles x 4 doubles per lane), block j on wave j & 3, no barrier in the
//      phase.  X(ti) = W(ti, ti) (B(ti) - sum_{k < ti} R(ti, k) X(k)), all on the matrix cores.
// The serial part is the diagonal tile's factorization and inversion on wave 0 (16 dependent sqrt / reciprocal
// steps and two 120-long fma chains per column block); the waves 1-3 hide their updates behind it.
//
// The sums of an entry stay in the registers of the lane that owns it across the slice's samples and leave the
// workgroup once: onto the outputs when the samples are not sliced, else into the per-slice workspace that a second
// kernel adds up in slice order.  No floating-point atomics.
#include "fy_tiles.hpp"
#include "lse_state.hpp"

namespace nmgp {

constexpr int kYcRhs = 15;          // rows l_h per right-hand-side block; the 16th column is b
constexpr int kYcWs = 5;            // workspace words per (slice, entry): three sums and the lse state

__device__ inline double yc_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

struct YcOut {
  double *mu_sum, *y2_sum, *f2_sum, *lse_max, *lse_sum, *Mu, *Var;
  const double* y_true;
};

template <int NT>
__global__ __launch_bounds__(kFyThreads) void ycond_accum_kernel(
    const double* __restrict__ pair_mu, const double* __restrict__ pair_sd, int64_t ld_pair,
    const double* __restrict__ z_p, int64_t z_stride, const double* __restrict__ mu_g,
    const double* __restrict__ var_g, const double* __restrict__ Y_obs, double s2, int D, int N, int S, int per,
    const int32_t* __restrict__ e_off, int E, YcOut o, int64_t s_off, double* __restrict__ ws, int n_blocks) {
  constexpr int T = NT * (NT + 1) / 2;                          // lower-triangular tiles
  constexpr int NP = NT * kFyTile;                              // padded D
  constexpr int KMAX = (T + kFyWaves - 1) / kFyWaves;           // A tiles of one wave
  constexpr int JMAX = NT > 1 ? (NT + 1) / 3 : 1;               // panel tiles of one of the waves 1-3
  constexpr int NB = (NP + kYcRhs - 1) / kYcRhs;                // right-hand-side blocks at |H| = NP
  constexpr int KB = (NB + kFyWaves - 1) / kFyWaves;            // blocks of one wave
  extern __shared__ __attribute__((aligned(16))) double yc_smem[];
  double* Lt = yc_smem;                                         // T tiles: L
  double* At = Lt + T * kFyTileElems;                           // T tiles: A, then its factor (diagonal: inverse)
  double* vinv = At + T * kFyTileElems;                         // NP: 1 / (var_g + 1e-4), 0 past D
  double* mug = vinv + NP;                                      // NP: mu_g
  double* wv = mug + NP;                                        // NP: 1 / s2 where observed, else 0
  double* wy = wv + NP;                                         // NP: w o y (0 where missing)
  double* bv = wy + NP;                                         // NP: b, 0 past D
  int* hl = (int*)(bv + NP);                                    // NP: the missing outputs of this row, ascending
  int* flags = hl + NP;                                         // [0], [1]: bad sample by parity; [2]: |H|

  const int n = fy_block_input(n_blocks);
  if (n >= N) return;
  // offsets clamped to 0..E and made monotone: no table can make the kernel leave its buffers
  const int e0 = min(max(e_off[n], 0), E);
  const int e1 = min(max(e_off[n + 1], e0), E);
  if (e1 == e0) return;                                         // nothing missing at this input
  const int slice = blockIdx.y;
  const int s0 = slice * per, s1 = min(S, s0 + per);
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform32(tid >> 6);
  const int Q = D * (D + 1) / 2;
  const int ar = lane & 15, ak = lane >> 4;                     // MFMA operand row / k of this lane
  const double nan = __builtin_nan("");

  for (int e = tid; e < 2 * T * kFyTileElems + 5 * NP; e += kFyThreads) yc_smem[e] = 0.0;
  if (tid < 3) flags[tid] = 0;
  __syncthreads();
  if (tid < D) {
    const double y = Y_obs[(int64_t)n * D + tid];
    const bool obs = __builtin_isfinite(y);
    wv[tid] = obs ? 1.0 / s2 : 0.0;
    wy[tid] = obs ? y / s2 : 0.0;
  }
  if (tid == 0) {                                               // the list of the missing outputs, once per row
    int c = 0;
    for (int d = 0; d < D; ++d)
      if (!__builtin_isfinite(Y_obs[(int64_t)n * D + d])) hl[c++] = d;
    flags[2] = c;
  }
  __syncthreads();
  // the entry table and the mask must agree; where they do not, the smaller count holds
  const int nH = uniform32(min(flags[2], e1 - e0));
  const int nB = (nH + kYcRhs - 1) / kYcRhs;

  // the entries this lane owns: block wave + 4 kb, column ar < 15, held by the lanes 0..14 of the wave
  double sm[KB], sy[KB], sf[KB], lm[KB], lr[KB], yt[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    sm[kb] = sy[kb] = sf[kb] = lr[kb] = 0.0;
    lm[kb] = -INFINITY;
    yt[kb] = nan;
    const int ci = (wave + kb * kFyWaves) * kYcRhs + ar;
    if (o.y_true && lane < kYcRhs && ci < nH) yt[kb] = o.y_true[e0 + ci];
  }

  for (int s = s0; s < s1; ++s) {
    // ---- 1. pair samples -> L tiles; V^-1, mu_g
    fy_load_L<true>(Lt, pair_mu, pair_sd, ld_pair, z_p + (int64_t)s * z_stride + n, n, N, Q, tid, &flags[s & 1]);
    if (tid < D) {
      const int64_t g = ((int64_t)s * N + n) * D + tid;
      const double v = var_g[g] + 1e-4;
      if (!(__builtin_isfinite(v) && v > 0.0)) flags[s & 1] = 1;
      vinv[tid] = 1.0 / v;
      mug[tid] = mu_g[g];
    }
    if (tid == 0) flags[(s + 1) & 1] = 0;                       // last read before the barrier that ended sample s - 1
    __syncthreads();
    const bool bad = flags[s & 1] != 0;

    // ---- 2. A tiles on the matrix cores; b
    int tw = wave;
    asm volatile("" : "+s"(tw));                                // tile coordinates recomputed per sample, as fy.hip
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int t = tw + k * kFyWaves;
      if (t < T) {
        const int ti = uniform32(fy_tri_row(t));
        const int tj = t - fy_ntiles(ti);
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int kt = ti; kt < NT; ++kt) {
          const double* Ai = Lt + (fy_ntiles(kt) + ti) * kFyTileElems;
          const double* Bj = Lt + (fy_ntiles(kt) + tj) * kFyTileElems;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const int off = fy_tile_off(kk * 4 + ak, ar);
            acc = Mfma<double>::mma(Ai[off] * wv[kt * kFyTile + kk * 4 + ak], Bj[off], acc);
          }
        }
        double* Ao = At + (fy_ntiles(ti) + tj) * kFyTileElems;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = Mfma<double>::row(lane, r);
          double a = acc[r];
          if (ti == tj && row == ar) a += ti * kFyTile + row < D ? vinv[ti * kFyTile + row] : 1.0;
          Ao[fy_tile_off(row, ar)] = a;
        }
      }
    }
    {
      const int col = tid >> 1, half = tid & 1;
      double c = 0.0;
      if (col < D) {
        const int tj = col >> 4, cc = col & 15;
        for (int i = col + half; i < D; i += 2)
          c = fma(Lt[(fy_ntiles(i >> 4) + tj) * kFyTileElems + fy_tile_off(i & 15, cc)], wy[i], c);
      }
      c += __shfl_xor(c, 1, 64);
      if (col < D && half == 0) bv[col] = fma(vinv[col], mug[col], c);
    }
    __syncthreads();

    // ---- 3. tiled Cholesky of A in place, left-looking; the diagonal tiles end as the inverses of their factors
#pragma unroll 1
    for (int k = 0; k < NT; ++k) {
      double* Dk = At + (fy_ntiles(k) + k) * kFyTileElems;
      f64x4 tt[JMAX];
      if (wave == 0) {
        // the updated diagonal tile, full and symmetric, through LDS into rows
        f64x4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = Dk[fy_tile_off(Mfma<double>::row(lane, r), ar)];
        for (int m = 0; m < k; ++m) {
          const double* Pk = At + (fy_ntiles(k) + m) * kFyTileElems;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const double p = Pk[fy_tile_off(ar, kk * 4 + ak)];
            acc = Mfma<double>::mma(-p, p, acc);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) Dk[fy_tile_off(Mfma<double>::row(lane, r), ar)] = acc[r];
        double a[kFyTile], rinv[kFyTile], x[kFyTile];
#pragma unroll
        for (int c = 0; c < kFyTile; ++c) {                     // from the lower triangle: w sits in one operand of
          const double lo = Dk[fy_tile_off(ar, c)], up = Dk[fy_tile_off(c, ar)];   // step 2, so a_ij and a_ji can
          a[c] = c <= ar ? lo : up;                             // differ in the last bit
        }
        // right-looking on the full symmetric tile: lane i holds row i, row j of the Schur complement is lane j's
#pragma unroll
        for (int j = 0; j < kFyTile; ++j) {
          rinv[j] = 1.0 / sqrt(yc_readlane(a[j], j));
          const double lij = a[j] * rinv[j];
#pragma unroll
          for (int c = j + 1; c < kFyTile; ++c) a[c] = fma(-lij, yc_readlane(a[c], j) * rinv[j], a[c]);
          a[j] = lij;
        }
        // the inverse of the factor by forward substitution, lane = column (l_ik is register k of lane i)
#pragma unroll
        for (int i = 0; i < kFyTile; ++i) {
          double v = i == ar ? 1.0 : 0.0;
#pragma unroll
          for (int c = 0; c < i; ++c) v = fma(-yc_readlane(a[c], i), x[c], v);
          x[i] = v * rinv[i];
        }
        if (lane < kFyTile) {
#pragma unroll
          for (int i = 0; i < kFyTile; ++i) Dk[fy_tile_off(i, ar)] = x[i];
        }
      } else {
        // T^T of the tiles below: register r holds T^T[ak + 4 r][ar] = T[ar][ak + 4 r]
#pragma unroll
        for (int jj = 0; jj < JMAX; ++jj) {
          const int i = k + wave + 3 * jj;
          if (i < NT) {
            const double* Aik = At + (fy_ntiles(i) + k) * kFyTileElems;
            f64x4 acc;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = Aik[fy_tile_off(ar, Mfma<double>::row(lane, r))];
            for (int m = 0; m < k; ++m) {
              const double* Pk = At + (fy_ntiles(k) + m) * kFyTileElems;
              const double* Pi = At + (fy_ntiles(i) + m) * kFyTileElems;
#pragma unroll
              for (int kk = 0; kk < 4; ++kk) {
                const int off = fy_tile_off(ar, kk * 4 + ak);
                acc = Mfma<double>::mma(-Pk[off], Pi[off], acc);
              }
            }
            tt[jj] = acc;
          }
        }
      }
      __syncthreads();
      if (wave != 0) {
#pragma unroll
        for (int jj = 0; jj < JMAX; ++jj) {
          const int i = k + wave + 3 * jj;
          if (i < NT) {
            f64x4 p = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int r = 0; r < 4; ++r)
              p = Mfma<double>::mma(Dk[fy_tile_off(ar, Mfma<double>::row(lane, r))], tt[jj][r], p);
            double* Aik = At + (fy_ntiles(i) + k) * kFyTileElems;
#pragma unroll
            for (int r = 0; r < 4; ++r) Aik[fy_tile_off(ar, Mfma<double>::row(lane, r))] = p[r];
          }
        }
      }
      __syncthreads();
    }

    // ---- 4. forward solves, one block of right-hand sides per wave at a time, and the entries' mu and v
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const int blk = wave + kb * kFyWaves;
      if (blk < nB) {
        const int ci = blk * kYcRhs + ar;
        const bool isb = ar == kYcRhs, live = !isb && ci < nH;
        const int h = live ? hl[ci] : -1;
        const double* Lh = Lt + fy_ntiles(max(h, 0) >> 4) * kFyTileElems;
        f64x4 X[NT];
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
          f64x4 t;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int jr = Mfma<double>::row(lane, r), j = ti * kFyTile + jr;
            double v = isb ? bv[j] : 0.0;
            if (j <= h) v = Lh[ti * kFyTileElems + fy_tile_off(h & 15, jr)];
            t[r] = v;
          }
#pragma unroll
          for (int kt = 0; kt < ti; ++kt) {
            const double* Rt = At + (fy_ntiles(ti) + kt) * kFyTileElems;
#pragma unroll
            for (int r = 0; r < 4; ++r)
              t = Mfma<double>::mma(-Rt[fy_tile_off(ar, Mfma<double>::row(lane, r))], X[kt][r], t);
          }
          const double* Wt = At + (fy_ntiles(ti) + ti) * kFyTileElems;
          f64x4 x = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int r = 0; r < 4; ++r) x = Mfma<double>::mma(Wt[fy_tile_off(ar, Mfma<double>::row(lane, r))], t[r], x);
          X[ti] = x;
        }
        double pm = 0.0, pv = 0.0;
#pragma unroll
        for (int ti = 0; ti < NT; ++ti) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double c = __shfl(X[ti][r], (lane & 48) | kYcRhs, 64);
            pm = fma(X[ti][r], c, pm);
            pv = fma(X[ti][r], X[ti][r], pv);
          }
        }
        pm += __shfl_xor(pm, 16, 64);
        pv += __shfl_xor(pv, 16, 64);
        pm += __shfl_xor(pm, 32, 64);
        pv += __shfl_xor(pv, 32, 64);
        if (live && lane < kYcRhs) {
          const double mu = bad ? nan : pm;
          const double v = bad ? nan : pv + s2;
          const double f2 = bad ? nan : fma(mu, mu, pv);
          sm[kb] += mu;
          sy[kb] += fma(mu, mu, v);
          sf[kb] += f2;
          if (__builtin_isfinite(yt[kb])) {
            const double d = yt[kb] - mu;
            const double ll = -0.5 * (log(6.283185307179586477 * v) + d * d / v);
            y_lse_combine(lm[kb], lr[kb], ll, 1.0, &lm[kb], &lr[kb]);
          }
          if (o.Mu) {
            const int64_t at = (s_off + s) * (int64_t)E + e0 + ci;
            o.Mu[at] = mu;
            o.Var[at] = v;
          }
        }
      }
    }
    __syncthreads();                                            // L and A are free for the next sample
  }

  // ---- the slice's sums leave the workgroup
  const bool direct = gridDim.y == 1;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int ci = (wave + kb * kFyWaves) * kYcRhs + ar;
    if (lane < kYcRhs && ci < nH) {
      const int64_t e = (int64_t)e0 + ci;
      if (direct) {
        o.mu_sum[e] += sm[kb];
        o.y2_sum[e] += sy[kb];
        o.f2_sum[e] += sf[kb];
        if (__builtin_isfinite(yt[kb])) {
          double m, r;
          y_lse_combine(o.lse_max[e], o.lse_sum[e], lm[kb], lr[kb], &m, &r);
          o.lse_max[e] = m;
          o.lse_sum[e] = r;
        }
      } else {
        double* w = ws + ((int64_t)slice * E + e) * kYcWs;
        w[0] = sm[kb];
        w[1] = sy[kb];
        w[2] = sf[kb];
        w[3] = lm[kb];
        w[4] = lr[kb];
      }
    }
  }
}

// The outputs += the slices' partial sums, in slice order; one thread per entry.
__global__ __launch_bounds__(256) void ycond_reduce_kernel(const double* __restrict__ ws, int nsl, int E, YcOut o) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  double a = 0.0, b = 0.0, c = 0.0, m = -INFINITY, r = 0.0;
  for (int sl = 0; sl < nsl; ++sl) {
    const double* w = ws + ((int64_t)sl * E + e) * kYcWs;
    a += w[0];
    b += w[1];
    c += w[2];
    y_lse_combine(m, r, w[3], w[4], &m, &r);
  }
  o.mu_sum[e] += a;
  o.y2_sum[e] += b;
  o.f2_sum[e] += c;
  if (o.y_true && __builtin_isfinite(o.y_true[e])) {
    y_lse_combine(o.lse_max[e], o.lse_sum[e], m, r, &m, &r);
    o.lse_max[e] = m;
    o.lse_sum[e] = r;
  }
}

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int64_t nmgp_ycond_workspace_size(int D, int N, int S) {
  if (D < 1 || D > kFyMaxD || N <= 0 || S <= 0) return 0;
  int nsl, per;
  fy_slicing(N, S, &nsl, &per);
  return nsl == 1 ? 0 : (int64_t)nsl * N * D * kYcWs * (int64_t)sizeof(double);
}

int nmgp_ycond_accum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                         int64_t z_stride, const double* mu_g, const double* var_g, const double* Y_obs, double s2,
                         int D, int N, int S, const int32_t* e_off, int E, double* mu_sum, double* y2_sum,
                         double* f2_sum, const double* y_true, double* lse_max, double* lse_sum, double* Mu,
                         double* Var, int64_t ld, int64_t s_off, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (D < 1 || D > kFyMaxD || N < 0 || S < 0 || E < 0 || s_off < 0) return NMGP_ERR_YCOND_ARG;
  if ((int64_t)E > (int64_t)N * D) return NMGP_ERR_YCOND_ARG;
  if ((Mu == nullptr) != (Var == nullptr)) return NMGP_ERR_YCOND_ARG;
  if (y_true && (!lse_max || !lse_sum)) return NMGP_ERR_YCOND_ARG;
  if (N == 0 || S == 0 || E == 0) return NMGP_OK;
  if (!pair_mu || !pair_sd || !z_p || !mu_g || !var_g || !Y_obs || !e_off) return NMGP_ERR_YCOND_ARG;
  if (!mu_sum || !y2_sum || !f2_sum) return NMGP_ERR_YCOND_ARG;
  if (!(s2 > 0.0) || ld_pair < N || z_stride < 0 || N > 0x7fffffff - kFyXcds) return NMGP_ERR_YCOND_ARG;
  if (Mu && ld < s_off + S) return NMGP_ERR_YCOND_ARG;
  int nsl, per;
  fy_slicing(N, S, &nsl, &per);
  if (!ws_covers(nmgp_ycond_workspace_size(D, N, S), ws, ws_bytes)) return NMGP_ERR_YCOND_ARG;
  const YcOut o = {mu_sum, y2_sum, f2_sum, lse_max, lse_sum, Mu, Var, y_true};
  const int rc = fy_dispatch_nt((D + kFyTile - 1) / kFyTile, NMGP_ERR_YCOND_ARG, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    const size_t smem = (size_t)(2 * fy_ntiles(NT) * kFyTileElems + 5 * NT * kFyTile) * sizeof(double) +
                        (size_t)(NT * kFyTile + 4) * sizeof(int);
    return fy_launch<ycond_accum_kernel<NT>>(smem, N, nsl, stream, pair_mu, pair_sd, ld_pair, z_p, z_stride, mu_g,
                                             var_g, Y_obs, s2, D, N, S, per, e_off, E, o, s_off, (double*)ws);
  });
  if (rc != NMGP_OK) return rc;
  if (nsl > 1) {
    hipLaunchKernelGGL(ycond_reduce_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, stream,
                       (const double*)ws, nsl, E, o);
    NMGP_CHECK_LAUNCH();
  }
  return NMGP_OK;
}

}  // extern "C"
