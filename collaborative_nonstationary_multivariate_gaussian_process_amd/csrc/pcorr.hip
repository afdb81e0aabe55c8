// Partial correlations of the outputs, fused like the correlations of fy.hip: per sample s and input n the pair
// samples -> L, W = L^-1, Omega = W^T W = (L L^T)^-1, pcorr = -D^-1/2 Omega D^-1/2 (diagonal 1), accumulated over the
// samples on the device and, for a list of pairs, collected per sample into the layout nmgp_quantile_rows_f64 sorts.
// The (S, N, D, D) tensor is never stored.  The reference has no partial-correlation code; the quantity is a pure
// function of the covariance of NMGP.sample_FY (reference code/nmgp_dsvi.py:567-569).
//
// One workgroup (4 waves) per (input n, slice of samples), L and W side by side in LDS in the tile layout of
// fy_tiles.hpp (2 x 72 KiB at D = 128, 2 x 20 KiB at D = 50, plus 1 KiB: under the CU's 160 KiB at every D <= 128).
// The rows of L past D carry a unit diagonal, so W is [[W_D, 0], [0, I]] and Omega's leading block is untouched.
//
// The inverse: the 16 x 16 diagonal tiles are inverted by forward substitution, one tile per 16 lanes (lane = column
// of the inverse, 120 chained fma), all NT <= 8 of them at once on the 16 lane groups of the workgroup.  The tiles
// below go tile row by tile row, W(ti, tj) = -W(ti, ti) sum_{tj <= k < ti} L(ti, k) W(k, tj), on
// v_mfma_f64_16x16x4_f64; the sum's accumulator registers are fed straight back as the B operand of the product
// with W(ti, ti) (register r of the C layout holds k = (lane >> 4) + 4 r; the A operand is read in that k order),
// so no LDS round trip lies between the two.  The ti tiles of a row are dealt to the 4 waves; a barrier ends each
// row.  That recurrence is the serial part: row ti costs its longest wave ceil(ti / 4) chains of up to 4 ti + 4
// dependent MFMAs, 176 MFMAs on the critical path at NT = 8 against 448 / 4 = 112 if the rows could overlap, and
// NT barriers.  Splitting a tile's k sum over waves would shorten the chains but needs an LDS reduction and a
// barrier per row more; the row-wise split is kept because Omega (480 MFMAs at NT = 8, no dependences between
// tiles) is the larger half and runs perfectly dealt.  Omega tile (ti, tj <= ti) = sum_{kt >= ti} W(kt, ti)^T
// W(kt, tj): both operands are read as 4 whole rows of a tile (512 contiguous bytes, no bank conflict), the tiles
// are dealt round-robin and each wave keeps its tiles' running sums in registers across the slice's samples, as
// fy.hip does.  The sums leave the workgroup once: onto pc_sum / pc_sq when the samples are not sliced, else into
// the per-slice workspace that a second kernel adds up in slice order (no floating-point atomics).
//
// Pair collection: the normalised lower triangle is written over L (no longer needed), and thread t stores the
// pairs t, t + 256, ... of the list to C[p, n, s_off + s].  The stores run along the pair axis, 8 bytes each, one
// sample at a time: samples are NOT staged to make runs along s (that would take a third matrix in LDS at D = 128);
// tools/pcorr_probe.py records what this plain form costs.
//
// Group collection (nmgp_pcorr_accum_groups_f64): the same triangle over L, reduced per group of a table of (i, j)
// groups by the device function that cgroup.hip uses (fy_groups.hpp) into Cg[k, n, sg_off + s].  Sums, pair list and
// groups are three independent switches of the one launch; L^-1 and Omega are computed once for whichever are asked.
#include "fy_groups.hpp"

namespace nmgp {

template <int NT>
__global__ __launch_bounds__(kFyThreads) void pcorr_accum_kernel(
    const double* __restrict__ pair_mu, const double* __restrict__ pair_sd, int64_t ld_pair,
    const double* __restrict__ z_p, int64_t z_stride, int D, int N, int S, int per, double* __restrict__ pc_sum,
    double* __restrict__ pc_sq, const int32_t* __restrict__ pi, const int32_t* __restrict__ pj, int P,
    double* __restrict__ C, int64_t ld_c, int64_t s_off, const int32_t* __restrict__ goff,
    const uint32_t* __restrict__ gent, int K, int E, double* __restrict__ Cg, int64_t ld_cg, int64_t sg_off,
    double* __restrict__ ws, int n_blocks) {
  constexpr int T = NT * (NT + 1) / 2;                  // lower-triangular tiles
  constexpr int KMAX = (T + kFyWaves - 1) / kFyWaves;   // Omega tiles of one wave
  extern __shared__ __attribute__((aligned(16))) double pc_smem[];
  double* Lt = pc_smem;                                 // T tiles: L, later the normalised result
  double* Wt = Lt + T * kFyTileElems;                   // T tiles: L^-1
  double* Is = Wt + T * kFyTileElems;                   // NT * 16: sqrt(1 / Omega_ii), 0 past D
  __shared__ int bad_flag[2];                           // a diagonal of L that is 0, inf or NaN, by sample parity
  __shared__ double part[2 * kFyWaves];                 // wave sums of a group that the whole workgroup adds

  const int n = fy_block_input(n_blocks);
  if (n >= N) return;
  const int slice = blockIdx.y;
  const int s0 = slice * per, s1 = min(S, s0 + per);
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform32(tid >> 6);
  const int Q = D * (D + 1) / 2;
  const bool accumulate = pc_sum != nullptr;
  const bool keep = P > 0 || K > 0;                     // the normalised triangle is wanted in LDS
  int par = 0;

  for (int e = tid; e < 2 * T * kFyTileElems + NT * kFyTile; e += kFyThreads) pc_smem[e] = 0.0;
  if (tid < 2) bad_flag[tid] = 0;
  __syncthreads();
  // unit diagonal in the rows past D (never overwritten: the pair samples and the results stay inside D)
  if (tid >= D && tid < NT * kFyTile)
    Lt[(fy_ntiles(tid >> 4) + (tid >> 4)) * kFyTileElems + fy_tile_off(tid & 15, tid & 15)] = 1.0;

  f64x4 sum[KMAX], sq[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) sum[k] = sq[k] = f64x4{0.0, 0.0, 0.0, 0.0};

  const int ar = lane & 15, ak = lane >> 4;             // MFMA operand row / k of this lane
  const double nan = __builtin_nan("");
  __syncthreads();

  for (int s = s0; s < s1; ++s) {
    // ---- pair samples -> L tiles: fy_load_L<true> of fy_tiles.hpp (which says why the loop is not unrolled),
    // kept as a copy here, like the column sums and the exit of the sums below: with the shared functions the
    // sums-only launch measured 2-3 % slower (tools/pcorr_probe.py), with every stage local as before
    const double* zp = z_p + (int64_t)s * z_stride + n;
#pragma unroll 1
    for (int q = tid; q < Q; q += kFyThreads) {
      const int i = fy_tri_row(q);
      const int j = q - i * (i + 1) / 2;
      double l = pair_mu[(int64_t)q * ld_pair + n] + pair_sd[(int64_t)q * ld_pair + n] * zp[(int64_t)q * N];
      if (i == j) {
        l = exp(l);
        if (!(__builtin_isfinite(l) && l != 0.0)) bad_flag[s & 1] = 1;
      }
      Lt[(fy_ntiles(i >> 4) + (j >> 4)) * kFyTileElems + fy_tile_off(i & 15, j & 15)] = l;
    }
    if (tid == 0) bad_flag[(s + 1) & 1] = 0;            // last read two barriers before the end of sample s - 1
    __syncthreads();
    const bool bad = bad_flag[s & 1] != 0;

    // ---- diagonal tiles of W by forward substitution: tile t on wave t & 3, lanes 16 (t >> 2) ... + 15, lane =
    // column c of the inverse.  Lane groups without a tile redo the last one and store nothing.
    {
      const int t = ak * kFyWaves + wave, tc = min(t, NT - 1);
      const double* Ld = Lt + (fy_ntiles(tc) + tc) * kFyTileElems;
      const double dinv = 1.0 / Ld[fy_tile_off(ar, ar)];
      double x[kFyTile];
#pragma unroll
      for (int i = 0; i < kFyTile; ++i) {
        double a = i == ar ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) a = fma(-Ld[fy_tile_off(i, k)], x[k], a);
        x[i] = a * __shfl(dinv, (lane & 48) + i, 64);
      }
      if (t < NT) {
        double* Wd = Wt + (fy_ntiles(t) + t) * kFyTileElems;
#pragma unroll
        for (int i = 0; i < kFyTile; ++i) Wd[fy_tile_off(i, ar)] = x[i];
      }
    }
    __syncthreads();

    // ---- the tiles below the diagonal, tile row by tile row
    for (int ti = 1; ti < NT; ++ti) {
      const double* Dt = Wt + (fy_ntiles(ti) + ti) * kFyTileElems;
      for (int tj = wave; tj < ti; tj += kFyWaves) {
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k = tj; k < ti; ++k) {
          const double* At = Lt + (fy_ntiles(ti) + k) * kFyTileElems;
          const double* Bt = Wt + (fy_ntiles(k) + tj) * kFyTileElems;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
            acc = Mfma<double>::mma(At[fy_tile_off(ar, kk * 4 + ak)], Bt[fy_tile_off(kk * 4 + ak, ar)], acc);
        }
        f64x4 w = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) w = Mfma<double>::mma(Dt[fy_tile_off(ar, Mfma<double>::row(lane, r))], acc[r], w);
        double* Wo = Wt + (fy_ntiles(ti) + tj) * kFyTileElems;
#pragma unroll
        for (int r = 0; r < 4; ++r) Wo[fy_tile_off(Mfma<double>::row(lane, r), ar)] = -w[r];
      }
      __syncthreads();
    }

    // ---- the diagonal of Omega: two threads per column of W, rows of one parity each
    {
      const int col = tid >> 1, half = tid & 1;
      double c = 0.0;
      if (col < D) {
        const int tj = col >> 4, cc = col & 15;
        for (int k = tj * kFyTile + half; k < NT * kFyTile; k += 2) {
          const double v = Wt[(fy_ntiles(k >> 4) + tj) * kFyTileElems + fy_tile_off(k & 15, cc)];
          c = fma(v, v, c);
        }
      }
      c += __shfl_xor(c, 1, 64);
      if (col < D && half == 0) Is[col] = sqrt(1.0 / c);
    }
    __syncthreads();

    // ---- Omega tiles on the matrix cores, normalised, accumulated and (for the pair list) left in LDS over L
    int tw = wave;
    asm volatile("" : "+s"(tw));                        // tile coordinates recomputed per sample, as fy.hip
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int t = tw + k * kFyWaves;
      if (t < T) {
        const int ti = uniform32(fy_tri_row(t));
        const int tj = t - fy_ntiles(ti);
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int kt = ti; kt < NT; ++kt) {
          const double* At = Wt + (fy_ntiles(kt) + ti) * kFyTileElems;
          const double* Bt = Wt + (fy_ntiles(kt) + tj) * kFyTileElems;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const int o = fy_tile_off(kk * 4 + ak, ar);
            acc = Mfma<double>::mma(At[o], Bt[o], acc);
          }
        }
        const double isj = Is[tj * kFyTile + ar];
        double* Ro = Lt + (fy_ntiles(ti) + tj) * kFyTileElems;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = Mfma<double>::row(lane, r);
          const double isi = Is[ti * kFyTile + row];
          // the diagonal is 1, not 1 +- rounding (E[c^2] - mean^2 must be 0 there); a sample with a non-finite
          // or zero diagonal of L is NaN everywhere
          double c = -acc[r] * isi * isj;
          if (ti == tj && row == ar) c = 1.0;
          if (bad) c = nan;
          if (accumulate) {
            sum[k][r] += c;
            sq[k][r] = fma(c, c, sq[k][r]);
          }
          // inside D and on or below the diagonal only: the zeros above it and the unit diagonal past D stay
          if (keep && ti * kFyTile + row < D && (ti > tj || ar <= row)) Ro[fy_tile_off(row, ar)] = c;
        }
      }
    }
    __syncthreads();

    // ---- the listed pairs and the groups of this sample
    if (keep) {
      for (int p = tid; p < P; p += kFyThreads) {
        const int i = pi[p], j = pj[p];
        const int a = max(i, j), b = min(i, j);
        double v = nan;
        if (b >= 0 && a < D) v = Lt[(fy_ntiles(a >> 4) + (b >> 4)) * kFyTileElems + fy_tile_off(a & 15, b & 15)];
        C[((int64_t)p * N + n) * ld_c + s_off + s] = v;
      }
      if (K > 0)
        fy_group_reduce(Lt, D, goff, gent, K, E, part, par, Cg + (int64_t)n * ld_cg + sg_off + s,
                        (int64_t)N * ld_cg, tid);
      __syncthreads();
    }
  }

  if (!accumulate) return;
  // ---- the slice's sums leave the workgroup: lower triangle held, both triangles written
  const int64_t dd = (int64_t)D * D;
  const bool direct = gridDim.y == 1;
  double* o_sum = direct ? pc_sum + (int64_t)n * dd : ws + (((int64_t)slice * N + n) * 2) * dd;
  double* o_sq = direct ? pc_sq + (int64_t)n * dd : o_sum + dd;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int t = wave + k * kFyWaves;
    if (t < T) {
      const int ti = uniform32(fy_tri_row(t));
      const int tj = t - fy_ntiles(ti);
      const int j = tj * kFyTile + ar;
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

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int64_t nmgp_pcorr_workspace_size(int D, int N, int S) { return fy_tri_workspace_bytes(D, N, S); }

int nmgp_pcorr_accum_groups_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                                int64_t z_stride, int D, int N, int S, double* pc_sum, double* pc_sq,
                                const int32_t* pi, const int32_t* pj, int P, double* C, int64_t ld_c, int64_t s_off,
                                const int32_t* goff, const int32_t* gent, int K, int E, double* Cg, int64_t ld_cg,
                                int64_t sg_off, void* ws, int64_t ws_bytes, hipStream_t stream) {
  if (D < 1 || D > kFyMaxD || N < 0 || S < 0 || P < 0 || s_off < 0 || K < 0 || sg_off < 0)
    return NMGP_ERR_PCORR_ARG;
  if ((pc_sum == nullptr) != (pc_sq == nullptr)) return NMGP_ERR_PCORR_ARG;
  if (!pc_sum && P == 0 && K == 0) return NMGP_ERR_PCORR_ARG;
  if (N == 0 || S == 0) return NMGP_OK;
  if (!pair_mu || !pair_sd || !z_p) return NMGP_ERR_PCORR_ARG;
  if (ld_pair < N || z_stride < 0 || N > 0x7fffffff - kFyXcds) return NMGP_ERR_PCORR_ARG;
  if (P > 0 && (!pi || !pj || !C || ld_c < s_off + S)) return NMGP_ERR_PCORR_ARG;
  if (K > 0 && (!goff || !gent || !Cg || E < K || ld_cg < sg_off + S)) return NMGP_ERR_PCORR_ARG;
  int nsl, per;
  fy_slicing(N, S, &nsl, &per);
  if (pc_sum && !ws_covers(fy_tri_workspace_bytes(D, N, S), ws, ws_bytes)) return NMGP_ERR_PCORR_ARG;
  const int rc = fy_dispatch_nt((D + kFyTile - 1) / kFyTile, NMGP_ERR_PCORR_ARG, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    const size_t smem = (size_t)(2 * fy_ntiles(NT) * kFyTileElems + NT * kFyTile) * sizeof(double);
    return fy_launch<pcorr_accum_kernel<NT>>(smem, N, nsl, stream, pair_mu, pair_sd, ld_pair, z_p, z_stride, D, N, S,
                                             per, pc_sum, pc_sq, pi, pj, P, C, ld_c, s_off, goff,
                                             (const uint32_t*)gent, K, E, Cg, ld_cg, sg_off, (double*)ws);
  });
  if (rc != NMGP_OK || !pc_sum || nsl == 1) return rc;
  return fy_tri_reduce((const double*)ws, nsl, D, N, pc_sum, pc_sq, stream);
}

// the form without groups: the same launch, K = 0
int nmgp_pcorr_accum_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                         int64_t z_stride, int D, int N, int S, double* pc_sum, double* pc_sq, const int32_t* pi,
                         const int32_t* pj, int P, double* C, int64_t ld_c, int64_t s_off, void* ws, int64_t ws_bytes,
                         hipStream_t stream) {
  return nmgp_pcorr_accum_groups_f64(pair_mu, pair_sd, ld_pair, z_p, z_stride, D, N, S, pc_sum, pc_sq, pi, pj, P, C,
                                     ld_c, s_off, nullptr, nullptr, 0, 0, nullptr, 0, 0, ws, ws_bytes, stream);
}

}  // extern "C"
