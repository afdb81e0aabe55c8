// Group means of the output correlations of NMGP.sample_FY (reference NMGP_ECoG_full.py:456-544, "Post analysis":
// the correlations averaged over the left / right / top / bottom neighbours of the electrode grid and over all pairs
// 1, 2 or 3 grid steps apart, plotted over time): per sample s and input n the plain mean of corr[s, n, i, j] over
// every group of a table of (i, j) groups, stored as C[k, n, s_off + s] -- the (K, N, S) samples whose quantiles are
// the credible band of a group mean.  The (S, N, D, D) tensor is never stored, and neither are per-pair samples: the
// reduction over the pairs happens next to the correlation matrix, in LDS.
//
// One workgroup (4 waves) per (input n, slice of samples), the tile layout and the XCD-aware input mapping of
// fy_tiles.hpp.  LDS: L (T tiles), the normalised lower triangle R (T tiles) and Is -- 2 x 72 KiB + 1 KiB = 145
// KiB at D = 128, 2 x 20 KiB + 0.5 KiB at D = 50: the budget of pcorr.hip, under the CU's 160 KiB at every D <= 128.
// Per sample the stages that fy.hip runs: pair samples -> L and diagonal of cov -> Is from the same definitions
// (fy_load_L, fy_row_sums of fy_tiles.hpp); cov tiles on v_mfma_f64_16x16x4_f64 in the tile dealing and k order of
// fy.hip, normalised in its order (acc * isi * isj, diagonal 1 where finite, non-finite values kept), written to R
// instead of being accumulated -- a copy of fy.hip's loop, not a shared function: handing the element to a sink
// cost 1 % at D = 50 with the 28-group table (tools/corr_group_probe.py); then the group reduction of
// fy_groups.hpp.  So a group of one pair is bit for bit the correlation that fy.hip accumulates, which
// tests/test_gpu_corr_groups.py checks.
//
// Nothing is accumulated across samples: no workspace, no atomics, every (k, n, s) is written once by the one
// workgroup that owns (n, s), from that sample alone; the slices (fy_slicing) only fill the chip when N < 256.
// The table is read from global memory once per sample (4 E bytes; at D = 128 there is no LDS left to hold it) and
// stays in the L1 / L2; the stores are 8 bytes each, K per sample and workgroup, not staged into runs along s.
//
// Measured (tools/corr_group_probe.py, N = 800, one chunk, against fy_accum_ on the same inputs): 1.04x - 1.4x at
// D = 50.  At D = 128 the nearly empty 5 x 5 grid table already costs 1.4x (the second tile region leaves one
// workgroup per CU, one wave per SIMD, where fy.hip has two), one group of all 8128 pairs 1.6x, the 28 groups of a
// 7-network partition 2.0x: with a single wave per SIMD the dependent chain of a group (offsets, entries, LDS,
// butterfly, store; a barrier for each of the 21 groups above 256 entries) is exposed, about 1 us per group.
// Splitting the long groups over the waves pays (32 instead of 127 entries per lane for "all"); unrolling the entry
// loops by 4 changed nothing and was not kept.  Overlapping groups inside a wave is the lever left.
#include "fy_groups.hpp"

namespace nmgp {

template <int NT>
__global__ __launch_bounds__(kFyThreads) void corr_group_kernel(
    const double* __restrict__ pair_mu, const double* __restrict__ pair_sd, int64_t ld_pair,
    const double* __restrict__ z_p, int64_t z_stride, int D, int N, int S, int per,
    const int32_t* __restrict__ goff, const uint32_t* __restrict__ gent, int K, int E, double* __restrict__ C,
    int64_t ld_c, int64_t s_off, int n_blocks) {
  constexpr int T = NT * (NT + 1) / 2;                  // lower-triangular tiles
  constexpr int KMAX = (T + kFyWaves - 1) / kFyWaves;   // cov tiles of one wave
  extern __shared__ __attribute__((aligned(16))) double cg_smem[];
  double* Lt = cg_smem;                                 // T tiles: L
  double* Rt = Lt + T * kFyTileElems;                   // T tiles: the normalised lower triangle
  double* Is = Rt + T * kFyTileElems;                   // NT * 16: sqrt(1 / cov_ii), 0 past D
  __shared__ double part[2 * kFyWaves];                 // wave sums of a group that the whole workgroup adds

  const int n = fy_block_input(n_blocks);
  if (n >= N) return;
  const int slice = blockIdx.y;
  const int s0 = slice * per, s1 = min(S, s0 + per);
  const int tid = threadIdx.x, lane = tid & 63, wave = uniform32(tid >> 6);
  const int Q = D * (D + 1) / 2;

  for (int e = tid; e < 2 * T * kFyTileElems + NT * kFyTile; e += kFyThreads) cg_smem[e] = 0.0;

  const int ar = lane & 15, ak = lane >> 4;
  const int64_t k_stride = (int64_t)N * ld_c;
  int par = 0;
  __syncthreads();

  for (int s = s0; s < s1; ++s) {
    // ---- pair samples -> L tiles
    fy_load_L<false>(Lt, pair_mu, pair_sd, ld_pair, z_p + (int64_t)s * z_stride + n, n, N, Q, tid, nullptr);
    __syncthreads();

    // ---- the diagonal of cov
    {
      const double c = fy_row_sums<false>(Lt, nullptr, D, tid, nullptr);
      if ((tid >> 1) < D && (tid & 1) == 0) Is[tid >> 1] = sqrt(1.0 / c);
    }
    __syncthreads();

    // ---- cov tiles on the matrix cores, normalised into R
    int tw = wave;
    asm volatile("" : "+s"(tw));                        // tile coordinates recomputed per sample, as fy.hip
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
        const double isj = Is[tj * kFyTile + ar];
        double* Ro = Rt + t * kFyTileElems;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = Mfma<double>::row(lane, r);
          const double isi = Is[ti * kFyTile + row];
          // as fy.hip: the diagonal is exactly 1 unless the expression is not finite there; rows and columns past
          // D have Is = 0 and are never read (an entry is compared with D first)
          double c = acc[r] * isi * isj;
          if (ti == tj && row == ar && __builtin_isfinite(c)) c = 1.0;
          Ro[fy_tile_off(row, ar)] = c;
        }
      }
    }
    __syncthreads();

    // ---- the groups of this sample.  R is next written two barriers from here, L and Is are not read below.
    fy_group_reduce(Rt, D, goff, gent, K, E, part, par, C + (int64_t)n * ld_c + s_off + s, k_stride, tid);
  }
}

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int nmgp_corr_group_f64(const double* pair_mu, const double* pair_sd, int64_t ld_pair, const double* z_p,
                        int64_t z_stride, int D, int N, int S, const int32_t* goff, const int32_t* gent, int K,
                        int E, double* C, int64_t ld_c, int64_t s_off, hipStream_t stream) {
  if (D < 1 || D > kFyMaxD || N < 0 || S < 0 || K < 0 || s_off < 0) return NMGP_ERR_CGROUP_ARG;
  if (K == 0 || N == 0 || S == 0) return NMGP_OK;
  if (!pair_mu || !pair_sd || !z_p || !goff || !gent || !C) return NMGP_ERR_CGROUP_ARG;
  if (E < K || ld_pair < N || z_stride < 0 || ld_c < s_off + S || N > 0x7fffffff - kFyXcds)
    return NMGP_ERR_CGROUP_ARG;
  int nsl, per;
  fy_slicing(N, S, &nsl, &per);
  return fy_dispatch_nt((D + kFyTile - 1) / kFyTile, NMGP_ERR_CGROUP_ARG, [&](auto nt) {
    constexpr int NT = decltype(nt)::value;
    const size_t smem = (size_t)(2 * fy_ntiles(NT) * kFyTileElems + NT * kFyTile) * sizeof(double);
    return fy_launch<corr_group_kernel<NT>>(smem, N, nsl, stream, pair_mu, pair_sd, ld_pair, z_p, z_stride, D, N, S,
                                            per, goff, (const uint32_t*)gent, K, E, C, ld_c, s_off);
  });
}

}  // extern "C"
