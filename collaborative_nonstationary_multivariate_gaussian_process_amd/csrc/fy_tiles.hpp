// The LDS tile layout, the sample slicing and the stages that the fused posterior summaries share (fy.hip,
// cgroup.hip, pcorr.hip, ycond.hip): a lower-triangular matrix of up to 128 rows as its 16 x 16 tiles, one workgroup
// of 4 waves per (input, slice of samples).  A stage defined here is force-inlined at its call sites.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace nmgp {

constexpr int kFyThreads = 256;
constexpr int kFyWaves = kFyThreads / kWave;
constexpr int kFyTile = 16;
constexpr int kFyTileElems = kFyTile * kFyTile;
constexpr int kFyMaxD = 128;
constexpr int kFyXcds = 8;

__host__ __device__ inline int fy_ntiles(int nt) { return nt * (nt + 1) / 2; }
__device__ inline int fy_tile_off(int r, int c) { return r * kFyTile + (c ^ ((r >> 1) << 1)); }
// Row of element q of a packed lower triangle: the largest i with i (i + 1) / 2 <= q (q <= 8255; the float
// estimate is off by at most one).
__device__ inline int fy_tri_row(int q) {
  int i = (int)((sqrtf((float)(8 * q + 1)) - 1.0f) * 0.5f);
  i += (i + 1) * (i + 2) / 2 <= q;
  i -= i * (i + 1) / 2 > q;
  return i;
}

// The input of this workgroup.  Consecutive inputs share an XCD (and its L2): the (Q, N) operands are read at one n
// per workgroup, so the 8 inputs of a 64-byte line are best fetched by workgroups behind one L2.
__device__ __forceinline__ int fy_block_input(int n_blocks) {
  const int bid = blockIdx.x;
  return (bid % kFyXcds) * (n_blocks / kFyXcds) + bid / kFyXcds;
}

// Pair samples of one sample and input -> the tiles of L, exp on the diagonal; zp points at the sample's pair noise
// of input n.  FLAG_BAD: a diagonal entry that is 0, inf or NaN after the exp sets *bad_slot.
template <bool FLAG_BAD>
__device__ __forceinline__ void fy_load_L(double* Lt, const double* __restrict__ pair_mu,
                                          const double* __restrict__ pair_sd, int64_t ld_pair,
                                          const double* __restrict__ zp, int n, int N, int Q, int tid, int* bad_slot) {
  // not unrolled: with 4 or 8 pairs' loads in flight per lane the launch took 20-25 % longer at D = 50 and 128
  // (each lane's load is a 64-byte line of its own, shared only with the neighbouring inputs' workgroups)
#pragma unroll 1
  for (int q = tid; q < Q; q += kFyThreads) {
    const int i = fy_tri_row(q);
    const int j = q - i * (i + 1) / 2;
    double l = pair_mu[(int64_t)q * ld_pair + n] + pair_sd[(int64_t)q * ld_pair + n] * zp[(int64_t)q * N];
    if (i == j) {
      l = exp(l);
      if constexpr (FLAG_BAD) {
        if (!(__builtin_isfinite(l) && l != 0.0)) *bad_slot = 1;
      }
    }
    Lt[(fy_ntiles(i >> 4) + (j >> 4)) * kFyTileElems + fy_tile_off(i & 15, j & 15)] = l;
  }
}

// cov_ii = |row i of L|^2 by two threads per row, columns of one parity each; both threads return the sum.  WITH_G:
// the same loop also forms the row's product with the vector Gs, returned through *f.
template <bool WITH_G>
__device__ __forceinline__ double fy_row_sums(const double* Lt, const double* Gs, int D, int tid, double* f_out) {
  const int frow = tid >> 1, fhalf = tid & 1;
  double f = 0.0, c = 0.0;
  if (frow < D) {
    const int ti = frow >> 4, r = frow & 15;
    const double* rowt = Lt + fy_ntiles(ti) * kFyTileElems;
    for (int j = fhalf; j <= frow; j += 2) {
      const double v = rowt[(j >> 4) * kFyTileElems + fy_tile_off(r, j & 15)];
      if constexpr (WITH_G) f = fma(v, Gs[j], f);
      c = fma(v, v, c);
    }
  }
  if constexpr (WITH_G) *f_out = f + __shfl_xor(f, 1, 64);
  return c + __shfl_xor(c, 1, 64);
}

// ---------------------------------------------------------------------------------------------------- host side
// Sample slices: none while the inputs alone fill the chip's 256 CUs, else as many as keep N * slices <= 512.
static void fy_slicing(int N, int S, int* nsl, int* per) {
  int want = N >= 256 ? 1 : 512 / N;
  if (want > S) want = S;
  if (want < 1) want = 1;
  *per = (S + want - 1) / want;
  *nsl = (S + *per - 1) / *per;
}

// Bytes of the workspace that fy.hip and pcorr.hip hand their slices' sums through: a sum and a sum of squares (D, D) per slice and input.
static int64_t fy_tri_workspace_bytes(int D, int N, int S) {
  if (D < 1 || D > kFyMaxD || N <= 0 || S <= 0) return 0;
  int nsl, per;
  fy_slicing(N, S, &nsl, &per);
  return nsl == 1 ? 0 : (int64_t)nsl * N * 2 * D * D * (int64_t)sizeof(double);
}

// out_sum / out_sq (N, D, D) += the nsl slices' partial sums in that workspace, in slice order (defined in fy.hip).
int fy_tri_reduce(const double* ws, int nsl, int D, int N, double* out_sum, double* out_sq, hipStream_t stream);

// Launch of one kernel instantiation of the family over (inputs rounded up to whole XCD rounds, nsl slices) with
// smem bytes of dynamic LDS, asked for once per instantiation (more than the default 64 KiB has to be).  The grid's x
// extent is the kernel's last parameter (fy_block_input).
template <auto Kernel, class... Args>
static int fy_launch(size_t smem, int N, int nsl, hipStream_t s, Args... args) {
  allow_dynamic_lds<Kernel>(smem);
  const int n_blocks = (N + kFyXcds - 1) / kFyXcds * kFyXcds;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)n_blocks, (unsigned)nsl), dim3(kFyThreads), smem, s, args..., n_blocks);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

// f(std::integral_constant<int, NT>) for the NT = nt tile rows of D <= 128, else err.
template <class F> static int fy_dispatch_nt(int nt, int err, F f) {
  switch (nt) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return err;
  }
}

}  // namespace nmgp
