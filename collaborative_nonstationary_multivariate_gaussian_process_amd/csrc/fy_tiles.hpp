// The LDS tile layout and the sample slicing that the fused posterior summaries share (fy.hip, pcorr.hip): a lower-
// triangular matrix of up to 128 rows as its 16 x 16 tiles, one workgroup of 4 waves per (input, slice of samples).
#pragma once
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

// Sample slices: none while the inputs alone fill the chip's 256 CUs, else as many as keep N * slices <= 512.
static void fy_slicing(int N, int S, int* nsl, int* per) {
  int want = N >= 256 ? 1 : 512 / N;
  if (want > S) want = S;
  if (want < 1) want = 1;
  *per = (S + want - 1) / want;
  *nsl = (S + *per - 1) / *per;
}

}  // namespace nmgp
