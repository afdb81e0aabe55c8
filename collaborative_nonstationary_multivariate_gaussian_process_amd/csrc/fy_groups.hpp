// The group reduction that cgroup.hip and pcorr.hip share: a normalised lower triangle in the tile layout of
// fy_tiles.hpp in LDS + a CSR table of groups of (i, j) entries -> the plain mean of every group, stored to
// C[k, n, col].  The caller has put a barrier between the last write of the triangle and this call.
//
// Table: goff (K + 1 int32 offsets into the entries), gent (E packed entries (max(i, j) << 16) | min(i, j)); both in
// device memory, so a launch can be captured.  Nothing in the table can make the reduction leave its buffers: the
// offsets are clamped to 0..E and made monotone (an empty group is 0 / 0 = NaN), and an entry is unpacked, ordered
// again and compared with D before it indexes LDS (an entry outside 0..D-1 is NaN, and so is its group).
//
// Summation order, a function of the group alone (not of the other groups of the call, of the slice or of the wave
// the group lands on): a group of g <= 256 entries belongs to one wave, lane l adds the entries l, l + 64, ... in
// that order and the 64 lane sums are combined by the xor butterfly 32, 16, ..., 1 (both partners add the same two
// values, so every lane holds the same bits); groups are dealt round-robin to the 4 waves.  A longer group is summed
// by the whole workgroup: thread t adds the entries t, t + 256, ..., each wave combines its lanes by the same
// butterfly, the 4 wave sums go through LDS and thread 0 adds them in wave order.  One barrier per long group (the
// LDS slots alternate), none for the short ones.
#pragma once
#include "fy_tiles.hpp"

namespace nmgp {

constexpr int kFyGroupWaveMax = 256;         // entries of the longest group that one wave sums

__device__ inline double fy_group_entry(const double* __restrict__ Rt, uint32_t e, int D) {
  const int hi = (int)(e >> 16), lo = (int)(e & 0xffffu);
  const int a = max(hi, lo), b = min(hi, lo);
  if (a >= D) return __builtin_nan("");
  return Rt[(fy_ntiles(a >> 4) + (b >> 4)) * kFyTileElems + fy_tile_off(a & 15, b & 15)];
}

__device__ inline double fy_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Cn = C + n * ld_c + column of this sample; group k is stored at Cn[k * k_stride].  part: 2 x kFyWaves doubles of
// LDS; par: the slot parity, carried by the caller from one call to the next.
__device__ inline void fy_group_reduce(const double* __restrict__ Rt, int D, const int32_t* __restrict__ goff,
                                       const uint32_t* __restrict__ gent, int K, int E, double* part, int& par,
                                       double* __restrict__ Cn, int64_t k_stride, int tid) {
  const int lane = tid & 63, wave = uniform32(tid >> 6);
  for (int k = wave; k < K; k += kFyWaves) {
    const int beg = min(max(uniform32(goff[k]), 0), E), end = min(max(uniform32(goff[k + 1]), beg), E);
    const int g = end - beg;
    if (g > kFyGroupWaveMax) continue;
    double v = 0.0;
    for (int e = beg + lane; e < end; e += kWave) v += fy_group_entry(Rt, gent[e], D);
    v = fy_wave_sum(v);
    if (lane == 0) Cn[(int64_t)k * k_stride] = v / (double)g;
  }
  for (int k = 0; k < K; ++k) {
    const int beg = min(max(uniform32(goff[k]), 0), E), end = min(max(uniform32(goff[k + 1]), beg), E);
    const int g = end - beg;
    if (g <= kFyGroupWaveMax) continue;
    double v = 0.0;
    for (int e = beg + tid; e < end; e += kFyThreads) v += fy_group_entry(Rt, gent[e], D);
    v = fy_wave_sum(v);
    double* slot = part + par * kFyWaves;
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    if (tid == 0) Cn[(int64_t)k * k_stride] = (((slot[0] + slot[1]) + slot[2]) + slot[3]) / (double)g;
    par ^= 1;
  }
}

}  // namespace nmgp
