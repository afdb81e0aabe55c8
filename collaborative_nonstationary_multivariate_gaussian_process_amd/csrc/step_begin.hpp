// The start of a graph-replayed training step (dsvi.hip's step_begin_kernel explains it) as a body for workgroup `wg`
// of `nwg`: shared by that kernel and by the step-head kernel (head.hip), whose begin workgroups are a part of its grid.
#pragma once
#include "common.hpp"

namespace nmgp {

// ------------------------------------------------------------------------------------ Philox
__device__ inline void philox_round(uint32_t (&c)[4], uint32_t (&k)[2]) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0;
  const uint32_t h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
  c[0] = h1 ^ c[1] ^ k[0];
  c[1] = l1;
  c[2] = h0 ^ c[3] ^ k[1];
  c[3] = l0;
  k[0] += 0x9E3779B9u;
  k[1] += 0xBB67AE85u;
}

// normals 4t .. 4t+3 of the Philox-4x32-10 stream (key = seed, counter = (t, base)), Box-Muller
template <typename T>
__device__ inline void normal_quad(T* out, int64_t n, uint64_t seed, uint64_t base, int64_t t) {
  uint32_t c[4] = {(uint32_t)t, (uint32_t)((uint64_t)t >> 32), (uint32_t)base, (uint32_t)(base >> 32)};
  uint32_t k[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
#pragma unroll
  for (int r = 0; r < 10; ++r) philox_round(c, k);
  const double inv = 2.3283064365386963e-10;   // 2^-32
  double u[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) u[q] = ((double)c[q] + 0.5) * inv;
  const double two_pi = 6.283185307179586;
  const double r0 = sqrt(-2.0 * log(u[0])), r1 = sqrt(-2.0 * log(u[2]));
  double z[4] = {r0 * cos(two_pi * u[1]), r0 * sin(two_pi * u[1]), r1 * cos(two_pi * u[3]), r1 * sin(two_pi * u[3])};
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (t * 4 + q < n) out[t * 4 + q] = (T)z[q];
}

template <typename T> struct BeginArgs {
  const T* Xb; const T* Yb; const int32_t* Ib; const int32_t* Sb;
  int64_t B, nseg, nbatch;
  int64_t* bctr;
  T* x; T* y; int32_t* ro; int32_t* seg;
  T* noise; int64_t nnoise; uint64_t seed; int64_t* nctr; int32_t* done;
  T* grad; int64_t ngrad;
};

// block `wg` == 0 gathers the minibatch; every block draws its share of the noise and zeroes its share of the gradient;
// the last of the nwg blocks to arrive advances the noise counter and re-arms the arrival word
template <typename T>
__device__ inline void step_begin_body(const BeginArgs<T>& A, int wg, int nwg) {
  const auto Xb = A.Xb;
  const auto Yb = A.Yb;
  const auto Ib = A.Ib;
  const auto Sb = A.Sb;
  const auto B = A.B;
  const auto nseg = A.nseg;
  const auto nbatch = A.nbatch;
  const auto bctr = A.bctr;
  const auto x = A.x;
  const auto y = A.y;
  const auto ro = A.ro;
  const auto seg = A.seg;
  const auto noise = A.noise;
  const auto nnoise = A.nnoise;
  const auto seed = A.seed;
  const auto nctr = A.nctr;
  const auto done = A.done;
  const auto grad = A.grad;
  const auto ngrad = A.ngrad;
  const uint64_t base = (uint64_t)nctr[0];
  const int64_t tid = (int64_t)wg * blockDim.x + threadIdx.x, stride = (int64_t)nwg * blockDim.x;
  for (int64_t q = tid; q * 4 < nnoise; q += stride) normal_quad<T>(noise, nnoise, seed, base, q);
  if ((((uintptr_t)grad) & 15) == 0) {      // 16-byte stores
    constexpr int V = 16 / (int)sizeof(T);
    struct alignas(16) Z { T e[V]; };
    const Z z{};
    const int64_t nv = ngrad / V;
    for (int64_t i = tid; i < nv; i += stride) ((Z*)grad)[i] = z;
    for (int64_t i = nv * V + tid; i < ngrad; i += stride) grad[i] = (T)0;
  } else {
    for (int64_t i = tid; i < ngrad; i += stride) grad[i] = (T)0;
  }
  if (wg == 0) {
    const int64_t b = bctr[0] % nbatch;
    for (int64_t i = threadIdx.x; i < B; i += blockDim.x) {
      x[i] = Xb[b * B + i];
      y[i] = Yb[b * B + i];
      ro[i] = Ib[b * B + i];
    }
    for (int64_t i = threadIdx.x; i < nseg; i += blockDim.x) seg[i] = Sb[b * nseg + i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (wg == 0) bctr[0] += 1;
    const int old = __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == nwg - 1) {
      nctr[0] += 1;
      __hip_atomic_store(done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace nmgp
