// The start of a captured training step in ONE launch: step_begin_kernel (minibatch gather, Philox noise, gradient
// zeroing), the pairwise launch that builds the three RBF K22 + lam I and the grouped-GEMM launch that forms
// Sigma_v + lam I = tril(S_v) tril(S_v)^T + lam I.  The two builders read only theta, yet as launches of their own they
// sat on the main chain behind step_begin, each behind a graph hand-off, and the first fused factorization started
// ~34 us after the minibatch was ready.  Here the three are independent sets of workgroups of one grid:
//
//   [0, nlat)                  Sigma_v: workgroup b walks the tiles of the grouped-GEMM launch exactly as workgroup b
//                              of gemm_lat_kernel<T, 8, 32, 4> does (lat_walk; nlat is that launch's grid, a multiple
//                              of 8, so the XCD-chunked tile order is the same too)
//   [nlat, nlat + npw)         K22: pairwise tiles, TWO per workgroup (the pairwise body is written for 256 threads;
//                              threads 0..255 take tile 2w, threads 256..511 tile 2w + 1 -- the body has no barrier)
//   [nlat + npw, .. + nbegin)  begin: step_begin_body; the arrival word counts these workgroups only
//
// The builders come first in the grid: they are what the next launch (the fused factorization) waits for.  No workgroup
// waits for another; every value is computed by the shared bodies (lat_tile.hpp, pairwise_tile.hpp, step_begin.hpp),
// so the results are those of the three launches bit for bit.
#include "common.hpp"
#include "lat_tile.hpp"
#include "pairwise_tile.hpp"
#include "step_begin.hpp"

namespace nmgp {
namespace {

constexpr int HEAD_LW = 8, HEAD_LKP = 32;      // the gemm_lat instance of the step's Sigma_v launch

template <typename T>
__global__ __launch_bounds__(64 * HEAD_LW, 4) void step_head_kernel(BeginArgs<T> beg, int nbegin, PwArgs pw, int pw_tiles,
                                                                    int npw, LatArgs lat,
                                                                    const nmgp_gemm_desc* __restrict__ descs, int nlat) {
  __shared__ T red[HEAD_LW * LTM * LTN];
  const int b = (int)blockIdx.x;
  if (b < nlat) {
    lat_walk<T, HEAD_LW, HEAD_LKP>(lat, descs, nullptr, b, nlat, red);
  } else if (b < nlat + npw) {
    const int tile = 2 * (b - nlat) + ((int)threadIdx.x >> 8);
    if (tile < pw_tiles) pairwise_tile<T>(pw, tile, (int)threadIdx.x & 255);
  } else {
    step_begin_body<T>(beg, b - nlat - npw, nbegin);
  }
}

template <typename T>
int step_head(const T* Xb, const T* Yb, const int32_t* Ib, const int32_t* Sb, int64_t B, int64_t nseg, int64_t nbatch,
              int64_t* bctr, T* x, T* y, int32_t* ro, int32_t* seg, T* noise, int64_t nnoise, uint64_t seed,
              int64_t* nctr, int32_t* done, T* grad, int64_t ngrad, const nmgp_pairwise_desc* pw, int npd, int pw_tiles,
              const nmgp_gemm_desc* gd, int ngd, int lat_tiles, const int32_t* lat_seg, hipStream_t s) {
  if (!Xb || !Yb || !Ib || !Sb) return -1;
  if (B <= 0 || nseg <= 0 || nbatch <= 0) return -5;
  if (!bctr) return -8;
  if (!x || !y || !ro || !seg) return -9;
  if (!noise || nnoise < 0 || !nctr || !done) return -13;
  if (!grad || ngrad < 0) return -18;
  if (!pw || npd <= 0 || pw_tiles <= 0) return -20;
  if (!gd || ngd <= 0 || lat_tiles <= 0) return -23;
  // the begin workgroups cover the work of step_begin_kernel's grid (at most 256 workgroups of 256 threads) at 512
  const int64_t work = std::max((nnoise + 3) / 4, ngrad);
  const int nbegin = (int)std::max<int64_t>(1, std::min<int64_t>((work + 511) / 512, 128));
  const int npw = (pw_tiles + 1) / 2;
  const int nlat = ((lat_tiles + 7) / 8) * 8;
  BeginArgs<T> beg{Xb, Yb, Ib, Sb, B, nseg, nbatch, bctr, x, y, ro, seg, noise, nnoise, seed, nctr, done, grad, ngrad};
  PwArgs pa;
  pa.descs = pw;
  pa.nd = npd;
  pa.inl = nmgp_pairwise_desc{};
  LatArgs la;
  la.descs = gd;
  la.nprob = ngd;
  la.total = lat_tiles;
  la.seg = lat_seg;     // (segment table of row- or k-segmented problems; NULL when the group has none)
  la.dyn_start = nullptr;
  hipLaunchKernelGGL(step_head_kernel<T>, dim3((unsigned)(nlat + npw + nbegin)), dim3(64 * HEAD_LW), 0, s, beg, nbegin, pa,
                     pw_tiles, npw, la, gd, nlat);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

}  // namespace
}  // namespace nmgp

extern "C" {
#define NMGP_STEP_HEAD(T, sfx)                                                                                       \
  int nmgp_step_head_##sfx(const T* Xb, const T* Yb, const int32_t* Ib, const int32_t* Sb, int64_t B, int64_t nseg,  \
                           int64_t nbatch, int64_t* bctr, T* x, T* y, int32_t* ro, int32_t* seg, T* noise,           \
                           int64_t nnoise, uint64_t seed, int64_t* nctr, int32_t* done, T* grad, int64_t ngrad,      \
                           const nmgp_pairwise_desc* pw, int npd, int pw_tiles, const nmgp_gemm_desc* gd, int ngd,   \
                           int lat_tiles, const int32_t* lat_seg, hipStream_t s) {                                   \
    return nmgp::step_head<T>(Xb, Yb, Ib, Sb, B, nseg, nbatch, bctr, x, y, ro, seg, noise, nnoise, seed, nctr, done,  \
                              grad, ngrad, pw, npd, pw_tiles, gd, ngd, lat_tiles, lat_seg, s);                       \
  }
NMGP_STEP_HEAD(double, f64)
NMGP_STEP_HEAD(float, f32)
#undef NMGP_STEP_HEAD
}
