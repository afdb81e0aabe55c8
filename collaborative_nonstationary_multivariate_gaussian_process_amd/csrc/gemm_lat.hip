// Latency-oriented grouped GEMM for the short-k products of the DSVI step (same descriptors and
// semantics as gemm.hip's grouped kernel; the host picks this kernel per group, hip_ops.GemmGroup).
//
// The step's GEMMs are B x M x M and M x M x M products with k = M = 256 (projections T = K12 C^-T,
// P = T C^-1, the quadratic-form factors W = P L, the P-bar / R adjoints, C^-T C^-1): 0.1-1 GFLOP
// each, a few hundred 64x64 tiles, 4-8 k-tiles per tile.  There the LDS-staged kernel waits on one
// global round trip per k-tile and on split-K hand-offs, and reaches 5-18% MFMA-busy.  This kernel
// is shaped for latency instead:
//   * 32x32 output tile per workgroup, the k range split over its waves in 32- or 64-wide panels (wave w
//     takes panels w, w+LW, ...), partial tiles summed through LDS in wave order (deterministic);
//   * no LDS staging of operands: each lane loads exactly the MFMA operands it feeds, straight into
//     registers, all of a panel's loads in flight at once.  The k index is permuted inside a panel
//     (MFMA step s, k-slot g = lane >> 4 takes k = kp + NV g + s, NV = panel / 4), so a lane's NV
//     values of one row of A (or column of B) are consecutive in k: 16-byte loads for a k-contiguous
//     operand, or a 128-byte segment across 16 lanes per load (k step in the scalar offset) for an
//     m/n-contiguous one;
//   * XCD-aware tile order: workgroup b runs on XCD b % 8 and gets tile (b % 8) * per + b / 8, so all
//     column tiles of a row block (which share its A rows) run on one XCD and hit its L2.
// Masks (bounds, triangular operands, k tail), k-blocked operands (kb % 64 == 0), segment-table row
// and k ranges, k-scaling, output masks and the beta / rs(i) E / diagonal epilogue follow
// nmgp_gemm_desc exactly.  Long k ranges (the M x M x B reductions over the minibatch) are also split
// over workgroups (desc.ksplit), partials combined by the last arriving chunk in chunk order.
#include "common.hpp"
#include "lat_tile.hpp"

namespace nmgp {
namespace {

template <typename T, int LW, int LKP, int OCC>
__global__ __launch_bounds__(64 * LW, OCC) void gemm_lat_kernel(LatArgs args,
                                                                             const nmgp_gemm_desc* __restrict__ descs,
                                                                             const int32_t* __restrict__ dyn) {
  __shared__ T red[LW * LTM * LTN];
  lat_walk<T, LW, LKP>(args, descs, dyn, (int)blockIdx.x, (int)gridDim.x, red);
}

// the next tile with output in this workgroup's sequence b, b + gridDim.x, ... (b advanced past it)
template <typename T, int LW, int LKP>
__device__ __forceinline__ bool lat_next(const LatArgs& args, const nmgp_gemm_desc* __restrict__ descs,
                                         const int32_t* __restrict__ dyn, int total, int per, int lim, int& b,
                                         LatJob& J) {
  for (; b < lim; b += gridDim.x) {
    const int tile = (b & 7) * per + (b >> 3);
    if (tile < total && lat_decode<T, LW, LKP>(args, descs, dyn, tile, b == (int)blockIdx.x, J)) {
      b += gridDim.x;
      return true;
    }
  }
  return false;
}

// Persistent form for launches with more tiles than one round of workgroups (round 6): one
// workgroup per CU walks its tiles (the same XCD-chunked order as gemm_lat_kernel) with two tiles in flight -- the
// first panel of the next tile is loaded before the current tile's MFMAs and LDS reduction, so its global round
// trip hides under them.  Each tile is computed exactly as gemm_lat_kernel computes it (same panels per wave, same
// reduction order): results are bit-identical to the non-persistent launch.
template <typename T, int LW, int LKP>
__global__ __launch_bounds__(64 * LW, 1) void gemm_lat_pipe_kernel(LatArgs args,
                                                                   const nmgp_gemm_desc* __restrict__ descs,
                                                                   const int32_t* __restrict__ dyn) {
  __shared__ T red[LW * LTM * LTN];
  constexpr int NV = LKP / 4;
  const int total = __builtin_amdgcn_readfirstlane(dyn ? dyn[args.nprob] : args.total);
  const int per = (total + 7) >> 3;
  const int lim = 8 * per;
  int b = blockIdx.x;
  LatJob J0, J1;
  T a0[2][NV], b0[2][NV], a1[2][NV], b1[2][NV];
  bool h0 = lat_next<T, LW, LKP>(args, descs, dyn, total, per, lim, b, J0);
  if (h0) lat_load_first<T, LW, LKP>(J0, descs, a0, b0);
  while (h0) {
    const bool h1 = lat_next<T, LW, LKP>(args, descs, dyn, total, per, lim, b, J1);
    if (h1) lat_load_first<T, LW, LKP>(J1, descs, a1, b1);
    lat_run<T, LW, LKP>(args, descs, J0, a0, b0, red);
    __syncthreads();
    if (!h1) break;
    h0 = lat_next<T, LW, LKP>(args, descs, dyn, total, per, lim, b, J0);
    if (h0) lat_load_first<T, LW, LKP>(J0, descs, a0, b0);
    lat_run<T, LW, LKP>(args, descs, J1, a1, b1, red);
    __syncthreads();
  }
}

// Tile plan of a grouped launch for this minibatch (as gemm.hip's plan kernel, 32-row tiles).
__global__ __launch_bounds__(256) void lat_plan_kernel(const nmgp_gemm_desc* __restrict__ descs, int nprob,
                                                       const int32_t* __restrict__ seg, int32_t* dyn_start) {
  __shared__ int buf[256];
  __shared__ int carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nprob; base += 256) {
    const int p = base + t;
    int v = 0;
    if (p < nprob) {
      const nmgp_gemm_desc& d = descs[p];
      int tm = d.tiles_m;
      if (d.row_seg >= 0 && seg != nullptr) {
        const int span = d.seg_span > 0 ? d.seg_span : 1;
        const int m = seg[d.row_seg + span] - seg[d.row_seg];
        tm = min(tm, max(0, (m + LTM - 1) / LTM));
      }
      v = tm * d.tiles_n * (d.ksplit > 1 ? d.ksplit : 1);
    }
    buf[t] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
      const int add = t >= off ? buf[t - off] : 0;
      __syncthreads();
      buf[t] += add;
      __syncthreads();
    }
    if (p < nprob) dyn_start[p] = carry + buf[t] - v;
    __syncthreads();
    if (t == 255) carry += buf[255];
    __syncthreads();
  }
  if (t == 0) dyn_start[nprob] = carry;
}

template <typename T>
int launch_lat(const nmgp_gemm_desc* d_desc, int nprob, int total_tiles, const int32_t* d_seg, int32_t* d_plan,
               int grid, hipStream_t s, bool planned = false, bool pipe = false) {
  if (d_desc == nullptr) return -1;
  if (nprob <= 0) return -2;
  if (total_tiles < 0) return -3;
  if (total_tiles == 0) return NMGP_OK;
  LatArgs a;
  a.descs = d_desc;
  a.nprob = nprob;
  a.total = total_tiles;
  a.seg = d_seg;
  a.dyn_start = nullptr;
  int wgs = ((total_tiles + 7) / 8) * 8;
  if (d_plan != nullptr) {
    if (!planned) {
      hipLaunchKernelGGL(lat_plan_kernel, dim3(1), dim3(256), 0, s, d_desc, nprob, d_seg, d_plan);
      NMGP_CHECK_LAUNCH();
    }
    a.dyn_start = d_plan;
    if (grid > 0) wgs = min(wgs, ((grid + 7) / 8) * 8);   // a multiple of 8 keeps each workgroup on one XCD chunk
  }
  if (pipe) {
    // persistent: one workgroup per CU (the XCD chunking needs a multiple of 8), never more than the tiles
    static int n_cu = 0;
    if (n_cu == 0) {
      int dev = 0, v = 0;
      if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) ==
                                                  hipSuccess && v > 0)
        n_cu = v;
      else
        n_cu = 256;
    }
    wgs = min(wgs, max(8, (n_cu / 8) * 8));
    hipLaunchKernelGGL((gemm_lat_pipe_kernel<T, 8, 32>), dim3(wgs), dim3(512), 0, s, a, d_desc, a.dyn_start);
    NMGP_CHECK_LAUNCH();
    return NMGP_OK;
  }
  // 8 waves x 32-wide panels with registers capped at 128 so two workgroups share a CU (round 2: PM2.5 step +1%
  // over one workgroup per CU).  hip_ops.GemmGroup sizes split-K for 8 waves x 32.
  hipLaunchKernelGGL((gemm_lat_kernel<T, 8, 32, 4>), dim3(wgs), dim3(512), 0, s, a, d_desc, a.dyn_start);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

}  // namespace
}  // namespace nmgp

extern "C" {
int nmgp_gemm_grouped_lat_f64(const nmgp_gemm_desc* d, int np, int tt, const int32_t* seg, int32_t* plan, int grid,
                              hipStream_t s) {
  return nmgp::launch_lat<double>(d, np, tt, seg, plan, grid, s);
}
int nmgp_gemm_grouped_lat_f32(const nmgp_gemm_desc* d, int np, int tt, const int32_t* seg, int32_t* plan, int grid,
                              hipStream_t s) {
  return nmgp::launch_lat<float>(d, np, tt, seg, plan, grid, s);
}
int nmgp_gemm_plan_lat(const nmgp_gemm_desc* d, int np, const int32_t* seg, int32_t* plan, hipStream_t s) {
  if (!d || !plan) return -1;
  if (np <= 0) return -2;
  hipLaunchKernelGGL(nmgp::lat_plan_kernel, dim3(1), dim3(256), 0, s, d, np, seg, plan);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}
int nmgp_gemm_grouped_lat_planned_f64(const nmgp_gemm_desc* d, int np, int tt, const int32_t* seg, int32_t* plan,
                                      int grid, hipStream_t s) {
  if (!plan) return -5;
  return nmgp::launch_lat<double>(d, np, tt, seg, plan, grid, s, true);
}
int nmgp_gemm_grouped_lat_planned_f32(const nmgp_gemm_desc* d, int np, int tt, const int32_t* seg, int32_t* plan,
                                      int grid, hipStream_t s) {
  if (!plan) return -5;
  return nmgp::launch_lat<float>(d, np, tt, seg, plan, grid, s, true);
}
// persistent two-tiles-in-flight launches (same arguments; planned != 0: the device tile plan is already computed)
int nmgp_gemm_grouped_lat_pipe_f64(const nmgp_gemm_desc* d, int np, int tt, const int32_t* seg, int32_t* plan,
                                   int planned, hipStream_t s) {
  if (planned && !plan) return -5;
  return nmgp::launch_lat<double>(d, np, tt, seg, plan, 0, s, planned != 0, true);
}
int nmgp_gemm_grouped_lat_pipe_f32(const nmgp_gemm_desc* d, int np, int tt, const int32_t* seg, int32_t* plan,
                                   int planned, hipStream_t s) {
  if (planned && !plan) return -5;
  return nmgp::launch_lat<float>(d, np, tt, seg, plan, 0, s, planned != 0, true);
}
}
