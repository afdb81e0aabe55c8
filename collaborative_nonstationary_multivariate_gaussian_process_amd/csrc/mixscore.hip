// Exact scores of equal-weight Gaussian mixtures: CRPS, PIT and quantiles of the predictives that summarize_Y and
// impute_Y end in.  The reference has no such code; the inputs are the component buffers the merged kernels collect
// (Mu / Var (S, E) of ycond.hip, F (S, N) of ysum.hip with one scalar variance).  fp64, no matrix cores.
//
// Per entry e the components are (mu_s, v_s), s < S, sigma_s = sqrt(v_s), the truth y:
//   A(m, v) = m erf(m / sqrt(2 v)) + sqrt(2 v / pi) exp(-m^2 / (2 v))      (both summands >= 0)
//   pit = (1/S) sum_s Phi((y - mu_s) / sigma_s),   t1 = (1/S) sum_s A(y - mu_s, v_s),
//   t2 = (sum_{t<s} A(mu_s - mu_t, v_s + v_t) + sum_s sigma_s / sqrt(pi)) / S^2   (the spread),   crps = t1 - t2,
//   q_p: the root of F(q) = (1/S) sum_s Phi((q - mu_s) / sigma_s) = p, bisected from the bracket
//        [min_s, max_s](mu_s + z_p sigma_s) widened by 1e-12 max_s(|mu_s| + |z_p| sigma_s) until no double lies
//        strictly between its ends; the end with the smaller |F - p| is returned.
//
// Layout.  The component axis is the slow one, so a workgroup serves kMsEnt = 8 ADJACENT entries: every row access
// of a wave is 8 rows x one 64-byte segment, never an 8-byte column walk.  Thread t of the 256 owns entry t & 7 and
// is s-lane t >> 3 of its 32.
//
// Pair kernel (the hot loop, S^2 / 2 terms per entry): the components are cut into tiles of kMsTile = 128; the
// lower triangle of tile pairs (I, J <= I) in row-major order is cut into nsl = min(#pairs, 64) slices of equal
// pair counts, a function of S alone.  A workgroup = (8 entries, slice).  Per tile pair the thread holds
// kMsR = 4 components s = 128 I + lane + 32 r in registers and walks the 128 components t of tile J through LDS
// (one ds_read of (mu_t, v_t), shared by the 4 s-lanes of the entry in the lane group, feeds 4 pair terms);
// on a diagonal tile pair only t < s counts.  The thread's 4 accumulators are added in a fixed order, then the 32
// s-lanes of an entry by a xor butterfly inside the wave and the 4 waves in wave order; the slice's partial goes to
// ws[slice * E + e].  The entry kernel adds the partials in slice order.  No floating-point atomics: the same call
// gives the same bits, and an entry's bits do not depend on which other entries are in the call.
//
// Entry kernel (O(S) per entry and O(S steps) per quantile): the same workgroup shape; one pass gives sum sigma,
// the validity of the entry, pit and t1; per quantile one pass gives the bracket and every bisection step is one
// pass with one workgroup reduction.  A quantile that is not down to adjacent doubles after kMsSteps steps is
// written as NaN and counted in *unconverged (an integer atomic).
//
// With one scalar variance (HET = false: the homoscedastic summarize_Y case) sigma, the pair sigma sqrt(2 v) and
// their reciprocals are hoisted out of every loop: a compile-time variant.
#include "common.hpp"

namespace nmgp {

constexpr int kMsEnt = 8;                            // adjacent entries of a workgroup: 64-byte row segments
constexpr int kMsLanes = 32;                         // s-lanes per entry
constexpr int kMsR = 4;                              // components a thread holds in registers
constexpr int kMsTile = kMsLanes * kMsR;             // components per tile
constexpr int kMsThreads = kMsEnt * kMsLanes;
constexpr int kMsWaves = kMsThreads / 64;
constexpr int kMsMaxSlices = 64;
constexpr int kMsMaxQ = 16;
constexpr int kMsMaxS = 1 << 20;                     // 8192 tiles: the tile-pair count fits an int
constexpr int kMsSteps = 200;                        // bisection steps before a quantile counts as unconverged
constexpr double kInvSqrt2 = 0.70710678118654752440;
constexpr double kSqrt2OverPi = 0.79788456080286535588;
constexpr double kInvSqrtPi = 0.56418958354775628695;

struct MsQ {
  double z[kMsMaxQ], p[kMsMaxQ];
  int nq;
};

struct MsOut {
  double *pit, *crps, *spread, *quant;
  int64_t ld_q;
  int* unconverged;
};

// tile pairs of the triangle and slices: functions of S alone
inline void ms_slicing(int S, int* ntp, int* nsl) {
  const int64_t nt = (S + kMsTile - 1) / kMsTile, n = S < 2 ? 0 : nt * (nt + 1) / 2;
  *ntp = (int)n;
  *nsl = (int)(n < kMsMaxSlices ? n : kMsMaxSlices);
}

__device__ inline int ms_tri_row(int k) {            // the I with I (I + 1) / 2 <= k < (I + 1) (I + 2) / 2
  int i = (int)((sqrtf(8.0f * (float)k + 1.0f) - 1.0f) * 0.5f);
  while ((int64_t)i * (i + 1) / 2 > k) --i;
  while ((int64_t)(i + 1) * (i + 2) / 2 <= k) ++i;
  return i;
}

struct MsAdd { __device__ static double op(double a, double b) { return a + b; } };
struct MsMin { __device__ static double op(double a, double b) { return fmin(a, b); } };
struct MsMax { __device__ static double op(double a, double b) { return fmax(a, b); } };

// K reductions over the 32 s-lanes of every entry of the workgroup: a xor butterfly over the lanes of the entry in
// the wave, then the waves in wave order.  The order does not depend on the entry's place in the workgroup; the
// result is valid in every thread of the entry.  red: K * kMsWaves * kMsEnt doubles.
template <typename Op, int K> __device__ inline void ms_ent_reduce(double (&v)[K], double* red) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = tid & (kMsEnt - 1);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = Op::op(v[k], __shfl_xor(v[k], 8, 64));
    v[k] = Op::op(v[k], __shfl_xor(v[k], 16, 64));
    v[k] = Op::op(v[k], __shfl_xor(v[k], 32, 64));
  }
  __syncthreads();                                   // red is free
  if (lane < kMsEnt) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[(k * kMsWaves + w) * kMsEnt + j] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = red[k * kMsWaves * kMsEnt + j];
#pragma unroll
    for (int i = 1; i < kMsWaves; ++i) s = Op::op(s, red[(k * kMsWaves + i) * kMsEnt + j]);
    v[k] = s;
  }
}

// A(m, v) with sig = sqrt(v) and, in the scalar-variance variant, its hoisted reciprocal
template <bool HET> __device__ inline double ms_A(double m, double sig, double rsig) {
  const double z = HET ? m / sig : m * rsig;
  return fma(m, erf(z * kInvSqrt2), sig * kSqrt2OverPi * exp(-0.5 * z * z));
}

template <bool HET>
__global__ __launch_bounds__(kMsThreads) void mix_pair_kernel(const double* __restrict__ Mu, int64_t ld_mu,
                                                              const double* __restrict__ Var, int64_t ld_var,
                                                              double v0, int S, int64_t E, int ntp, int nsl,
                                                              double* __restrict__ ws) {
  __shared__ double tmu[kMsTile * kMsEnt];
  __shared__ double tv[HET ? kMsTile * kMsEnt : 1];
  __shared__ double red[kMsWaves * kMsEnt];
  const int tid = threadIdx.x, j = tid & (kMsEnt - 1), sl = tid >> 3, wave = uniform32(tid >> 6);
  const int64_t e = (int64_t)blockIdx.x * kMsEnt + j;
  const bool live = e < E;
  const int slice = blockIdx.y;
  const int k0 = (int)((int64_t)slice * ntp / nsl), k1 = (int)((int64_t)(slice + 1) * ntp / nsl);
  const double sig0 = sqrt(2.0 * v0), rsig0 = 1.0 / sig0;      // the pair sigma of the scalar variant

  double acc[kMsR], ms[kMsR], vs[kMsR];
  bool ok[kMsR];
#pragma unroll
  for (int r = 0; r < kMsR; ++r) {
    acc[r] = ms[r] = 0.0;
    vs[r] = 1.0;
    ok[r] = false;
  }
  int Icur = -1;
  for (int k = k0; k < k1; ++k) {
    const int I = ms_tri_row(k), J = k - (int)((int64_t)I * (I + 1) / 2);
    if (I != Icur) {
      Icur = I;
#pragma unroll
      for (int r = 0; r < kMsR; ++r) {
        const int64_t s = (int64_t)I * kMsTile + sl + kMsLanes * r;
        ok[r] = live && s < S;
        ms[r] = ok[r] ? Mu[s * ld_mu + e] : 0.0;
        if (HET) vs[r] = ok[r] ? Var[s * ld_var + e] : 1.0;
      }
    }
    __syncthreads();                                 // the previous tile has been read
#pragma unroll
    for (int q = 0; q < kMsR; ++q) {                 // tile J -> LDS: row tt of the tile, this thread's entry
      const int tt = sl + kMsLanes * q;
      const int64_t t = (int64_t)J * kMsTile + tt;
      const bool in = live && t < S;
      tmu[tt * kMsEnt + j] = in ? Mu[t * ld_mu + e] : 0.0;
      if (HET) tv[tt * kMsEnt + j] = in ? Var[t * ld_var + e] : 1.0;
    }
    __syncthreads();
    const int tcount = min(kMsTile, S - J * kMsTile);
    double a[kMsR] = {0.0, 0.0, 0.0, 0.0};
    if (I == J) {                                    // diagonal tile pair: t < s only
      const int bound = min(tcount, wave * 8 + 8 + kMsLanes * (kMsR - 1));
      for (int tt = 0; tt < bound; ++tt) {
        const double mt = tmu[tt * kMsEnt + j];
        const double vt = HET ? tv[tt * kMsEnt + j] : 0.0;
#pragma unroll
        for (int r = 0; r < kMsR; ++r) {
          const double sig = HET ? sqrt(vs[r] + vt) : sig0;
          const double term = ms_A<HET>(ms[r] - mt, sig, rsig0);
          a[r] += tt < sl + kMsLanes * r ? term : 0.0;
        }
      }
    } else {
      for (int tt = 0; tt < tcount; ++tt) {
        const double mt = tmu[tt * kMsEnt + j];
        const double vt = HET ? tv[tt * kMsEnt + j] : 0.0;
#pragma unroll
        for (int r = 0; r < kMsR; ++r) {
          const double sig = HET ? sqrt(vs[r] + vt) : sig0;
          a[r] += ms_A<HET>(ms[r] - mt, sig, rsig0);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kMsR; ++r) acc[r] += ok[r] ? a[r] : 0.0;
  }
  double tot[1] = {(acc[0] + acc[1]) + (acc[2] + acc[3])};
  ms_ent_reduce<MsAdd>(tot, red);
  if (tid < kMsEnt && live) ws[(int64_t)slice * E + e] = tot[0];
}

template <bool HET>
__global__ __launch_bounds__(kMsThreads) void mix_entry_kernel(const double* __restrict__ Mu, int64_t ld_mu,
                                                               const double* __restrict__ Var, int64_t ld_var,
                                                               double v0, int S, int64_t E,
                                                               const double* __restrict__ y, MsQ Q,
                                                               const double* __restrict__ ws, int nsl, MsOut o) {
  __shared__ double red[4 * kMsWaves * kMsEnt];
  const int tid = threadIdx.x, j = tid & (kMsEnt - 1), sl = tid >> 3;
  const int64_t e = (int64_t)blockIdx.x * kMsEnt + j;
  const bool live = e < E;
  const double nan = __builtin_nan("");
  const double sig0 = sqrt(v0), rsig0 = 1.0 / sig0;
  const double yv = (y && live) ? y[e] : nan;

  // ---- one pass: sum sigma, validity, pit and t1
  double r4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t s = sl; s < S; s += kMsLanes) {
    const double m = live ? Mu[s * ld_mu + e] : 0.0;
    const double v = HET ? (live ? Var[s * ld_var + e] : 1.0) : v0;
    if (!(__builtin_isfinite(m) && __builtin_isfinite(v) && v > 0.0)) r4[3] = 1.0;
    const double sig = HET ? sqrt(v) : sig0;
    r4[0] += sig;
    if (y) {
      const double d = yv - m;
      const double z = HET ? d / sig : d * rsig0;
      r4[1] += 0.5 * erfc(-z * kInvSqrt2);
      r4[2] += fma(d, erf(z * kInvSqrt2), sig * kSqrt2OverPi * exp(-0.5 * z * z));
    }
  }
  ms_ent_reduce<MsAdd>(r4, red);
  const bool bad = !(r4[3] == 0.0);
  if (tid < kMsEnt && live) {
    const bool yok = __builtin_isfinite(yv);
    if (o.crps || o.spread) {
      double P = 0.0;
      for (int k = 0; k < nsl; ++k) P += ws[(int64_t)k * E + e];          // slice order
      const double t2 = (P + r4[0] * kInvSqrtPi) / ((double)S * (double)S);
      if (o.spread) o.spread[e] = bad ? nan : t2;
      if (o.crps) o.crps[e] = bad || !yok ? nan : r4[2] / (double)S - t2;
    }
    if (o.pit) o.pit[e] = bad || !yok ? nan : r4[1] / (double)S;
  }

  // ---- quantiles: bracket, then bisection down to adjacent doubles
  for (int q = 0; q < Q.nq; ++q) {
    const double zq = Q.z[q], pq = Q.p[q], az = fabs(zq);
    double lo[1] = {INFINITY}, hi[2] = {-INFINITY, 0.0};
    for (int64_t s = sl; s < S; s += kMsLanes) {
      const double m = live ? Mu[s * ld_mu + e] : 0.0;
      const double sig = HET ? sqrt(live ? Var[s * ld_var + e] : 1.0) : sig0;
      const double c = fma(zq, sig, m);
      lo[0] = fmin(lo[0], c);
      hi[0] = fmax(hi[0], c);
      hi[1] = fmax(hi[1], fma(az, sig, fabs(m)));
    }
    ms_ent_reduce<MsMin>(lo, red);
    ms_ent_reduce<MsMax>(hi, red);
    double a = lo[0] - 1e-12 * hi[1], b = hi[0] + 1e-12 * hi[1];
    double fa = INFINITY, fb = INFINITY;             // |F - p| at the ends, where they were evaluated
    bool done = bad || !live, conv = false;
    for (int step = 0; step <= kMsSteps; ++step) {
      const double mid = a + 0.5 * (b - a);
      if (!done && !(mid > a && mid < b)) done = conv = true;
      if (step == kMsSteps || !__syncthreads_or(!done)) break;
      double F[1] = {0.0};
      for (int64_t s = sl; s < S; s += kMsLanes) {
        const double m = live ? Mu[s * ld_mu + e] : 0.0;
        const double d = mid - m;
        const double z = HET ? d / sqrt(live ? Var[s * ld_var + e] : 1.0) : d * rsig0;
        F[0] += 0.5 * erfc(-z * kInvSqrt2);
      }
      ms_ent_reduce<MsAdd>(F, red);
      if (!done) {
        const double res = F[0] / (double)S - pq;
        if (res < 0.0) {
          a = mid;
          fa = -res;
        } else {
          b = mid;
          fb = res;
        }
      }
    }
    if (tid < kMsEnt && live) {
      o.quant[(int64_t)q * o.ld_q + e] = bad || !conv ? nan : (fa <= fb ? a : b);
      if (!bad && !conv) atomicAdd(o.unconverged, 1);
    }
  }
}

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int64_t nmgp_mix_score_workspace_size(int S, int64_t E) {
  if (S < 1 || S > kMsMaxS || E <= 0) return 0;
  int ntp, nsl;
  ms_slicing(S, &ntp, &nsl);
  return (int64_t)nsl * E * (int64_t)sizeof(double);
}

int nmgp_mix_score_f64(const double* Mu, int64_t ld_mu, const double* Var, int64_t ld_var, double var_scalar, int S,
                       int64_t E, const double* y, const double* z_p, const double* p, int nq, double* pit,
                       double* crps, double* spread, double* quantiles, int64_t ld_q, int32_t* unconverged, void* ws,
                       int64_t ws_bytes, hipStream_t stream) {
  if (S < 1 || S > kMsMaxS || E < 0 || nq < 0 || nq > kMsMaxQ) return NMGP_ERR_MIX_ARG;
  if (E > (int64_t)0x7fffffff * kMsEnt) return NMGP_ERR_MIX_ARG;
  if (nq > 0 && (!z_p || !p)) return NMGP_ERR_MIX_ARG;
  MsQ Q;
  Q.nq = nq;
  for (int k = 0; k < nq; ++k) {
    if (!(p[k] > 0.0 && p[k] < 1.0) || z_p[k] - z_p[k] != 0.0) return NMGP_ERR_MIX_ARG;
    Q.z[k] = z_p[k];
    Q.p[k] = p[k];
  }
  if (E == 0) return NMGP_OK;                        // no entry: nothing to launch, and no buffer to point at
  if ((pit || crps) && !y) return NMGP_ERR_MIX_ARG;
  if (nq > 0 && (!quantiles || !unconverged || ld_q < E)) return NMGP_ERR_MIX_ARG;
  if (!Mu || ld_mu < E) return NMGP_ERR_MIX_ARG;
  if (Var ? ld_var < E : !(var_scalar > 0.0 && var_scalar - var_scalar == 0.0)) return NMGP_ERR_MIX_ARG;
  if (!pit && !crps && !spread && nq == 0) return NMGP_ERR_MIX_ARG;
  int ntp, nsl;
  ms_slicing(S, &ntp, &nsl);
  const bool pairs = crps || spread;
  if (pairs && !ws_covers((int64_t)nsl * E * (int64_t)sizeof(double), ws, ws_bytes)) return NMGP_ERR_MIX_ARG;
  const unsigned nblk = (unsigned)((E + kMsEnt - 1) / kMsEnt);
  const MsOut o = {pit, crps, spread, quantiles, ld_q, (int*)unconverged};
  const double* yy = (pit || crps) ? y : nullptr;
  if (pairs && nsl > 0) {
    if (Var)
      hipLaunchKernelGGL(mix_pair_kernel<true>, dim3(nblk, (unsigned)nsl), dim3(kMsThreads), 0, stream, Mu, ld_mu,
                         Var, ld_var, 0.0, S, E, ntp, nsl, (double*)ws);
    else
      hipLaunchKernelGGL(mix_pair_kernel<false>, dim3(nblk, (unsigned)nsl), dim3(kMsThreads), 0, stream, Mu, ld_mu,
                         (const double*)nullptr, (int64_t)0, var_scalar, S, E, ntp, nsl, (double*)ws);
    NMGP_CHECK_LAUNCH();
  }
  if (Var)
    hipLaunchKernelGGL(mix_entry_kernel<true>, dim3(nblk), dim3(kMsThreads), 0, stream, Mu, ld_mu, Var, ld_var, 0.0,
                       S, E, yy, Q, (const double*)ws, nsl, o);
  else
    hipLaunchKernelGGL(mix_entry_kernel<false>, dim3(nblk), dim3(kMsThreads), 0, stream, Mu, ld_mu,
                       (const double*)nullptr, (int64_t)0, var_scalar, S, E, yy, Q, (const double*)ws, nsl, o);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

}  // extern "C"
