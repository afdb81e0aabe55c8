// Local stationary fits around the inducing points: the reference's pre_estimation_partial (code/pre_nmgp.py:102-125,
// imported as nmgp_dsvi.pre_estimation) as one launch, one workgroup per inducing point z_m.  The reference builds
// kron(K, B) + s I (P D x P D) for every likelihood evaluation of a BFGS started at (-6, -6); here the window's
// likelihood is evaluated in its eigen form and minimised by a fixed, bounded search.
//
// Window: the P rows with the smallest |x_n - z_m|, ties to the lower row, kept in ascending row order.  Every thread
// keeps a sorted private top-P of its stride of the scan; the lists are merged by P rounds of a workgroup arg-min over
// the lists' heads (wave butterfly, then the four wave results through LDS).
//
// Likelihood: vec(Y_loc) ~ N(0, K(ell) (x) B + s I), B = V_B diag(mu) V_B^T of all rows (the caller passes mu and
// Yrot = Y V_B), K = V_K diag(lam) V_K^T of the window:
//   nll(log s, log ell) = 1/2 sum_pd [ log G_pd + E_pd / G_pd ] + 1/2 P D log 2 pi,  G_pd = lam_p mu_d + s,
//   E = T o T,  T = V_K^T Yrot_loc.
// K is built as the reference does (divide by ell, then difference; ell < 1e-8 clamped) and diagonalised by the
// parallel cyclic Jacobi of eig.hip on a P x P tile (circle ordering, P / 2 pairs a round, 30 sweeps at most; a
// rotation is skipped at |a_pq| <= max(2^-52 sqrt|a_pp a_qq|, 2^-55): K has a unit diagonal, and its spectrum is
// only needed to the absolute accuracy of lam mu + s; the annihilated pair is stored as an exact zero).  A solve that
// still rotates in its last sweep sets a flag bit.
//
// Arithmetic: plain fp64 VALU.  One evaluation is P^3 Jacobi work per sweep plus P^2 D <= 131k multiply-adds for T,
// against dozens of dependent workgroup reductions per evaluation: the launch is bound by barrier latency, and the
// 16x16x4 matrix-core tile would be mostly padding at P = 10.
//
// Search (tests/_preest_ref.py states the same steps in numpy): box log ell in [log(delta / 4), log(16 span)], delta
// the smallest positive gap of the sorted window inputs, span their range (span = 0: degenerate flag, NaN results);
// log s in log(mean mu) + [-14, 2].  32 log-ell nodes; at each the profile over s: 33 nodes, a safeguarded Newton in
// the bracket one node either side of the best (bisection when the step leaves the bracket; step <= 1e-10 or 60
// iterations), the better of the Newton point and the node kept (the node on a tie).  Then golden section on the
// profiled objective between the nodes either side of the best ell node, to a width of 1e-9 or 64 iterations; the
// answer is the best of the node and the two last interior points (the node on a tie), so an optimum on a box edge
// is the edge itself, and its flag bit is set by equality.  Every loop is capped; every sum has a fixed order (thread
// strides, the DPP wave sum, the waves in order), so a window's bits do not depend on the launch or on the other
// windows in it.  No communication between workgroups.
//
// LDS: Yrot_loc, E and lam mu^T (P x D doubles each, <= 96 KiB together, dynamic), the Jacobi tiles A and V
// (32 x 33 doubles each) and a few vectors (static, 18 KiB).
#include <math.h>

#include "common.hpp"

namespace nmgp {

constexpr int kPeThreads = 256, kPeMaxP = 32, kPeMinP = 3, kPeMaxD = 128, kPeLd = kPeMaxP + 1;
constexpr int kPeSweeps = 30, kPeEllNodes = 32, kPeSNodes = 33, kPeNewton = 60, kPeGolden = 64;
constexpr double kPeNewtonStep = 1e-10, kPeGoldenWidth = 1e-9, kPeGoldenR = 0.6180339887498949;
constexpr double kPeSLo = -14.0, kPeSHi = 2.0, kPeLog2Pi = 1.8378770664093453;
constexpr int kPeFlagEllLo = 1, kPeFlagEllHi = 2, kPeFlagSLo = 4, kPeFlagSHi = 8, kPeFlagJacobi = 16,
              kPeFlagDegenerate = 32;

struct PeShared {
  double A[kPeMaxP * kPeLd], V[kPeMaxP * kPeLd];
  double xs[kPeMaxP], us[kPeMaxP], lam[kPeMaxP], rot[kPeMaxP], srt[kPeMaxP];
  double mu[kPeMaxD];
  double red[48];
  double wd[4];
  double box[4];
  int wi[4];
  int sel[kPeMaxP], idx[kPeMaxP];
  int rotated, jacobi_bad, degenerate;
};

__device__ inline bool pe_less(double d0, int i0, double d1, int i1) { return d0 < d1 || (d0 == d1 && i0 < i1); }

// The window of z_m: s.idx (ascending rows), s.xs, Yl (P x D), s.mu; s.degenerate when fewer than P finite distances.
__device__ void pe_window(PeShared& s, double* Yl, const double* __restrict__ x, int64_t x_stride,
                          const double* __restrict__ Yrot, int64_t ld_y, const double* __restrict__ mu, double zm, int N,
                          int D, int P) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double kd[kPeMaxP];
  int ki[kPeMaxP];
  int cnt = 0;
  for (int n = tid; n < N; n += kPeThreads) {
    const double d = fabs(x[(int64_t)n * x_stride] - zm);
    if (!(d < INFINITY)) continue;
    if (cnt < P || pe_less(d, n, kd[cnt - 1], ki[cnt - 1])) {
      int j = cnt < P ? cnt++ : P - 1;
      while (j > 0 && pe_less(d, n, kd[j - 1], ki[j - 1])) {
        kd[j] = kd[j - 1];
        ki[j] = ki[j - 1];
        --j;
      }
      kd[j] = d;
      ki[j] = n;
    }
  }
  if (tid == 0) s.degenerate = 0;
  int head = 0;
  for (int r = 0; r < P; ++r) {
    double bd = head < cnt ? kd[head] : INFINITY;
    int bi = head < cnt ? ki[head] : 0x7fffffff;
    for (int o = 1; o < 64; o <<= 1) {
      const double od = __shfl_xor(bd, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (pe_less(od, oi, bd, bi)) {
        bd = od;
        bi = oi;
      }
    }
    __syncthreads();
    if (lane == 0) {
      s.wd[w] = bd;
      s.wi[w] = bi;
    }
    __syncthreads();
    bd = s.wd[0];
    bi = s.wi[0];
    for (int k = 1; k < kPeThreads / 64; ++k)
      if (pe_less(s.wd[k], s.wi[k], bd, bi)) {
        bd = s.wd[k];
        bi = s.wi[k];
      }
    if (head < cnt && ki[head] == bi) ++head;
    if (tid == 0) {
      s.sel[r] = bi;
      if (bi == 0x7fffffff) s.degenerate = 1;
    }
  }
  __syncthreads();
  if (tid < P) {
    const int v = s.sel[tid];
    int rank = 0;
    for (int j = 0; j < P; ++j) rank += (s.sel[j] < v || (s.sel[j] == v && j < tid)) ? 1 : 0;
    s.idx[rank] = v;
  }
  for (int d = tid; d < D; d += kPeThreads) s.mu[d] = mu[d];
  __syncthreads();
  const bool ok = s.degenerate == 0;
  if (tid < P) s.xs[tid] = ok ? x[(int64_t)s.idx[tid] * x_stride] : 0.0;
  for (int e = tid; e < P * D; e += kPeThreads) {
    const int p = e / D, d = e - p * D;
    Yl[e] = ok ? Yrot[(int64_t)s.idx[p] * ld_y + d] : 0.0;
  }
  __syncthreads();
}

// The window handed over as data (the local-factor form): xs (P), Yrot_loc (P x D) and mu (D) of this window; a
// window that arrives flagged (carry != 0) is not fitted.
__device__ void pe_window_data(PeShared& s, double* Yl, const double* __restrict__ xs, const double* __restrict__ Yrot_loc,
                               const double* __restrict__ mu, int D, int P, int carry) {
  const int tid = threadIdx.x;
  if (tid == 0) s.degenerate = carry != 0 ? 1 : 0;
  if (tid < P) s.xs[tid] = xs[tid];
  for (int d = tid; d < D; d += kPeThreads) s.mu[d] = mu[d];
  for (int e = tid; e < P * D; e += kPeThreads) Yl[e] = Yrot_loc[e];
  __syncthreads();
}

// Box of the search into s.box; sets s.degenerate at span 0 (thread 0 works, everybody sees the result).
__device__ void pe_box(PeShared& s, int P, int D) {
  if (threadIdx.x == 0 && s.degenerate == 0) {
    for (int i = 0; i < P; ++i) {
      const double v = s.xs[i];
      int j = i;
      while (j > 0 && s.srt[j - 1] > v) {
        s.srt[j] = s.srt[j - 1];
        --j;
      }
      s.srt[j] = v;
    }
    const double span = s.srt[P - 1] - s.srt[0];
    double delta = INFINITY;
    for (int i = 1; i < P; ++i) {
      const double g = s.srt[i] - s.srt[i - 1];
      if (g > 0.0 && g < delta) delta = g;
    }
    double m = 0.0;
    for (int d = 0; d < D; ++d) m += s.mu[d];
    const double c = log(m / (double)D);
    if (!(span > 0.0)) {
      s.degenerate = 1;
    } else {
      s.box[0] = log(delta / 4.0);
      s.box[1] = log(16.0 * span);
      s.box[2] = c + kPeSLo;
      s.box[3] = c + kPeSHi;
    }
  }
  __syncthreads();
}

// lam, E and G0 = lam mu^T of the window at one length scale.
__device__ void pe_eval_ell(PeShared& s, const double* Yl, double* Eb, double* G0, double log_ell, int P, int D) {
  const int tid = threadIdx.x;
  const int np = P + (P & 1), half = np >> 1, m = np - 1;
  double ell = exp(log_ell);
  if (ell < 1e-8) ell = 1e-8;
  __syncthreads();
  if (tid < P) s.us[tid] = s.xs[tid] / ell;
  __syncthreads();
  for (int e = tid; e < np * np; e += kPeThreads) {
    const int i = e / np, j = e - i * np;
    double a = i == j ? 1.0 : 0.0;
    if (i < P && j < P) {
      const double d = s.us[i] - s.us[j];
      a = exp(__dmul_rn(__dmul_rn(-0.5, d), d));
    }
    s.A[i * kPeLd + j] = a;
    s.V[i * kPeLd + j] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  bool conv = false;
  for (int sw = 0; sw < kPeSweeps; ++sw) {
    if (tid == 0) s.rotated = 0;
    __syncthreads();
    for (int r = 0; r < m; ++r) {
      if (tid < half) {
        int p, q;
        if (tid == 0) {
          p = r;
          q = m;
        } else {
          p = (r + tid) % m;
          q = (r - tid + m) % m;
        }
        const double app = s.A[p * kPeLd + p], aqq = s.A[q * kPeLd + q], apq = s.A[p * kPeLd + q];
        double c = 1.0, sn = 0.0;
        const double thr = fmax(0x1p-52 * sqrt(fabs(app * aqq)), 0x1p-55);
        if (fabs(apq) > thr) {
          const double tau = (aqq - app) / (2.0 * apq);
          const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + tt * tt);
          sn = tt * c;
          s.rotated = 1;
        }
        s.rot[2 * tid] = c;
        s.rot[2 * tid + 1] = sn;
      }
      __syncthreads();
      for (int e = tid; e < half * np; e += kPeThreads) {       // rows p, q  <-  J^T A
        const int k = e / np, j = e - k * np;
        const double sn = s.rot[2 * k + 1];
        if (sn != 0.0) {
          const int p = k == 0 ? r : (r + k) % m, q = k == 0 ? m : (r - k + m) % m;
          const double c = s.rot[2 * k];
          const double ap = s.A[p * kPeLd + j], aq = s.A[q * kPeLd + j];
          s.A[p * kPeLd + j] = c * ap - sn * aq;
          s.A[q * kPeLd + j] = sn * ap + c * aq;
        }
      }
      __syncthreads();
      for (int e = tid; e < half * np; e += kPeThreads) {       // columns p, q  <-  A J, V J
        const int i = e / half, k = e - i * half;
        const double sn = s.rot[2 * k + 1];
        if (sn != 0.0) {
          const int p = k == 0 ? r : (r + k) % m, q = k == 0 ? m : (r - k + m) % m;
          const double c = s.rot[2 * k];
          const double ap = s.A[i * kPeLd + p], aq = s.A[i * kPeLd + q];
          // the annihilated pair is stored as an exact zero: left as the rounded residual, the two copies a_pq and
          // a_qp differ, the next sweep reads the other one, and a nearly rank-one K never stops rotating
          s.A[i * kPeLd + p] = i == q ? 0.0 : c * ap - sn * aq;
          s.A[i * kPeLd + q] = i == p ? 0.0 : sn * ap + c * aq;
          const double vp = s.V[i * kPeLd + p], vq = s.V[i * kPeLd + q];
          s.V[i * kPeLd + p] = c * vp - sn * vq;
          s.V[i * kPeLd + q] = sn * vp + c * vq;
        }
      }
      __syncthreads();
    }
    if (s.rotated == 0) {
      conv = true;
      break;
    }
    __syncthreads();
  }
  if (tid < P) s.lam[tid] = s.A[tid * kPeLd + tid];
  if (tid == 0 && !conv) s.jacobi_bad = 1;
  __syncthreads();
  for (int e = tid; e < P * D; e += kPeThreads) {
    const int p = e / D, d = e - p * D;
    double t = 0.0;
    for (int i = 0; i < P; ++i) t = fma(s.V[i * kPeLd + p], Yl[i * D + d], t);
    Eb[e] = t * t;
    G0[e] = __dmul_rn(s.lam[p], s.mu[d]);
  }
  __syncthreads();
}

// nll at log s = t for the current lam / E (every thread gets the same bits).
__device__ double pe_f(PeShared& s, const double* Eb, const double* G0, double t, int PD) {
  const double sv = exp(t);
  double acc = 0.0;
  for (int e = threadIdx.x; e < PD; e += kPeThreads) {
    const double G = G0[e] + sv;
    acc += log(G) + Eb[e] / G;
  }
  acc = block_sum(acc, s.red);
  return 0.5 * acc + 0.5 * (double)PD * kPeLog2Pi;
}

__device__ void pe_derivs(PeShared& s, const double* Eb, const double* G0, double t, int PD, double& g1, double& g2) {
  const double sv = exp(t);
  double v[2] = {0.0, 0.0};
  for (int e = threadIdx.x; e < PD; e += kPeThreads) {
    const double G = G0[e] + sv;
    const double r = sv / G, q = Eb[e] / G;
    v[0] += r - q * r;
    v[1] += r - r * r - q * r + 2.0 * q * r * r;
  }
  block_sum_n<double, 2>(v, s.red);
  g1 = 0.5 * v[0];
  g2 = 0.5 * v[1];
}

__device__ inline double pe_node(double lo, double hi, double h, int k, int last) { return k == last ? hi : lo + k * h; }

// min over log s in [lo, hi] at the current lam / E -> t, f.
__device__ void pe_profile(PeShared& s, const double* Eb, const double* G0, int PD, double lo, double hi, double& t_out,
                           double& f_out) {
  const double h = (hi - lo) / (double)(kPeSNodes - 1);
  int kb = 0;
  double fb = pe_f(s, Eb, G0, lo, PD);
  for (int k = 1; k < kPeSNodes; ++k) {
    const double fk = pe_f(s, Eb, G0, pe_node(lo, hi, h, k, kPeSNodes - 1), PD);
    if (fk < fb) {
      kb = k;
      fb = fk;
    }
  }
  double a = pe_node(lo, hi, h, max(kb - 1, 0), kPeSNodes - 1);
  double b = pe_node(lo, hi, h, min(kb + 1, kPeSNodes - 1), kPeSNodes - 1);
  const double tk = pe_node(lo, hi, h, kb, kPeSNodes - 1);
  double t = tk;
  for (int it = 0; it < kPeNewton; ++it) {
    double g1, g2;
    pe_derivs(s, Eb, G0, t, PD, g1, g2);
    if (g1 > 0.0) b = t;
    else a = t;
    double tn = g2 > 0.0 ? t - g1 / g2 : __builtin_nan("");
    if (!(tn > a && tn < b)) tn = 0.5 * (a + b);
    const double step = fabs(tn - t);
    t = tn;
    if (!(step > kPeNewtonStep)) break;
  }
  double ft = pe_f(s, Eb, G0, t, PD);
  if (!(ft < fb)) {
    t = tk;
    ft = fb;
  }
  t_out = t;
  f_out = ft;
}

__device__ inline void pe_prof_at(PeShared& s, const double* Yl, double* Eb, double* G0, double le, int P, int D,
                                  double& t, double& f) {
  pe_eval_ell(s, Yl, Eb, G0, le, P, D);
  pe_profile(s, Eb, G0, P * D, s.box[2], s.box[3], t, f);
}

// MODE 0: the search.  MODE 1: nll at the caller's n_eval (log s, log ell) pairs per window.  WIN: the windows come as
// data, x = xs (M, P), Yrot = Yrot_loc (M, P, D), mu (M, D); z, the strides and N are not read; win_flags (optional):
// a window with a non-zero entry is not fitted, its results are NaN and its flags that entry.
template <int MODE, bool WIN = false>
__global__ __launch_bounds__(kPeThreads) void preest_kernel(
    const double* __restrict__ x, int64_t x_stride, const double* __restrict__ Yrot, int64_t ld_y,
    const double* __restrict__ mu, const double* __restrict__ z, int64_t z_stride, int N, int D, int P,
    const double* __restrict__ pars, int n_eval, double* __restrict__ out_ell, double* __restrict__ out_s,
    double* __restrict__ out_nll, int* __restrict__ out_flags, int* __restrict__ out_nbr, double* __restrict__ out_box,
    const int* __restrict__ win_flags) {
  extern __shared__ __attribute__((aligned(16))) double pe_smem[];
  __shared__ PeShared s;
  double *Yl = pe_smem, *Eb = Yl + P * D, *G0 = Eb + P * D;
  const int tid = threadIdx.x, mwin = blockIdx.x, PD = P * D;
  const double nan = __builtin_nan("");
  if (tid == 0) s.jacobi_bad = 0;
  int bad_flag = kPeFlagDegenerate;
  if constexpr (WIN) {
    const int carry = win_flags ? win_flags[mwin] : 0;
    if (carry != 0) bad_flag = carry;
    pe_window_data(s, Yl, x + (int64_t)mwin * P, Yrot + (int64_t)mwin * PD, mu + (int64_t)mwin * D, D, P, carry);
  } else
    pe_window(s, Yl, x, x_stride, Yrot, ld_y, mu, z[(int64_t)mwin * z_stride], N, D, P);
  if (out_nbr && tid < P) out_nbr[(int64_t)mwin * P + tid] = s.idx[tid];

  if (MODE == 1) {
    const bool bad = s.degenerate != 0;
    for (int e = 0; e < n_eval; ++e) {
      const double ls = pars[((int64_t)mwin * n_eval + e) * 2], le = pars[((int64_t)mwin * n_eval + e) * 2 + 1];
      double f = nan;
      if (!bad) {
        pe_eval_ell(s, Yl, Eb, G0, le, P, D);
        f = pe_f(s, Eb, G0, ls, PD);
      }
      if (tid == 0) out_nll[(int64_t)mwin * n_eval + e] = f;
    }
    __syncthreads();
    if (tid == 0)
      out_flags[mwin] = (bad ? bad_flag : 0) | (s.jacobi_bad ? kPeFlagJacobi : 0);
    return;
  }

  pe_box(s, P, D);
  if (s.degenerate) {
    if (tid == 0) {
      out_ell[mwin] = nan;
      out_s[mwin] = nan;
      out_nll[mwin] = nan;
      out_flags[mwin] = bad_flag;
    }
    if (out_box && tid < 4) out_box[(int64_t)mwin * 4 + tid] = nan;
    return;
  }
  const double lo_e = s.box[0], hi_e = s.box[1];
  const double h = (hi_e - lo_e) / (double)(kPeEllNodes - 1);
  int jb = 0;
  double tb, fb;
  pe_prof_at(s, Yl, Eb, G0, lo_e, P, D, tb, fb);
  for (int j = 1; j < kPeEllNodes; ++j) {
    double tj, fj;
    pe_prof_at(s, Yl, Eb, G0, pe_node(lo_e, hi_e, h, j, kPeEllNodes - 1), P, D, tj, fj);
    if (fj < fb) {
      jb = j;
      tb = tj;
      fb = fj;
    }
  }
  double a = pe_node(lo_e, hi_e, h, max(jb - 1, 0), kPeEllNodes - 1);
  double b = pe_node(lo_e, hi_e, h, min(jb + 1, kPeEllNodes - 1), kPeEllNodes - 1);
  double c = b - kPeGoldenR * (b - a), d = a + kPeGoldenR * (b - a);
  double tc, fc, td, fd;
  pe_prof_at(s, Yl, Eb, G0, c, P, D, tc, fc);
  pe_prof_at(s, Yl, Eb, G0, d, P, D, td, fd);
  for (int it = 0; it < kPeGolden; ++it) {
    if (!(b - a > kPeGoldenWidth)) break;
    if (fc < fd) {
      b = d;
      d = c;
      td = tc;
      fd = fc;
      c = b - kPeGoldenR * (b - a);
      pe_prof_at(s, Yl, Eb, G0, c, P, D, tc, fc);
    } else {
      a = c;
      c = d;
      tc = td;
      fc = fd;
      d = a + kPeGoldenR * (b - a);
      pe_prof_at(s, Yl, Eb, G0, d, P, D, td, fd);
    }
  }
  double le = pe_node(lo_e, hi_e, h, jb, kPeEllNodes - 1), ls = tb, f = fb;
  if (fc < f) {
    le = c;
    ls = tc;
    f = fc;
  }
  if (fd < f) {
    le = d;
    ls = td;
    f = fd;
  }
  if (tid == 0) {
    out_ell[mwin] = le;
    out_s[mwin] = ls;
    out_nll[mwin] = f;
    out_flags[mwin] = (le == lo_e ? kPeFlagEllLo : 0) | (le == hi_e ? kPeFlagEllHi : 0) |
                      (ls == s.box[2] ? kPeFlagSLo : 0) | (ls == s.box[3] ? kPeFlagSHi : 0) |
                      (s.jacobi_bad ? kPeFlagJacobi : 0);
  }
  if (out_box && tid < 4) out_box[(int64_t)mwin * 4 + tid] = s.box[tid];
}

static bool pe_args_ok(const void* x, int64_t x_stride, const void* Yrot, int64_t ld_y, const void* mu, const void* z,
                       int64_t z_stride, int N, int D, int M, int P) {
  if (P < kPeMinP || P > kPeMaxP || D < 1 || D > kPeMaxD || N < P || M < 0) return false;
  if (!x || !Yrot || !mu || !z) return false;
  if (x_stride < 1 || z_stride < 1 || ld_y < D) return false;
  // element offsets of x, z, Yrot and the neighbour table stay below 2^31
  const int64_t lim = 0x7fffffffLL;
  if ((int64_t)(N - 1) * x_stride > lim || (int64_t)N * ld_y > lim || (int64_t)M * P > lim) return false;
  if (M > 0 && (int64_t)(M - 1) * z_stride > lim) return false;
  return true;
}

template <int MODE, bool WIN = false, class... Args>
static int pe_launch(int M, int P, int D, hipStream_t stream, Args... args) {
  allow_dynamic_lds<preest_kernel<MODE, WIN>>((size_t)3 * kPeMaxP * kPeMaxD * sizeof(double));
  const size_t smem = (size_t)3 * P * D * sizeof(double);
  hipLaunchKernelGGL((preest_kernel<MODE, WIN>), dim3((unsigned)M), dim3(kPeThreads), smem, stream, args...);
  NMGP_CHECK_LAUNCH();
  return NMGP_OK;
}

}  // namespace nmgp

using namespace nmgp;

extern "C" {

int nmgp_pre_estimate_f64(const double* x, int64_t x_stride, const double* Yrot, int64_t ld_y, const double* mu,
                          const double* z, int64_t z_stride, int N, int D, int M, int P, double* log_ell,
                          double* log_s, double* nll, int32_t* flags, int32_t* neighbours, double* box,
                          hipStream_t stream) {
  if (!pe_args_ok(x, x_stride, Yrot, ld_y, mu, z, z_stride, N, D, M, P)) return NMGP_ERR_PREEST_ARG;
  if (!log_ell || !log_s || !nll || !flags) return NMGP_ERR_PREEST_ARG;
  if (M == 0) return NMGP_OK;
  return pe_launch<0>(M, P, D, stream, x, x_stride, Yrot, ld_y, mu, z, z_stride, N, D, P, (const double*)nullptr, 0,
                      log_ell, log_s, nll, (int*)flags, (int*)neighbours, box, (const int*)nullptr);
}

int nmgp_pre_loglik_f64(const double* x, int64_t x_stride, const double* Yrot, int64_t ld_y, const double* mu,
                        const double* z, int64_t z_stride, int N, int D, int M, int P, const double* pars, int E,
                        double* nll, int32_t* flags, int32_t* neighbours, hipStream_t stream) {
  if (!pe_args_ok(x, x_stride, Yrot, ld_y, mu, z, z_stride, N, D, M, P)) return NMGP_ERR_PREEST_ARG;
  if (E < 0 || (int64_t)M * E > 0x3fffffffLL || !flags || (E > 0 && (!pars || !nll))) return NMGP_ERR_PREEST_ARG;
  if (M == 0) return NMGP_OK;
  return pe_launch<1>(M, P, D, stream, x, x_stride, Yrot, ld_y, mu, z, z_stride, N, D, P, pars, E,
                      (double*)nullptr, (double*)nullptr, nll, (int*)flags, (int*)neighbours, (double*)nullptr,
                      (const int*)nullptr);
}

static bool pe_windows_ok(const void* xs, const void* Yrot_loc, const void* mu, int M, int D, int P) {
  if (P < kPeMinP || P > kPeMaxP || D < 1 || D > kPeMaxD || M < 0) return false;
  if (!xs || !Yrot_loc || !mu) return false;
  return (int64_t)M * P * D <= 0x7fffffffLL;
}

int nmgp_pre_estimate_windows_f64(const double* xs, const double* Yrot_loc, const double* mu, int M, int D, int P,
                                  const int32_t* window_flags, double* log_ell, double* log_s, double* nll,
                                  int32_t* flags, double* box, hipStream_t stream) {
  if (!pe_windows_ok(xs, Yrot_loc, mu, M, D, P)) return NMGP_ERR_PREEST_ARG;
  if (!log_ell || !log_s || !nll || !flags) return NMGP_ERR_PREEST_ARG;
  if (M == 0) return NMGP_OK;
  return pe_launch<0, true>(M, P, D, stream, xs, (int64_t)1, Yrot_loc, (int64_t)D, mu, (const double*)nullptr,
                            (int64_t)1, P, D, P, (const double*)nullptr, 0, log_ell, log_s, nll, (int*)flags,
                            (int*)nullptr, box, (const int*)window_flags);
}

int nmgp_pre_loglik_windows_f64(const double* xs, const double* Yrot_loc, const double* mu, int M, int D, int P,
                                const int32_t* window_flags, const double* pars, int E, double* nll, int32_t* flags,
                                hipStream_t stream) {
  if (!pe_windows_ok(xs, Yrot_loc, mu, M, D, P)) return NMGP_ERR_PREEST_ARG;
  if (E < 0 || (int64_t)M * E > 0x3fffffffLL || !flags || (E > 0 && (!pars || !nll))) return NMGP_ERR_PREEST_ARG;
  if (M == 0) return NMGP_OK;
  return pe_launch<1, true>(M, P, D, stream, xs, (int64_t)1, Yrot_loc, (int64_t)D, mu, (const double*)nullptr,
                            (int64_t)1, P, D, P, pars, E, (double*)nullptr, (double*)nullptr, nll, (int*)flags,
                            (int*)nullptr, (double*)nullptr, (const int*)window_flags);
}

}  // extern "C"
