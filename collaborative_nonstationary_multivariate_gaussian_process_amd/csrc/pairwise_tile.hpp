// One 8-row x 64-column tile of the forward pairwise builders (pairwise.hip explains them): the body of
// pairwise_kernel, shared with the step-head kernel (head.hip), which runs a descriptor group's tiles in some of its
// workgroups: one definition, so every caller rounds alike.
#pragma once
#include "common.hpp"

namespace nmgp {

// 8-row x 64-column tiles, two rows per wave (round 6: 32-row tiles left the M x M priors' K22 (256 x 256) at 96
// workgroups and the K_G12 backward (2000 x 256) at 252, each wave working through 8 rows in turn; include/nmgp_hip.h
// pairwise descriptors' `tiles`, the backward's partial sums are per 8-row tile)
constexpr int PR = 8, PC = 64;
constexpr int PRF = PR;

struct PwArgs {
  const nmgp_pairwise_desc* descs;
  int nd;
  nmgp_pairwise_desc inl;
};

template <typename D>
__device__ inline const D* find_desc(const D* descs, int nd, const D* inl, int tile) {
  if (descs == nullptr) return inl;
  int lo = 0, hi = nd - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].tile_start <= tile) lo = mid; else hi = mid - 1;
  }
  return &descs[lo];
}

template <typename T>
__device__ inline T sqdist(const T* X, const T* Z, int i, int j, int p, int dist, T inv_ls) {
  if (dist == NMGP_DIST_DIFF) {
    T r2 = 0;
    for (int f = 0; f < p; ++f) {
      const T dd = X[(int64_t)i * p + f] * inv_ls - Z[(int64_t)j * p + f] * inv_ls;
      r2 += dd * dd;
    }
    return r2;
  }
  T xn = 0, zn = 0, xz = 0;
  for (int f = 0; f < p; ++f) {
    const T a = X[(int64_t)i * p + f] * inv_ls, b = Z[(int64_t)j * p + f] * inv_ls;
    xn += a * a;
    zn += b * b;
    xz += a * b;
  }
  return xn + zn - (T)2 * xz;
}

// Division (not multiply-by-reciprocal) keeps the forward bit-closer to the reference's x / ls.
template <typename T>
__device__ inline T sqdist_div(const T* X, const T* Z, int i, int j, int p, int dist, T ls) {
  if (dist == NMGP_DIST_DIFF) {
    T r2 = 0;
    for (int f = 0; f < p; ++f) {
      const T dd = X[(int64_t)i * p + f] / ls - Z[(int64_t)j * p + f] / ls;
      r2 += dd * dd;
    }
    return r2;
  }
  T xn = 0, zn = 0, xz = 0;
  for (int f = 0; f < p; ++f) {
    const T a = X[(int64_t)i * p + f] / ls, b = Z[(int64_t)j * p + f] / ls;
    xn += a * a;
    zn += b * b;
    xz += a * b;
  }
  return xn + zn - (T)2 * xz;
}

template <typename T>
__device__ inline void hyper_of(const T* hyp, int mode, int flags, T& s2, T& ls) {
  if (hyp == nullptr) return;
  s2 = hyp[0];
  if (flags & NMGP_HYP_LOG) s2 = dexp(s2);
  if (mode == NMGP_RBF) {
    ls = hyp[1];
    if (flags & NMGP_HYP_LOG) ls = dexp(ls);
  }
}

// tile `tile` of the group, by 256 threads: t is the thread's index among them
template <typename T>
__device__ inline void pairwise_tile(const PwArgs& args, int tile, int t) {
  const nmgp_pairwise_desc& d = *find_desc(args.descs, args.nd, &args.inl, tile);
  tile -= d.tile_start;
  const int n = d.n, m = d.m, p = d.p;
  const int ctn = (m + PC - 1) / PC;
  const int rt = tile / ctn, ct = tile - rt * ctn;
  const int j = ct * PC + (t & 63);
  if (j >= m) return;
  constexpr int PR = PRF;
  T s2 = (T)d.scale2, ls = (T)d.length_scale;
  hyper_of((const T*)d.hyp, d.mode, d.flags, s2, ls);
  const T* X = (const T*)d.X;
  const T* Z = (const T*)d.Z;
  const T* ellX = (const T*)d.ellX;
  const T* ellZ = (const T*)d.ellZ;
  const T* sigX = (const T*)d.sigX;
  const T* sigZ = (const T*)d.sigZ;
  T* K = (T*)d.K;
  const T dadd = (T)d.diag_add;
  const T lz = d.mode == NMGP_GIBBS ? ellZ[j] : (T)0;
  const T sz = sigZ ? sigZ[j] : (T)1;
#pragma unroll 2
  for (int e = 0; e < PR / 4; ++e) {
    const int i = rt * PR + (t >> 6) + 4 * e;
    if (i >= n) break;
    T k;
    if (d.mode == NMGP_RBF) {
      const T r2 = sqdist_div(X, Z, i, j, p, d.dist, ls);
      k = dexp((T)-0.5 * r2) * s2;
    } else {
      const T r2 = sqdist_div(X, Z, i, j, p, d.dist, (T)1);
      const T lx = ellX[i];
      const T S = lx * lx + lz * lz;
      const T C = dsqrt((T)2 * (lx * lz) / S);
      k = sigX ? ((sigX[i] * sz) * C) * dexp(-r2 / S) : s2 * C * dexp(-r2 / S);
    }
    if (i == j) k += dadd;
    K[(int64_t)i * d.ldk + j] = k;
  }
}

}  // namespace nmgp
