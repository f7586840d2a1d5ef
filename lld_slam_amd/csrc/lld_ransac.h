// lld_ransac.h — device pieces shared by the RANSAC solvers (lld_pnp.hip, lld_sim3solver.hip, lld_initializer.hip): the rand()
// stream and minimal-set draw of lld_ransac_stream.h, the cyclic Jacobi eigensolver, the canonical eigenvector sign, and the
// parts of a batch's count and resolve kernels that do not depend on the model.
// Everything is in an anonymous namespace (one copy per including file) and compiled without FMA contraction.
#ifndef LLD_RANSAC_H
#define LLD_RANSAC_H

#include <cstdint>

#include <hip/hip_runtime.h>

#include "lld_ransac_stream.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSweeps = 40;                  // most cyclic Jacobi sweeps
constexpr double kJacTol = 1e-36;            // stop: sum of squared off-diagonals <= kJacTol * sum of squared diagonals

// ------------------------------------------------------------------ strided scratch (LDS, lane-interleaved or not)
struct SP {
  double* p; int s;
  __device__ double& operator[](int i) const { return p[i * s]; }
  __device__ SP at(int o) const { return SP{p + o * s, s}; }
};

// Cyclic Jacobi on a symmetric n x n (row-major in A): eigenvalues on A's diagonal, eigenvectors in V's columns.
__device__ void jacobi(SP A, SP V, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
  for (int sw = 0; sw < kSweeps; ++sw) {
    double off = 0.0, dg = 0.0;
    for (int p = 0; p < n; ++p) {
      dg += A[p * n + p] * A[p * n + p];
      for (int q = p + 1; q < n; ++q) off += A[p * n + q] * A[p * n + q];
    }
    if (off <= kJacTol * dg) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        double apq = A[p * n + q];
        if (apq == 0.0) continue;
        double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
        }
        A[p * n + q] = 0.0;
        A[q * n + p] = 0.0;
        for (int k = 0; k < n; ++k) {
          double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
}

// Column `col` of V (n x n) into dst, its first largest-magnitude component made positive.
__device__ void canonical_col(SP V, int n, int col, SP dst) {
  int m = 0;
  for (int k = 1; k < n; ++k)
    if (fabs(V[k * n + col]) > fabs(V[m * n + col])) m = k;
  bool neg = V[m * n + col] < 0.0;
  for (int k = 0; k < n; ++k) dst[k] = neg ? -V[k * n + col] : V[k * n + col];
}

// ------------------------------------------------------------------ a batch of solvers: hypothesis slots, counts, flags
// The solver that owns hypothesis slot g of a call: off[n + 1] are the slot bounds, off[s] <= g < off[s + 1].
__device__ inline int solver_of(const int32_t* off, int n, int g) {
  int lo = 0, hi = n;                        // off[lo] <= g < off[hi]
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// One wavefront: how many i < n satisfy pred(i), by ballot / popcount (the same count on every lane).
template <class F>
__device__ inline int wave_count(int n, F pred) {
  const int lane = threadIdx.x & 63;
  int cnt = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool in = i < n && pred(i);
    cnt += __popcll(__ballot(in));
  }
  return cnt;
}

// The tail of a resolve workgroup of T lanes: vbInliers cleared, then, when a pose is returned, set at index[i] of every inlier.
template <int T, class F>
__device__ inline void scatter_inliers(uint8_t* flags, int n_flags, bool has_pose, const int32_t* index, int n, F pred) {
  for (int i = threadIdx.x; i < n_flags; i += T) flags[i] = 0;
  __syncthreads();
  if (!has_pose) return;
  for (int i = threadIdx.x; i < n; i += T)
    if (pred(i)) flags[index[i]] = 1;
}

}  // namespace

#endif
