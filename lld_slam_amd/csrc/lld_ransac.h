// lld_ransac.h — device pieces shared by the RANSAC solvers (lld_pnp.hip, lld_sim3solver.hip, lld_initializer.hip): one glibc rand() stream per
// solver (DEVIATION 1 of both sections of include/lld_amd.h), the cyclic Jacobi eigensolver and the canonical eigenvector sign.
// Everything is in an anonymous namespace (one copy per including file) and compiled without FMA contraction.
#ifndef LLD_RANSAC_H
#define LLD_RANSAC_H

#include <cstdint>

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace {

constexpr int kSweeps = 40;                  // most cyclic Jacobi sweeps
constexpr double kJacTol = 1e-36;            // stop: sum of squared off-diagonals <= kJacTol * sum of squared diagonals

// ------------------------------------------------------------------ glibc rand() on a lane
__device__ __host__ inline uint32_t rng_next(uint32_t* ring, int32_t& head) {
  int h = head;
  int h3 = h + 28; if (h3 >= 31) h3 -= 31;
  uint32_t x = ring[h] + ring[h3];
  ring[h] = x;
  head = h + 1 == 31 ? 0 : h + 1;
  return x;
}

// RandomInt(0, d - 1) (Thirdparty/DBoW2/DUtils/Random.cpp:47-50): int((double)rand() / (RAND_MAX + 1.0) * d)
__device__ __host__ inline int random_int(uint32_t* ring, int32_t& head, int d) {
  uint32_t r = rng_next(ring, head) >> 1;
  return int(((double)r / ((double)2147483647 + 1.0)) * (double)d);
}

static void srand_state(uint32_t seed, uint32_t* ring, int32_t* head) {
  if (seed == 0) seed = 1;
  int32_t r[34];
  int32_t word = (int32_t)seed;
  r[0] = word;
  for (int i = 1; i < 31; ++i) {
    int32_t hi = word / 127773, lo = word % 127773;
    word = 16807 * lo - 2836 * hi;
    if (word < 0) word += 2147483647;
    r[i] = word;
  }
  for (int i = 31; i < 34; ++i) r[i] = r[i - 31];
  for (int i = 0; i < 31; ++i) ring[i] = (uint32_t)r[3 + i];
  *head = 0;
  for (int i = 0; i < 310; ++i) rng_next(ring, *head);
}

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

}  // namespace

#endif
