// lld_ransac_stream.h — the parts of a RANSAC solver that define its bit-exact deviation "one glibc rand() stream per solver"
// (DEVIATION 1 of the PnP, Sim3 and Initializer sections of include/lld_amd.h): the stream, its save / rewind around a call's
// window, the minimal-set draw and the iteration budget.  No HIP header is needed: the file compiles under a plain C++17 host
// compiler as well (tests/test_ransac_stream.py does that), and under hipcc the same functions run on a lane.
#ifndef LLD_RANSAC_STREAM_H
#define LLD_RANSAC_STREAM_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define LLD_STREAM_FN __host__ __device__ inline
#else
#define LLD_STREAM_FN inline
#endif
#ifdef __clang__
#pragma clang fp contract(off)
#define LLD_UNROLL _Pragma("unroll")
#else
#define LLD_UNROLL _Pragma("GCC unroll 8")
#endif

namespace {

// ------------------------------------------------------------------ glibc rand() on a lane
LLD_STREAM_FN uint32_t rng_next(uint32_t* ring, int32_t& head) {
  int h = head;
  int h3 = h + 28; if (h3 >= 31) h3 -= 31;
  uint32_t x = ring[h] + ring[h3];
  ring[h] = x;
  head = h + 1 == 31 ? 0 : h + 1;
  return x;
}

// RandomInt(0, d - 1) (Thirdparty/DBoW2/DUtils/Random.cpp:47-50): int((double)rand() / (RAND_MAX + 1.0) * d)
LLD_STREAM_FN int random_int(uint32_t* ring, int32_t& head, int d) {
  uint32_t r = rng_next(ring, head) >> 1;
  return int(((double)r / ((double)2147483647 + 1.0)) * (double)d);
}

LLD_STREAM_FN void srand_state(uint32_t seed, uint32_t* ring, int32_t* head) {
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

// The stream of one solver whose state stays on the device.  A call draws its whole window ahead of knowing how many of the
// hypotheses iterate() would have made, so the sample kernel saves the stream first and the resolve kernel sets it to the saved
// one advanced by the draws actually made.
struct RansacStream {
  uint32_t ring[31]; int32_t head;           // r[i-31 .. i-1] of glibc's TYPE_3 table, ring[head] = r[i-31]
  uint32_t ring0[31]; int32_t head0;         // the stream at the start of the call's window

  LLD_STREAM_FN void save() {
    for (int i = 0; i < 31; ++i) ring0[i] = ring[i];
    head0 = head;
  }
  // The saved stream + `draws` draws.  Always inlined: optimised on its own first, its copies become one from a generic pointer
  // and r[] lands in scratch in the resolve kernels instead of registers.
  __attribute__((always_inline)) LLD_STREAM_FN void rewind(int draws) {
    uint32_t r[31];
    int32_t h = head0;
    for (int i = 0; i < 31; ++i) r[i] = ring0[i];
    for (int i = 0; i < draws; ++i) rng_next(r, h);
    for (int i = 0; i < 31; ++i) ring[i] = r[i];
    head = h;
  }
};

// One minimal set of K out of N (K <= N): vAvailableIndices = mvAllIndices, then K x (RandomInt over the remaining, take, swap
// the back into its place, pop).  The positions overwritten so far are kept in (pos, val) pairs instead of a copy of the index list.
template <int K>
LLD_STREAM_FN void draw_set(uint32_t* ring, int32_t& head, int N, int32_t* out) {
  int pos[K], val[K];
  LLD_UNROLL
  for (int i = 0; i < K; ++i) {
    const int size = N - i;
    const int r = random_int(ring, head, size);
    int v = r, back = size - 1;
    LLD_UNROLL
    for (int j = 0; j < i; ++j) {            // oldest first: the newest write of a position wins
      if (pos[j] == r) v = val[j];
      if (pos[j] == size - 1) back = val[j];
    }
    out[i] = v;
    pos[i] = r; val[i] = back;               // vAvailableIndices[randi] = back(); pop_back()
  }
}

// mRansacMaxIts of SetRansacParameters (PnPsolver.cc:121-157, Sim3Solver.cc:114-138) from the solver's own minimum inlier count
// and epsilon.  N < min_inliers gives epsilon > 1 (N = 0: inf) and a NaN quotient; the reference's (int) of it is INT_MIN on
// x86-64 (budget 1), written out here instead of left to an undefined conversion.  iterate() never draws for such a solver.
inline int ransac_max_iterations(double probability, float epsilon, int min_inliers, int N, int max_iterations) {
  int its = 1;
  if (min_inliers != N) {
    const double q = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
    its = std::isfinite(q) && q < 2147483647.0 ? (int)q : INT_MIN;
  }
  return std::max(1, std::min(its, max_iterations));
}

}  // namespace

#endif
