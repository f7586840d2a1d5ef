// lld_distinctive.h — the selection at the heart of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and
// MapLine::ComputeDistinctiveDescriptors (src/MapLine.cc:133-201) for the kernels that run it, once: from N descriptor rows to the first row
// with the strictly smallest median distance to the others.  lm_point_* / lm_line_wave (lld_landmark.hip: rows gathered in CSR form) and
// rf_point_* / rf_line_wave (lld_map_refresh.hip: rows fetched through the resident map's index rows) differ only in how the kept
// observers are compacted, where a row comes from, what an early return writes and where the winner goes; all of that stays with them.
// The LDS is the calling kernel's: it declares the arrays and passes them in, nothing here is __shared__.
// Device only.  The including file is compiled under `#pragma clang fp contract(off)`: every operation here is one IEEE operation.
#ifndef LLD_DISTINCTIVE_H
#define LLD_DISTINCTIVE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lld_wave.h"

namespace lld_dd {

constexpr int kWave = 64;
constexpr int kBlock = 256;                  // the workgroup form's block size

// vDists[0.5*(N-1)] of a row's sorted Hamming distances (:294) without the sort: the smallest v in [0, 256] with count(d <= v) > idx.
// count_le(v) is the lane's count over its N distances.
template <class CountLe>
__device__ __forceinline__ int sorted_at(int idx, CountLe count_le) {
  int lo = 0, hi = 256;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (count_le(mid) > idx) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// One wavefront, N <= 64 rows, lane i holds row i in (d0, d1) (lanes >= N: anything).  Row j reaches every lane by a lane broadcast; lane i
// keeps its distances in dist[j * 64 + i] (uint16, lane-contiguous, conflict free).  Returns, in every lane, median << 16 | row of the
// first row with the strictly smallest median: `median < BestMedian` in row order (:296-300).
__device__ __forceinline__ int point_wave(const uint4& d0, const uint4& d1, int N, int lane, uint16_t* dist) {
  for (int j = 0; j < N; ++j) {
    const uint4 b0 = make_uint4(lld_wave::bcast(d0.x, j), lld_wave::bcast(d0.y, j), lld_wave::bcast(d0.z, j), lld_wave::bcast(d0.w, j));
    const uint4 b1 = make_uint4(lld_wave::bcast(d1.x, j), lld_wave::bcast(d1.y, j), lld_wave::bcast(d1.z, j), lld_wave::bcast(d1.w, j));
    dist[j * kWave + lane] = (uint16_t)lld_wave::hamming256(d0, d1, b0, b1);
  }
  const int lo = sorted_at((int)(0.5 * (N - 1)), [&](int mid) {
    int cnt = 0;
    for (int j = 0; j < N; ++j) cnt += dist[j * kWave + lane] <= mid ? 1 : 0;
    return cnt;
  });
  return lld_wave::min(lane < N ? ((lo << 16) | lane) : 0x7fffffff);
}

// One workgroup of kBlock, N rows in LDS (rows[2 i], rows[2 i + 1]), written and a barrier passed before the call; every lane calls.  Rows are
// strided over the lanes and the distances recomputed from LDS (broadcast reads).  red holds kBlock / 64 ints.  One barrier inside.  Returns
// the same key as point_wave, in every lane.
__device__ __forceinline__ int point_block(const uint4* rows, int N, int tid, int* red) {
  const int idx = (int)(0.5 * (N - 1));
  int key = 0x7fffffff;
  for (int i = tid; i < N; i += kBlock) {    // ascending i per lane: the packed key keeps the first of equal medians
    const uint4 a0 = rows[2 * i], a1 = rows[2 * i + 1];
    const int lo = sorted_at(idx, [&](int mid) {
      int cnt = 0;
      for (int j = 0; j < N; ++j) cnt += lld_wave::hamming256(a0, a1, rows[2 * j], rows[2 * j + 1]) <= mid ? 1 : 0;
      return cnt;
    });
    const int k = (lo << 16) | i;
    key = k < key ? k : key;
  }
  key = lld_wave::min(key);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = key;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kBlock / kWave; ++q) key = red[q] < key ? red[q] : key;
  return key;
}

// One wavefront, N <= 64 rows of dim floats in LDS at rows[r * stride], written and a barrier passed before the call.  Lane i keeps
// (float)cv::norm(row i - row j) in dist[j * 64 + i], finds sorted[idx] by rank count and truncates it to int: `int median = vDists[...]`
// comes before the `<` test (:188).  Returns, in every lane, (median, row) of the first row with the strictly smallest median.
__device__ __forceinline__ int2 line(const float* rows, float* dist, int N, int dim, int stride, int lane) {
  const float* mine = rows + (lane < N ? lane : 0) * stride;
  for (int j = 0; j < N; ++j) {
    const float* other = rows + j * stride;
    double acc = 0.0;
    for (int k = 0; k < dim; ++k) { const float df = mine[k] - other[k]; acc = fma((double)df, (double)df, acc); }   // the product is exact in double
    dist[j * kWave + lane] = (float)__dsqrt_rn(acc);
  }
  const int idx = (int)(0.5 * (N - 1));
  float med = 0.f;                           // sorted[idx]: the value with rank_below <= idx < rank_below_or_equal
  for (int j = 0; j < N; ++j) {
    const float v = dist[j * kWave + lane];
    int lt = 0, le = 0;
    for (int k = 0; k < N; ++k) { const float u = dist[k * kWave + lane]; lt += u < v ? 1 : 0; le += u <= v ? 1 : 0; }
    if (lt <= idx && idx < le) med = v;
  }
  int m = lane < N ? (int)med : 0x7fffffff;
  int bi = lane;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int om = __shfl_xor(m, off), oi = __shfl_xor(bi, off);
    if (om < m || (om == m && oi < bi)) { m = om; bi = oi; }
  }
  return make_int2(m, bi);
}

}  // namespace lld_dd

#endif
