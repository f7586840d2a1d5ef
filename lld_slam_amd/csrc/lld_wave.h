// lld_wave.h — the cross-lane building blocks of the kernels, once: xor-butterfly reductions over a wavefront or an aligned sub-group, the
// fixed-order workgroup sum / maximum, the workgroup exclusive scan, the bitonic sort of 64-bit keys in LDS and the Hamming distance of two
// 256-bit descriptors.  Device-only, header-only, gfx950 (wavefronts of 64).  The order of the floating-point additions written at each
// function is part of its contract: `deterministic = 2` rests on it, and tests/test_gpu_wave_prims.py holds every function to
// a numpy model of exactly that order.
//
// Deliberately NOT here - different algorithms, not further copies of these:
//   hamming8 / bcnt_acc (lld_match.hip)       the inline-assembly accumulating popcount chain the brute-force matcher is tuned around
//   key_update (lld_match.hip)                the matcher's best/second key update
//   pair32_sum, the DPP pairings, wave_sum_all1, wave_sum28, block_sum1 (lld_pose.hip)   sums in the vector ALU with their own lane pairing
//                                             (xor 32, 16, 8, 7, 2, 1) and so their own addition order
//   the segmented __shfl_down sums (lld_ba_points.h, lld_ba_schur.h)                      runs of lanes of varying length, not aligned groups
//   the partial `xor 16, xor 32` column sums (lld_ba_solve.h, lld_ba_chol_sparse.h, lld_posegraph.hip pg dense solve)   two steps, not a full group
//   every (value, index) and best/second merge (lld_match.hip, lld_line_match.hip, lld_distinctive.h line, lld_bow_merge.h bow_match_node, the top-2 merge of
//                                             orb_search_kernel)   two coupled values per step
//   the ballot rankings and counts (lld_frame_finish.hip, lld_frame_lines.hip, lld_new_points.hip np_compact, lld_covisibility.hip,
//                                             lld_landmark.hip compact_kept, lld_orb_extract.hip, lld_ba_control.h)   order-preserving ranks from lane masks
//   wave_count and jacobi (lld_ransac.h)      already shared
//   the scan inside orb_search_kernel (lld_orb_search.hip)   same arithmetic as block_excl_scan without the leading barrier: the kernel is
//                                             held to unchanged machine code, and one more barrier would change it
#ifndef LLD_WAVE_H
#define LLD_WAVE_H

#include <hip/hip_runtime.h>

namespace lld_wave {

namespace detail {
// the lane's own value stays unless the other one is strictly smaller / greater (so it also stays against a NaN) ...
template <class T> __device__ __forceinline__ T lesser(T own, T other) { return other < own ? other : own; }
template <class T> __device__ __forceinline__ T greater(T own, T other) { return other > own ? other : own; }
// ... except for double, which keeps the fmax the optimisers were written with (a NaN loses on either side)
__device__ __forceinline__ double greater(double own, double other) { return fmax(own, other); }
}  // namespace detail

// ---------------------------------------------------------------------------------------------------------------- reductions
// W is a power of two <= 64; lanes form aligned groups of W.  Every lane of a group must be active (the whole wavefront for W = 64).  No
// LDS, no barrier.  Every lane returns its group's result.  Offsets run W/2, ..., 1: a lane adds, in this order, the partial sums of lane ^ W/2,
// ..., lane ^ 1 - the same tree in every lane, so all lanes of a group hold the same bits.

// sum of x over the group
template <int W = 64, class T>
__device__ __forceinline__ T sum(T x) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// sum() of several values through one butterfly, in place; each value gets exactly the additions of sum()
template <int W = 64, class... T>
__device__ __forceinline__ void sum_each(T&... x) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) ((x += __shfl_xor(x, o)), ...);
}

// minimum / maximum of x over the group (comparison rules: detail::lesser / greater)
template <int W = 64, class T>
__device__ __forceinline__ T min(T x) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) x = detail::lesser(x, (T)__shfl_xor(x, o));
  return x;
}
template <int W = 64, class T>
__device__ __forceinline__ T max(T x) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) x = detail::greater(x, (T)__shfl_xor(x, o));
  return x;
}

// x of lane l (0 <= l < W) of the caller's own aligned group of W lanes; l may differ from lane to lane.  The source lane must be active.
// For in-order sums over a sub-group: `for l: acc = acc + group_bcast<W>(x, l)` is the same sequence of additions in every lane of the group.
// (A move, no arithmetic: held by the packing test of tests/test_gpu_map_correct.py through mc_normal<8>.)
template <int W, class T>
__device__ __forceinline__ T group_bcast(T x, int l) { return __shfl(x, l, W); }

// v of lane l of the wavefront, l the same in every lane (it goes through a scalar register): a v_readlane, not a shuffle
__device__ __forceinline__ uint32_t bcast(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float bcastf(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// Sum of x over the workgroup (double or int); every lane returns it.  All blockDim.x lanes (a multiple of 64) call it; lds holds
// blockDim.x / 64 values.  Barriers: one before the wavefront totals are written (lds may still be read from an earlier call) and one after,
// none at the end.  Additions: sum<64>() inside each wavefront, then 0 + total[0] + total[1] + ... in ascending wavefront order.
template <class T>
__device__ __forceinline__ T block_sum(T x, T* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  x = sum(x);
  __syncthreads();
  if (lane == 0) lds[wave] = x;
  __syncthreads();
  T t = 0;
  for (int i = 0; i < nw; i++) t += lds[i];
  return t;
}

// max(0, maximum of x over the workgroup) - for magnitudes.  Lanes, lds and barriers as block_sum.
__device__ __forceinline__ double block_max(double x, double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  x = max(x);
  __syncthreads();
  if (lane == 0) lds[wave] = x;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < nw; i++) t = fmax(t, lds[i]);
  return t;
}

// ---------------------------------------------------------------------------------------------------------------- scan
// Exclusive prefix sum of v in thread order over a workgroup of exactly kThreads lanes (a multiple of 64), all calling; total = the sum, in
// every lane.  lds holds kThreads / 64 ints.  Barriers: one before the wavefront totals are written and one after, none at the end - so
// back-to-back calls may share lds, and no lane works alone.
template <int kThreads>
__device__ __forceinline__ int block_excl_scan(int v, int* lds, int& total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if (lane >= off) incl += t; }
  __syncthreads();                                             // (lds may still be read by the previous scan)
  if (lane == 63) lds[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll 4                                               // (all sixteen loads in flight cost bow_assemble 18 VGPRs and two waves per SIMD)
  for (int w = 0; w < kThreads / 64; w++) { const int t = lds[w]; if (w < wave) base += t; tot += t; }
  total = tot;
  return base + incl - v;
}

// ---------------------------------------------------------------------------------------------------------------- sort
// keys[0, npad) in LDS ascending; npad a power of two >= 2, the same in every lane (npad = 1: nothing to do, and no barrier).  A workgroup of exactly kThreads lanes, all calling, the
// keys written and a barrier passed before the call.  One barrier after each of the log2(npad) (log2(npad) + 1) / 2 steps, the last one
// included: the sorted keys may be read at once.  Each lane takes comparators, not elements (the half-index form), so none idles.
template <int kThreads>
__device__ __forceinline__ void bitonic_sort(unsigned long long* keys, int npad) {
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (npad >> 1); t += kThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const unsigned long long a = keys[lo], b = keys[hi];
        if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; }
      }
      __syncthreads();
    }
}

// The same network on (key, value) pairs: vals[i] travels with keys[i].  For keys that fill all 64 bits (a pointer, an id), where no value
// can be packed into the key.  Equal keys keep no particular order.  Lanes, npad and barriers as bitonic_sort.
template <int kThreads>
__device__ __forceinline__ void bitonic_sort_pairs(unsigned long long* keys, int* vals, int npad) {
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (npad >> 1); t += kThreads) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const unsigned long long a = keys[lo], b = keys[hi];
        if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; const int v = vals[lo]; vals[lo] = vals[hi]; vals[hi] = v; }
      }
      __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- Hamming distance
// DescriptorDistance of two 256-bit descriptors: plain popcounts of the eight word pairs, summed from the first word.  Any lane, no LDS.

// descriptor a = (a0, a1) against b = (b0, b1)
__device__ __forceinline__ int hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}
// a as eight words in registers
__device__ __forceinline__ int hamming256(const uint32_t (&a)[8], const uint4& b0, const uint4& b1) {
  return __popc(a[0] ^ b0.x) + __popc(a[1] ^ b0.y) + __popc(a[2] ^ b0.z) + __popc(a[3] ^ b0.w) +
         __popc(a[4] ^ b1.x) + __popc(a[5] ^ b1.y) + __popc(a[6] ^ b1.z) + __popc(a[7] ^ b1.w);
}
// ... against a descriptor in memory: b is 16-byte aligned and read as two uint4
__device__ __forceinline__ int hamming256(const uint32_t (&a)[8], const uint4* b) {
  const uint4 b0 = b[0], b1 = b[1];
  return hamming256(a, b0, b1);
}
// ... against eight words of which only 4-byte alignment is known
__device__ __forceinline__ int hamming256(const uint32_t (&a)[8], const uint32_t* b) {
  int d = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) d += __popc(a[w] ^ b[w]);
  return d;
}

}  // namespace lld_wave

#endif
