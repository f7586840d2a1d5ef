// lld_landmark.hip — the two per-landmark routines every thread of the reference runs between its searches and optimisations:
// MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (src/MapPoint.cc:242-307, :330-371) and
// MapLine::ComputeDistinctiveDescriptors (src/MapLine.cc:133-201), for a whole batch of landmarks in one call.  The rules restated
// and the deviations are written out in include/lld_amd.h; tests/landmark_ref.py restates them independently in numpy.
//
// The whole file is compiled without FMA contraction: every float operation is the one IEEE operation the restatement performs.
//
// Kernels (one call = one upload, the kernels its flags select, one download; no atomics, no scratch):
//   lm_point_wave   one wavefront (a workgroup of 64) per MapPoint with at most 64 kept observations.  The kept observations are
//                   compacted in list order by ballot; lane i holds descriptor i in 8 registers; row j reaches every lane by a lane
//                   broadcast; lane i keeps its row of distances in LDS (uint16, lane-contiguous, conflict free) and finds
//                   sorted[idx] by bisection on the value: the smallest v in [0, 256] with count(d <= v) > idx.  A wavefront min
//                   on (median << 16 | i) is the first row with the strictly smallest median.
//   lm_point_block  one workgroup of 256 per MapPoint with 65 .. LLD_LANDMARK_MAX_OBS kept observations: descriptors in LDS, rows
//                   strided over the lanes, the same bisection with the distances recomputed from LDS (broadcast reads).
//   lm_normal_wave  one wavefront per MapPoint: 64 terms (pos - Ow_i)/|pos - Ow_i| formed at once, then every lane adds them in
//                   observation order through lane broadcasts, so the float sum has the reference's order.  The term, the centre it
//                   reads and the final write are lld_normal_depth.h's, shared with the whole-map kernels of lld_map_correct.hip.
//   lm_line_wave    one wavefront per MapLine: rows in LDS (odd stride), float distances in LDS, sorted[idx] by rank count, the
//                   truncation to int, a wavefront min on (median, i).
// Every landmark is handled by one workgroup that reads nothing another workgroup writes: the result cannot depend on the batch.
#pragma clang fp contract(off)

#include <cmath>
#include <vector>

#include "lld_common.h"
#include "lld_normal_depth.h"
#include "lld_wave.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;

struct PointArgs {
  const int32_t* obs_start; const int32_t* obs_kf; const uint32_t* obs_desc; const uint8_t* kf_bad; const uint8_t* bad;
  const int32_t* list;                       // the MapPoints of this launch
  uint32_t* desc; int32_t* best_obs; int32_t* best_median; uint8_t* upd;
};

struct NormalArgs {
  const int32_t* obs_start; const int32_t* obs_kf; const float* kf_ow; const float* pos; const uint8_t* bad;
  const int32_t* ref_kf; const int32_t* ref_level; const float* level_scale; int32_t n_levels;
  float* normal; float* min_distance; float* max_distance; uint8_t* upd;
};

struct LineArgs {
  const int32_t* obs_start; const int32_t* obs_kf; const float* obs_desc; const uint8_t* kf_bad; const uint8_t* bad; int32_t dim;
  float* desc; int32_t* best_obs; int32_t* best_median; uint8_t* upd;
};

__device__ __forceinline__ uint32_t bcast(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ float bcastf(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// The observations of [s, e) whose keyframe is not bad, in list order: kept[r] = position in the landmark's own list.  Called by
// one whole wavefront; returns the count (the same in every lane).  Positions past `cap` are counted but not stored.
__device__ __forceinline__ int compact_kept(const int32_t* __restrict__ obs_kf, const uint8_t* __restrict__ kf_bad, int s, int e, int lane,
                                            int* kept, int cap) {
  int n = 0;
  for (int c = s; c < e; c += kWave) {
    const int o = c + lane;
    const bool keep = o < e && kf_bad[obs_kf[o]] == 0;
    const unsigned long long m = __ballot(keep);
    if (keep) {
      const int r = n + __popcll(m & ((1ull << lane) - 1ull));
      if (r < cap) kept[r] = o - s;
    }
    n += __popcll(m);
  }
  return n;
}

// grid: the list, block 64
__global__ __launch_bounds__(kWave) void lm_point_wave(PointArgs A) {
  __shared__ int kept[kWave];
  __shared__ uint16_t dist[kWave * kWave];   // dist[j * 64 + i] = DescriptorDistance(row i, row j)
  const int lane = threadIdx.x;
  const int p = A.list[blockIdx.x];
  const int s = A.obs_start[p], e = A.obs_start[p + 1];
  int N = 0;
  if (!A.bad[p]) N = compact_kept(A.obs_kf, A.kf_bad, s, e, lane, kept, kWave);
  N = N < kWave ? N : kWave;                 // the host sends only MapPoints with at most 64 kept observations here
  __syncthreads();
  if (N == 0) {                              // mbBad, observations.empty() or vDescriptors.empty(): return (:251-252, :256-257, :269-270)
    if (lane == 0) { A.best_obs[p] = -1; A.best_median[p] = -1; A.upd[p] = 0; }
    return;
  }
  uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
  if (lane < N) {
    const uint4* src = reinterpret_cast<const uint4*>(A.obs_desc + (size_t)(s + kept[lane]) * 8);
    d0 = src[0]; d1 = src[1];
  }
  for (int j = 0; j < N; ++j) {
    const uint4 b0 = make_uint4(bcast(d0.x, j), bcast(d0.y, j), bcast(d0.z, j), bcast(d0.w, j));
    const uint4 b1 = make_uint4(bcast(d1.x, j), bcast(d1.y, j), bcast(d1.z, j), bcast(d1.w, j));
    dist[j * kWave + lane] = (uint16_t)lld_wave::hamming256(d0, d1, b0, b1);
  }
  const int idx = (int)(0.5 * (N - 1));      // vDists[0.5*(N-1)] (:294)
  int lo = 0, hi = 256;                      // sorted[idx] = the smallest v with count(d <= v) >= idx + 1
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    int cnt = 0;
    for (int j = 0; j < N; ++j) cnt += dist[j * kWave + lane] <= mid ? 1 : 0;
    if (cnt > idx) hi = mid; else lo = mid + 1;
  }
  const int key = lld_wave::min(lane < N ? ((lo << 16) | lane) : 0x7fffffff);   // median < BestMedian in row order (:296-300)
  const int w = kept[key & 0xffff];
  if (lane < 8) A.desc[(size_t)p * 8 + lane] = A.obs_desc[(size_t)(s + w) * 8 + lane];
  if (lane == 0) { A.best_obs[p] = w; A.best_median[p] = key >> 16; A.upd[p] = 1; }
}

// grid: the list, block 256
__global__ __launch_bounds__(kBlock) void lm_point_block(PointArgs A) {
  __shared__ int kept[LLD_LANDMARK_MAX_OBS];
  __shared__ uint4 rows[LLD_LANDMARK_MAX_OBS * 2];
  __shared__ int red[kBlock / kWave];
  __shared__ int sN;
  const int tid = threadIdx.x;
  const int p = A.list[blockIdx.x];
  const int s = A.obs_start[p], e = A.obs_start[p + 1];
  if (tid < kWave) {
    int n = 0;
    if (!A.bad[p]) n = compact_kept(A.obs_kf, A.kf_bad, s, e, tid, kept, LLD_LANDMARK_MAX_OBS);
    if (tid == 0) sN = n < LLD_LANDMARK_MAX_OBS ? n : LLD_LANDMARK_MAX_OBS;
  }
  __syncthreads();
  const int N = sN;
  if (N == 0) {
    if (tid == 0) { A.best_obs[p] = -1; A.best_median[p] = -1; A.upd[p] = 0; }
    return;
  }
  for (int q = tid; q < 2 * N; q += kBlock)
    rows[q] = reinterpret_cast<const uint4*>(A.obs_desc + (size_t)(s + kept[q >> 1]) * 8)[q & 1];
  __syncthreads();
  const int idx = (int)(0.5 * (N - 1));
  int key = 0x7fffffff;
  for (int i = tid; i < N; i += kBlock) {    // ascending i per lane: the packed key keeps the first of equal medians
    const uint4 a0 = rows[2 * i], a1 = rows[2 * i + 1];
    int lo = 0, hi = 256;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      int cnt = 0;
      for (int j = 0; j < N; ++j) cnt += lld_wave::hamming256(a0, a1, rows[2 * j], rows[2 * j + 1]) <= mid ? 1 : 0;
      if (cnt > idx) hi = mid; else lo = mid + 1;
    }
    const int k = (lo << 16) | i;
    key = k < key ? k : key;
  }
  key = lld_wave::min(key);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = key;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < kBlock / kWave; ++q) key = red[q] < key ? red[q] : key;
  const int w = kept[key & 0xffff];
  if (tid < 8) A.desc[(size_t)p * 8 + tid] = A.obs_desc[(size_t)(s + w) * 8 + tid];
  if (tid == 0) { A.best_obs[p] = w; A.best_median[p] = key >> 16; A.upd[p] = 1; }
}

// grid: n_points, block 64
__global__ __launch_bounds__(kWave) void lm_normal_wave(NormalArgs A) {
  const int lane = threadIdx.x;
  const int p = blockIdx.x;
  const int s = A.obs_start[p], e = A.obs_start[p + 1];
  if (A.bad[p] || e == s) {                  // mbBad or observations.empty(): return (:338-339, :345-346); bad keyframes are NOT skipped
    if (lane == 0) A.upd[p] = 0;
    return;
  }
  const float px = A.pos[3 * (size_t)p], py = A.pos[3 * (size_t)p + 1], pz = A.pos[3 * (size_t)p + 2];
  const lld_nd::Centres C{A.kf_ow, A.kf_ow, nullptr};
  float nx = 0.f, ny = 0.f, nz = 0.f;
  for (int c = s; c < e; c += kWave) {
    const int o = c + lane;
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (o < e) lld_nd::term(px, py, pz, lld_nd::centre(C, A.obs_kf[o], 0), tx, ty, tz);
    const int cnt = e - c < kWave ? e - c : kWave;
    for (int l = 0; l < cnt; ++l) {          // normal = normal + ... in observation order, the same sum in every lane
      nx = nx + bcastf(tx, l); ny = ny + bcastf(ty, l); nz = nz + bcastf(tz, l);
    }
  }
  if (lane == 0) {
    lld_nd::finish(lld_nd::Out{A.normal, A.min_distance, A.max_distance}, p, px, py, pz, nx, ny, nz, e - s,
                   lld_nd::centre(C, A.ref_kf[p], 0), A.level_scale, A.ref_level[p], A.n_levels);
    A.upd[p] = 2;
  }
}

// grid: n_lines, block 64; dynamic LDS: 64 * (dim | 1) floats of rows, then 64 * 64 floats of distances
__global__ __launch_bounds__(kWave) void lm_line_wave(LineArgs A) {
  extern __shared__ float smem[];
  __shared__ int kept[kWave];
  const int dim = A.dim, stride = A.dim | 1;
  float* rows = smem;
  float* dist = smem + kWave * stride;       // dist[j * 64 + i] = (float)cv::norm(row i - row j)
  const int lane = threadIdx.x;
  const int p = blockIdx.x;
  const int s = A.obs_start[p], e = A.obs_start[p + 1];
  int N = 0;
  if (!A.bad[p]) N = compact_kept(A.obs_kf, A.kf_bad, s, e, lane, kept, kWave);
  N = N < kWave ? N : kWave;                 // the host refuses a longer list
  __syncthreads();
  if (N == 0) {
    if (lane == 0) { A.best_obs[p] = -1; A.best_median[p] = -1; A.upd[p] = 0; }
    return;
  }
  for (int r = 0; r < N; ++r) {
    const float* src = A.obs_desc + (size_t)(s + kept[r]) * dim;
    for (int k = lane; k < dim; k += kWave) rows[r * stride + k] = src[k];
  }
  __syncthreads();
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
  int m = lane < N ? (int)med : 0x7fffffff;   // int median = vDists[...]: the float is truncated before the `<` test (:188)
  int bi = lane;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int om = __shfl_xor(m, off), oi = __shfl_xor(bi, off);
    if (om < m || (om == m && oi < bi)) { m = om; bi = oi; }
  }
  for (int k = lane; k < dim; k += kWave) A.desc[(size_t)p * dim + k] = rows[bi * stride + k];
  if (lane == 0) { A.best_obs[p] = kept[bi]; A.best_median[p] = m; A.upd[p] = 1; }
}

inline size_t al(size_t b) { return (b + 255) & ~size_t(255); }

// CSR checks shared by both entry points: INVALID for a malformed list, UNSUPPORTED above `max_obs` per landmark.
int check_csr(int32_t n, int32_t n_obs, int32_t n_kf, const int32_t* obs_start, const int32_t* obs_kf, int max_obs) {
  if (obs_start[0] != 0 || obs_start[n] != n_obs) return LLD_ERR_INVALID;
  for (int i = 0; i < n; ++i) if (obs_start[i + 1] < obs_start[i]) return LLD_ERR_INVALID;
  for (int o = 0; o < n_obs; ++o) if (obs_kf[o] < 0 || obs_kf[o] >= n_kf) return LLD_ERR_INVALID;
  for (int i = 0; i < n; ++i) if (obs_start[i + 1] - obs_start[i] > max_obs) return LLD_ERR_UNSUPPORTED;
  return LLD_OK;
}

}  // namespace

extern "C" {

int lld_mappoint_refresh(lld_ctx* ctx, const lld_mappoint_refresh_in* in, lld_mappoint_refresh_out* out) {
  if (!ctx || !in || !out) return LLD_ERR_INVALID;
  const int32_t n = in->n_points, n_obs = in->n_obs, n_kf = in->n_kf;
  const bool want_desc = (in->flags & LLD_LANDMARK_DESCRIPTOR) != 0, want_norm = (in->flags & LLD_LANDMARK_NORMAL_DEPTH) != 0;
  if (n < 0 || n_obs < 0 || n_kf < 0) return LLD_ERR_INVALID;
  if ((in->flags & ~(uint32_t)(LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH)) || !(want_desc || want_norm)) return LLD_ERR_INVALID;
  if (n == 0) return LLD_OK;
  if (!in->obs_start || !in->bad || !out->updated || (n_obs > 0 && !in->obs_kf)) return LLD_ERR_INVALID;
  if (want_desc && ((n_obs > 0 && (!in->obs_desc || !in->kf_bad)) || !out->desc || !out->best_obs || !out->best_median)) return LLD_ERR_INVALID;
  if (want_norm && ((n_obs > 0 && !in->kf_ow) || !in->pos || !in->ref_kf || !in->ref_level || !in->level_scale || !out->normal ||
                    !out->min_distance || !out->max_distance))
    return LLD_ERR_INVALID;
  if (want_norm && (in->n_levels < 1 || in->n_levels > LLD_ORB_MAX_LEVELS)) return LLD_ERR_INVALID;
  int st = check_csr(n, n_obs, n_kf, in->obs_start, in->obs_kf, LLD_LANDMARK_MAX_OBS);
  if (st == LLD_ERR_INVALID) return st;
  if (want_norm)
    for (int i = 0; i < n; ++i) {
      if (in->bad[i] || in->obs_start[i + 1] == in->obs_start[i]) continue;   // never read for a point the rule skips
      if (in->ref_kf[i] < 0 || in->ref_kf[i] >= n_kf || in->ref_level[i] < 0 || in->ref_level[i] >= in->n_levels) return LLD_ERR_INVALID;
    }
  if (st) return st;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  // the two launch lists of the descriptor part, by kept observations
  std::vector<int32_t> list;
  int n_wave = 0;
  if (want_desc) {
    list.resize((size_t)n);
    std::vector<int32_t> big;
    for (int i = 0; i < n; ++i) {
      int kept = 0;
      for (int o = in->obs_start[i]; o < in->obs_start[i + 1]; ++o) kept += in->kf_bad[in->obs_kf[o]] == 0;
      if (kept <= kWave) list[n_wave++] = i; else big.push_back(i);
    }
    for (size_t q = 0; q < big.size(); ++q) list[n_wave + q] = big[q];
  }
  const int n_block = want_desc ? n - n_wave : 0;

  size_t inb = 0, outb = 0;
  auto add_in = [&](size_t b) { const size_t o = inb; inb += al(b); return o; };
  auto add_out = [&](size_t b) { const size_t o = outb; outb += al(b); return o; };
  const size_t o_start = add_in((size_t)(n + 1) * 4), o_kf = add_in((size_t)n_obs * 4), o_bad = add_in((size_t)n);
  const size_t o_desc = want_desc ? add_in((size_t)n_obs * 32) : 0, o_kfbad = want_desc ? add_in((size_t)n_kf) : 0;
  const size_t o_list = want_desc ? add_in((size_t)n * 4) : 0;
  const size_t o_ow = want_norm ? add_in((size_t)n_kf * 12) : 0, o_pos = want_norm ? add_in((size_t)n * 12) : 0;
  const size_t o_rkf = want_norm ? add_in((size_t)n * 4) : 0, o_rlv = want_norm ? add_in((size_t)n * 4) : 0;
  const size_t o_scale = want_norm ? add_in((size_t)LLD_ORB_MAX_LEVELS * 4) : 0;
  const size_t r_desc = want_desc ? add_out((size_t)n * 32) : 0, r_bo = want_desc ? add_out((size_t)n * 4) : 0;
  const size_t r_bm = want_desc ? add_out((size_t)n * 4) : 0, r_ud = want_desc ? add_out((size_t)n) : 0;
  const size_t r_nrm = want_norm ? add_out((size_t)n * 12) : 0, r_min = want_norm ? add_out((size_t)n * 4) : 0;
  const size_t r_max = want_norm ? add_out((size_t)n * 4) : 0, r_un = want_norm ? add_out((size_t)n) : 0;
  void* hb; st = lld_ctx_pinned(ctx, inb + outb, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, inb + outb + 256, &db); if (st) return st;
  char* h = (char*)hb; char* d = (char*)db; char* h_out = h + inb; char* d_out = d + inb;
  std::memcpy(h + o_start, in->obs_start, (size_t)(n + 1) * 4);
  if (n_obs) std::memcpy(h + o_kf, in->obs_kf, (size_t)n_obs * 4);
  std::memcpy(h + o_bad, in->bad, (size_t)n);
  if (want_desc) {
    if (n_obs) std::memcpy(h + o_desc, in->obs_desc, (size_t)n_obs * 32);
    if (n_kf && in->kf_bad) std::memcpy(h + o_kfbad, in->kf_bad, (size_t)n_kf);
    std::memcpy(h + o_list, list.data(), (size_t)n * 4);
  }
  if (want_norm) {
    if (n_kf && in->kf_ow) std::memcpy(h + o_ow, in->kf_ow, (size_t)n_kf * 12);
    std::memcpy(h + o_pos, in->pos, (size_t)n * 12);
    std::memcpy(h + o_rkf, in->ref_kf, (size_t)n * 4); std::memcpy(h + o_rlv, in->ref_level, (size_t)n * 4);
    std::memcpy(h + o_scale, in->level_scale, (size_t)in->n_levels * 4);
  }
  hipStream_t sm = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(d, h, inb, hipMemcpyHostToDevice, sm));
  if (want_desc) {
    PointArgs A;
    A.obs_start = reinterpret_cast<const int32_t*>(d + o_start); A.obs_kf = reinterpret_cast<const int32_t*>(d + o_kf);
    A.obs_desc = reinterpret_cast<const uint32_t*>(d + o_desc); A.kf_bad = reinterpret_cast<const uint8_t*>(d + o_kfbad);
    A.bad = reinterpret_cast<const uint8_t*>(d + o_bad); A.list = reinterpret_cast<const int32_t*>(d + o_list);
    A.desc = reinterpret_cast<uint32_t*>(d_out + r_desc); A.best_obs = reinterpret_cast<int32_t*>(d_out + r_bo);
    A.best_median = reinterpret_cast<int32_t*>(d_out + r_bm); A.upd = reinterpret_cast<uint8_t*>(d_out + r_ud);
    if (n_wave) hipLaunchKernelGGL(lm_point_wave, dim3(n_wave), dim3(kWave), 0, sm, A);
    if (n_block) { A.list += n_wave; hipLaunchKernelGGL(lm_point_block, dim3(n_block), dim3(kBlock), 0, sm, A); }
  }
  if (want_norm) {
    NormalArgs B;
    B.obs_start = reinterpret_cast<const int32_t*>(d + o_start); B.obs_kf = reinterpret_cast<const int32_t*>(d + o_kf);
    B.kf_ow = reinterpret_cast<const float*>(d + o_ow); B.pos = reinterpret_cast<const float*>(d + o_pos);
    B.bad = reinterpret_cast<const uint8_t*>(d + o_bad); B.ref_kf = reinterpret_cast<const int32_t*>(d + o_rkf);
    B.ref_level = reinterpret_cast<const int32_t*>(d + o_rlv); B.level_scale = reinterpret_cast<const float*>(d + o_scale);
    B.n_levels = in->n_levels;
    B.normal = reinterpret_cast<float*>(d_out + r_nrm); B.min_distance = reinterpret_cast<float*>(d_out + r_min);
    B.max_distance = reinterpret_cast<float*>(d_out + r_max); B.upd = reinterpret_cast<uint8_t*>(d_out + r_un);
    hipLaunchKernelGGL(lm_normal_wave, dim3(n), dim3(kWave), 0, sm, B);
  }
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(h_out, d_out, outb, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  // scatter: a landmark the rule left alone keeps what the caller passed in
  const uint8_t* ud = reinterpret_cast<const uint8_t*>(h_out + r_ud); const uint8_t* un = reinterpret_cast<const uint8_t*>(h_out + r_un);
  for (int i = 0; i < n; ++i) {
    uint8_t u = 0;
    if (want_desc) {
      out->best_obs[i] = reinterpret_cast<const int32_t*>(h_out + r_bo)[i];
      out->best_median[i] = reinterpret_cast<const int32_t*>(h_out + r_bm)[i];
      if (ud[i]) { std::memcpy(out->desc + (size_t)i * 8, h_out + r_desc + (size_t)i * 32, 32); u |= LLD_LANDMARK_DESCRIPTOR; }
    }
    if (want_norm && un[i]) {
      std::memcpy(out->normal + (size_t)i * 3, h_out + r_nrm + (size_t)i * 12, 12);
      out->min_distance[i] = reinterpret_cast<const float*>(h_out + r_min)[i];
      out->max_distance[i] = reinterpret_cast<const float*>(h_out + r_max)[i];
      u |= LLD_LANDMARK_NORMAL_DEPTH;
    }
    out->updated[i] = u;
  }
  return LLD_OK;
}

int lld_mapline_distinctive(lld_ctx* ctx, const lld_mapline_distinctive_in* in, lld_mapline_distinctive_out* out) {
  if (!ctx || !in || !out) return LLD_ERR_INVALID;
  const int32_t n = in->n_lines, n_obs = in->n_obs, n_kf = in->n_kf, dim = in->dim;
  if (n < 0 || n_obs < 0 || n_kf < 0) return LLD_ERR_INVALID;
  if (n == 0) return LLD_OK;
  if (dim < 1) return LLD_ERR_INVALID;
  if (!in->obs_start || !in->bad || (n_obs > 0 && (!in->obs_kf || !in->obs_desc || !in->kf_bad)) || !out->desc || !out->best_obs ||
      !out->best_median || !out->updated)
    return LLD_ERR_INVALID;
  int st = check_csr(n, n_obs, n_kf, in->obs_start, in->obs_kf, LLD_LANDMARK_MAX_LINE_OBS);
  if (st == LLD_ERR_INVALID) return st;
  if (dim > LLD_LANDMARK_MAX_LINE_DIM) return LLD_ERR_UNSUPPORTED;
  if (st) return st;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  size_t inb = 0, outb = 0;
  auto add_in = [&](size_t b) { const size_t o = inb; inb += al(b); return o; };
  auto add_out = [&](size_t b) { const size_t o = outb; outb += al(b); return o; };
  const size_t o_start = add_in((size_t)(n + 1) * 4), o_kf = add_in((size_t)n_obs * 4), o_bad = add_in((size_t)n);
  const size_t o_desc = add_in((size_t)n_obs * dim * 4), o_kfbad = add_in((size_t)n_kf);
  const size_t r_desc = add_out((size_t)n * dim * 4), r_bo = add_out((size_t)n * 4), r_bm = add_out((size_t)n * 4), r_u = add_out((size_t)n);
  void* hb; st = lld_ctx_pinned(ctx, inb + outb, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, inb + outb + 256, &db); if (st) return st;
  char* h = (char*)hb; char* d = (char*)db; char* h_out = h + inb; char* d_out = d + inb;
  std::memcpy(h + o_start, in->obs_start, (size_t)(n + 1) * 4);
  std::memcpy(h + o_bad, in->bad, (size_t)n);
  if (n_obs) {
    std::memcpy(h + o_kf, in->obs_kf, (size_t)n_obs * 4);
    std::memcpy(h + o_desc, in->obs_desc, (size_t)n_obs * dim * 4);
  }
  if (n_kf && in->kf_bad) std::memcpy(h + o_kfbad, in->kf_bad, (size_t)n_kf);
  LineArgs A;
  A.obs_start = reinterpret_cast<const int32_t*>(d + o_start); A.obs_kf = reinterpret_cast<const int32_t*>(d + o_kf);
  A.obs_desc = reinterpret_cast<const float*>(d + o_desc); A.kf_bad = reinterpret_cast<const uint8_t*>(d + o_kfbad);
  A.bad = reinterpret_cast<const uint8_t*>(d + o_bad); A.dim = dim;
  A.desc = reinterpret_cast<float*>(d_out + r_desc); A.best_obs = reinterpret_cast<int32_t*>(d_out + r_bo);
  A.best_median = reinterpret_cast<int32_t*>(d_out + r_bm); A.upd = reinterpret_cast<uint8_t*>(d_out + r_u);
  hipStream_t sm = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(d, h, inb, hipMemcpyHostToDevice, sm));
  const size_t lds = ((size_t)kWave * (dim | 1) + (size_t)kWave * kWave) * sizeof(float);
  hipLaunchKernelGGL(lm_line_wave, dim3(n), dim3(kWave), lds, sm, A);
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(h_out, d_out, outb, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  const uint8_t* u = reinterpret_cast<const uint8_t*>(h_out + r_u);
  for (int i = 0; i < n; ++i) {
    out->best_obs[i] = reinterpret_cast<const int32_t*>(h_out + r_bo)[i];
    out->best_median[i] = reinterpret_cast<const int32_t*>(h_out + r_bm)[i];
    if (u[i]) std::memcpy(out->desc + (size_t)i * dim, h_out + r_desc + (size_t)i * dim * 4, (size_t)dim * 4);
    out->updated[i] = u[i] ? LLD_LANDMARK_DESCRIPTOR : 0;
  }
  return LLD_OK;
}

}  // extern "C"
