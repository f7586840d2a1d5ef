// lld_landmark.hip — the two per-landmark routines every thread of the reference runs between its searches and optimisations:
// MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (src/MapPoint.cc:242-307, :330-371) and
// MapLine::ComputeDistinctiveDescriptors (src/MapLine.cc:133-201), for a whole batch of landmarks in one call.  The rules restated
// and the deviations are written out in include/lld_amd.h; tests/landmark_ref.py restates them independently in numpy.
//
// The whole file is compiled without FMA contraction: every float operation is the one IEEE operation the restatement performs.
// The selection of the distinctive descriptor (distances, sorted[idx], the first strictly smallest median) is lld_distinctive.h's, shared
// with lld_map_refresh.hip; the kernels here keep the compaction of the kept observations, the early return and where the winner goes.
// The host side declares its arrays on an UploadBlock (lld_upload_block.h) and travels through lld_round_trip.h.
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
#include "lld_distinctive.h"
#include "lld_normal_depth.h"
#include "lld_round_trip.h"
#include "lld_wave.h"

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;
static_assert(kWave == lld_dd::kWave && kBlock == lld_dd::kBlock, "lld_distinctive.h is written for these");

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

using lld_rt::round_trip;
using lld_track::UploadBlock;
using lld_wave::bcastf;

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
  const int key = lld_dd::point_wave(d0, d1, N, lane, dist);
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
  const int key = lld_dd::point_block(rows, N, tid, red);
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
  const int2 best = lld_dd::line(rows, dist, N, dim, stride, lane);
  const int m = best.x, bi = best.y;
  for (int k = lane; k < dim; k += kWave) A.desc[(size_t)p * dim + k] = rows[bi * stride + k];
  if (lane == 0) { A.best_obs[p] = kept[bi]; A.best_median[p] = m; A.upd[p] = 1; }
}

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

  const size_t nn = (size_t)n, no = (size_t)n_obs, nk = (size_t)n_kf, nd = want_desc ? 1 : 0, nv = want_norm ? 1 : 0;   // an array of a part not asked for is empty
  UploadBlock B;
  const auto u_start = B.take<int32_t>(nn + 1), u_kf = B.take<int32_t>(no); const auto u_bad = B.take<uint8_t>(nn);
  const auto u_desc = B.take<uint32_t>(nd * no, 8); const auto u_kfbad = B.take<uint8_t>(nd * nk); const auto u_list = B.take<int32_t>(nd * nn);
  const auto u_ow = B.take<float>(nv * nk, 3), u_pos = B.take<float>(nv * nn, 3); const auto u_rkf = B.take<int32_t>(nv * nn), u_rlv = B.take<int32_t>(nv * nn);
  const auto u_scale = B.take<float>(want_norm ? (size_t)in->n_levels : 0);
  B.end_upload();
  const auto r_desc = B.take<uint32_t>(nd * nn, 8); const auto r_bo = B.take<int32_t>(nd * nn), r_bm = B.take<int32_t>(nd * nn); const auto r_ud = B.take<uint8_t>(nd * nn);
  const auto r_nrm = B.take<float>(nv * nn, 3), r_min = B.take<float>(nv * nn), r_max = B.take<float>(nv * nn); const auto r_un = B.take<uint8_t>(nv * nn);
  B.end_download();
  void* hb; st = lld_ctx_pinned(ctx, B.size, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind((char*)hb, (char*)db);
  B.stage(u_start, in->obs_start); B.stage(u_kf, in->obs_kf); B.stage(u_bad, in->bad);
  B.stage(u_desc, in->obs_desc); B.stage(u_kfbad, in->kf_bad);
  B.stage(u_ow, in->kf_ow); B.stage(u_pos, in->pos); B.stage(u_rkf, in->ref_kf); B.stage(u_rlv, in->ref_level); B.stage(u_scale, in->level_scale);

  // the two launch lists of the descriptor part, by kept observations
  int n_wave = 0;
  if (want_desc) {
    int32_t* list = B.host(u_list);
    std::vector<int32_t> big;
    for (int i = 0; i < n; ++i) {
      int kept = 0;
      for (int o = in->obs_start[i]; o < in->obs_start[i + 1]; ++o) kept += in->kf_bad[in->obs_kf[o]] == 0;
      if (kept <= kWave) list[n_wave++] = i; else big.push_back(i);
    }
    for (size_t q = 0; q < big.size(); ++q) list[n_wave + q] = big[q];
  }
  const int n_block = want_desc ? n - n_wave : 0;

  st = round_trip(ctx->stream, B, nullptr, [&](hipStream_t sm) {
    if (want_desc) {
      PointArgs A{B.dev(u_start), B.dev(u_kf), B.dev(u_desc), B.dev(u_kfbad), B.dev(u_bad), B.dev(u_list), B.dev(r_desc), B.dev(r_bo), B.dev(r_bm), B.dev(r_ud)};
      if (n_wave) hipLaunchKernelGGL(lm_point_wave, dim3(n_wave), dim3(kWave), 0, sm, A);
      if (n_block) { A.list += n_wave; hipLaunchKernelGGL(lm_point_block, dim3(n_block), dim3(kBlock), 0, sm, A); }
    }
    if (want_norm) {
      const NormalArgs N{B.dev(u_start), B.dev(u_kf), B.dev(u_ow), B.dev(u_pos), B.dev(u_bad), B.dev(u_rkf), B.dev(u_rlv), B.dev(u_scale), in->n_levels,
                         B.dev(r_nrm), B.dev(r_min), B.dev(r_max), B.dev(r_un)};
      hipLaunchKernelGGL(lm_normal_wave, dim3(n), dim3(kWave), 0, sm, N);
    }
    return LLD_OK;
  });
  if (st) return st;
  // scatter: a landmark the rule left alone keeps what the caller passed in
  // (typed pointers as locals: B and the spans are captured by the launch above, and a byte store into `out` would make each one be read again)
  const uint8_t* ud = B.host(r_ud); const uint8_t* un = B.host(r_un);
  const int32_t* h_bo = B.host(r_bo); const int32_t* h_bm = B.host(r_bm); const uint32_t* h_desc = B.host(r_desc);
  const float* h_nrm = B.host(r_nrm); const float* h_min = B.host(r_min); const float* h_max = B.host(r_max);
  const bool desc_part = want_desc, norm_part = want_norm;
  const int count = n;
  for (int i = 0; i < count; ++i) {
    uint8_t u = 0;
    if (desc_part) {
      out->best_obs[i] = h_bo[i];
      out->best_median[i] = h_bm[i];
      if (ud[i]) { std::memcpy(out->desc + (size_t)i * 8, h_desc + (size_t)i * 8, 32); u |= LLD_LANDMARK_DESCRIPTOR; }
    }
    if (norm_part && un[i]) {
      std::memcpy(out->normal + (size_t)i * 3, h_nrm + (size_t)i * 3, 12);
      out->min_distance[i] = h_min[i];
      out->max_distance[i] = h_max[i];
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

  const size_t nn = (size_t)n, no = (size_t)n_obs;
  UploadBlock B;
  const auto u_start = B.take<int32_t>(nn + 1), u_kf = B.take<int32_t>(no); const auto u_bad = B.take<uint8_t>(nn);
  const auto u_desc = B.take<float>(no, (size_t)dim); const auto u_kfbad = B.take<uint8_t>((size_t)n_kf);
  B.end_upload();
  const auto r_desc = B.take<float>(nn, (size_t)dim); const auto r_bo = B.take<int32_t>(nn), r_bm = B.take<int32_t>(nn); const auto r_u = B.take<uint8_t>(nn);
  B.end_download();
  void* hb; st = lld_ctx_pinned(ctx, B.size, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind((char*)hb, (char*)db);
  B.stage(u_start, in->obs_start); B.stage(u_kf, in->obs_kf); B.stage(u_bad, in->bad); B.stage(u_desc, in->obs_desc); B.stage(u_kfbad, in->kf_bad);
  const LineArgs A{B.dev(u_start), B.dev(u_kf), B.dev(u_desc), B.dev(u_kfbad), B.dev(u_bad), dim, B.dev(r_desc), B.dev(r_bo), B.dev(r_bm), B.dev(r_u)};
  const size_t lds = ((size_t)kWave * (dim | 1) + (size_t)kWave * kWave) * sizeof(float);
  st = round_trip(ctx->stream, B, nullptr, [&](hipStream_t sm) {
    hipLaunchKernelGGL(lm_line_wave, dim3(n), dim3(kWave), lds, sm, A);
    return LLD_OK;
  });
  if (st) return st;
  const uint8_t* u = B.host(r_u);
  const int32_t* h_bo = B.host(r_bo); const int32_t* h_bm = B.host(r_bm); const float* h_desc = B.host(r_desc);
  const int count = n; const size_t width = (size_t)dim;
  for (int i = 0; i < count; ++i) {
    out->best_obs[i] = h_bo[i];
    out->best_median[i] = h_bm[i];
    if (u[i]) std::memcpy(out->desc + (size_t)i * width, h_desc + (size_t)i * width, width * 4);
    out->updated[i] = u[i] ? LLD_LANDMARK_DESCRIPTOR : 0;
  }
  return LLD_OK;
}

}  // extern "C"
