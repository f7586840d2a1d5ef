// lld_map_refresh.hip — MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth (src/MapPoint.cc:242-307, :330-371) and
// MapLine::ComputeDistinctiveDescriptors (src/MapLine.cc:133-201) on the resident map's tables: lld_map_refresh_points and
// lld_map_refresh_lines take a list of landmark slots, read the observation and index rows, the keyframes' bad flags, centres, octaves and
// descriptor rows where the map keeps them, and write p_desc / p_nrm / p_mind / p_maxd / l_desc in place.  The rules and the numerics are
// those of lld_mappoint_refresh / lld_mapline_distinctive (lld_landmark.hip), restated on how a descriptor row is fetched: through the
// landmark's index row into the keyframe's descriptor pool, not from a gathered array.  lld_map_download_points / _lines read the fixed
// rows back for an audit.  Shared with lld_landmark.hip: the selection cores (lld_distinctive.h); with lld_map_apply.hip: the ordered sum and
// the reference keyframe's level (lld_normal_depth.h); with every call on the map: the staging pair (lld_map_tables.h) and the timed upload /
// launches / download (lld_round_trip.h).
//
//   rf_check_kernel    sixteen lanes per named point: the early return, and every index held to the row it points into before any other
//                      kernel follows it - the verdict byte the kernels below obey, the reference keyframe and the level of the normal part
//   rf_point_wave      one wavefront per point with a stored row of at most 64: the kept observers compacted in row order by ballot, lane i
//                      holds descriptor i, rows reach every lane by lane broadcast, a lane's distances lie in LDS (uint16, lane-contiguous),
//                      sorted[idx] by bisection on the value, a wavefront min on (median << 16 | i)
//   rf_point_block     one workgroup of 256 per point with a stored row of 65 .. LLD_LANDMARK_MAX_OBS: descriptors in LDS, rows strided over
//                      the lanes, the same bisection with the distances recomputed from LDS
//   rf_normal_kernel   sixteen lanes per point: each lane forms terms, every lane adds them in row order (lld_normal_depth.h)
//   rf_line_wave       one wavefront per line: its own checks, rows in LDS (odd stride), float distances in LDS, sorted[idx] by rank count,
//                      the truncation to int, a wavefront min on (median, i)
//   rf_points_out / rf_lines_out   the outputs, read from the tables behind the writes
// No atomics, no scratch.  Every landmark is handled by one workgroup (one group of sixteen lanes) that reads nothing another one of the call
// writes: descriptors are read from keyframe pools and written to landmark rows, the normal part reads p_pos and writes p_nrm / p_mind /
// p_maxd of its own slot.  A slot is named at most once per call, so the result cannot depend on the query list.
#pragma clang fp contract(off)

#include <vector>

#include "lld_common.h"
#include "lld_distinctive.h"
#include "lld_map_tables.h"
#include "lld_normal_depth.h"
#include "lld_round_trip.h"
#include "lld_wave.h"

namespace {

using lld_map_dev::MapBa;
using lld_map_dev::MapDesc;
using lld_map_dev::MapDev;
using lld_map_dev::MapExt;
using lld_rt::blocks;
using lld_rt::copy_out;
using lld_rt::round_trip;
using lld_track::Span;
using lld_track::UploadBlock;

constexpr int kWave = 64;
constexpr int kBlock = 256;
static_assert(kWave == lld_dd::kWave && kBlock == lld_dd::kBlock, "lld_distinctive.h is written for these");
constexpr int kGroup = 16, kGroups = kBlock / kGroup;
constexpr uint8_t kDesc = LLD_LANDMARK_DESCRIPTOR, kNormal = LLD_LANDMARK_NORMAL_DEPTH;
constexpr uint8_t kNoIndex = LLD_MAP_REFRESH_NO_INDEX, kNoDesc = LLD_MAP_REFRESH_NO_DESCRIPTOR, kNoRef = LLD_MAP_REFRESH_NO_REFERENCE;
constexpr uint8_t kEarly = 0x80;                 // verdict only: the routine returns before it reads anything else

struct RfArgs {
  int32_t n, n_levels, want_desc, want_norm, has_ext, has_ba, has_desc;
  const int32_t* slot; const int32_t* list; const float* level_scale;
  const int32_t* p_ref;                          // null: lld_map_set_point_refs was never called
  uint8_t* verdict; int32_t* t_ref; int32_t* t_level;
  uint32_t* o_desc; int32_t* o_best; int32_t* o_med; float* o_nrm; float* o_mind; float* o_maxd; uint8_t* o_upd;
};

struct RfLineArgs {
  int32_t n, has_ba, has_desc;
  const int32_t* slot;
  float* o_desc; int32_t* o_best; int32_t* o_med; uint8_t* o_upd;
};

// ------------------------------------------------------------------------------------------------ points: what may be followed
__global__ __launch_bounds__(kBlock) void rf_check_kernel(MapDev M, MapExt X, MapBa Y, MapDesc Z, RfArgs A) {
  const int g = threadIdx.x / kGroup, gl = threadIdx.x % kGroup;
  for (int base = blockIdx.x * kGroups; base < A.n; base += gridDim.x * kGroups) {         // uniform over the workgroup
    const int q = base + g;
    const bool on = q < A.n;
    int s = 0; int2 row = make_int2(0, 0), ir = make_int2(0, 0); int ref = -1; uint8_t v = 0;
    if (on) {
      s = A.slot[q]; row = M.p_obs[s];
      if (M.p_state[s] != 1 || row.y <= 0) v = kEarly;                 // mbBad or never set, observations.empty()
      else {
        if (A.has_ext) ir = X.p_idx[s];
        if (ir.y != row.y) v = kNoIndex;
        if (A.p_ref) ref = A.p_ref[s];
      }
    }
    const int len = (on && !v) ? row.y : 0;
    int no_desc = 0, no_centre = 0, ref_at = 0x7fffffff;
    for (int j = gl; j < len; j += kGroup) {
      const int kf = M.obs_pool[row.x + j], idx = X.idx_pool[ir.x + j];
      if (A.want_desc && M.k_bad[kf] == 0) {
        const int2 dr = A.has_desc ? Z.k_desc[kf] : make_int2(0, 0);
        if (8 * (long long)idx + 8 > dr.y) no_desc = 1;
      }
      if (A.want_norm) {
        if (!A.has_ba || !Y.k_feat[kf]) no_centre = 1;
        if (kf == ref) ref_at = min(ref_at, j);
      }
    }
    ref_at = lld_wave::min<kGroup>(ref_at);
    lld_wave::sum_each<kGroup>(no_desc, no_centre);
    if (!on || gl != 0) continue;
    int level = 0;
    if (len) {
      if (no_desc) v |= kNoDesc;
      if (A.want_norm) {
        level = -1;                                // of the reference keyframe's own observation
        if (ref >= 0 && !no_centre && A.has_ext && A.has_ba) level = lld_nd::ref_level(ref, ref_at, len, X.idx_pool + ir.x, X.k_oct, X.oct_pool, Y.k_feat, A.n_levels);
        if (level < 0) { v |= kNoRef; level = 0; }
      }
    }
    A.verdict[q] = v; A.t_ref[q] = ref; A.t_level[q] = level;
    A.o_upd[q] = v & (uint8_t)~kEarly; A.o_best[q] = -1; A.o_med[q] = -1;
  }
}

// The observers of a checked point whose keyframe is not bad, in row order, chunk by chunk: kept[r] = position in the stored row, src[r] = where
// the observer's descriptor starts in the keyframes' pool.  One whole wavefront calls it; returns the count (the same in every lane).
__device__ __forceinline__ int compact_kept(const MapDev& M, const MapExt& X, const MapDesc& Z, int2 row, int2 ir, int len, int lane, int* kept, int* src) {
  int n = 0;
  for (int c = 0; c < len; c += kWave) {
    const int j = c + lane;
    bool keep = false; int off = 0;
    if (j < len) {
      const int kf = M.obs_pool[row.x + j];
      keep = M.k_bad[kf] == 0;
      if (keep) off = Z.k_desc[kf].x + 8 * X.idx_pool[ir.x + j];     // rf_check_kernel held the index to the row
    }
    const unsigned long long m = __ballot(keep);
    if (keep) { const int r = n + __popcll(m & ((1ull << lane) - 1ull)); kept[r] = j; src[r] = off; }
    n += __popcll(m);
  }
  return n;
}

// grid: the short rows of the list, block 64
__global__ __launch_bounds__(kWave) void rf_point_wave(MapDev M, MapExt X, MapDesc Z, RfArgs A, int first) {
  __shared__ int kept[kWave];
  __shared__ int src[kWave];
  __shared__ uint16_t dist[kWave * kWave];       // dist[j * 64 + i] = DescriptorDistance(row i, row j)
  const int lane = threadIdx.x;
  const int q = A.list[first + blockIdx.x];
  if (A.verdict[q]) return;                      // (uniform)
  const int s = A.slot[q];
  const int2 row = M.p_obs[s], ir = X.p_idx[s];
  const int N = compact_kept(M, X, Z, row, ir, row.y < kWave ? row.y : kWave, lane, kept, src);     // the host sends only rows of at most 64 here
  __syncthreads();
  if (N == 0) return;                            // vDescriptors.empty(): return (:269-270)
  uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
  if (lane < N) {
    const uint4* from = reinterpret_cast<const uint4*>(Z.kdesc_pool + src[lane]);   // rows start at multiples of eight words
    d0 = from[0]; d1 = from[1];
  }
  const int key = lld_dd::point_wave(d0, d1, N, lane, dist);
  const int w = key & 0xffff;
  if (lane < 8) M.p_desc[8 * (size_t)s + lane] = (uint32_t)Z.kdesc_pool[src[w] + lane];
  if (lane == 0) { A.o_best[q] = kept[w]; A.o_med[q] = key >> 16; A.o_upd[q] |= kDesc; }
}

// grid: the long rows of the list, block 256
__global__ __launch_bounds__(kBlock) void rf_point_block(MapDev M, MapExt X, MapDesc Z, RfArgs A, int first) {
  __shared__ int kept[LLD_LANDMARK_MAX_OBS];
  __shared__ int src[LLD_LANDMARK_MAX_OBS];
  __shared__ uint4 rows[LLD_LANDMARK_MAX_OBS * 2];
  __shared__ int red[kBlock / kWave];
  __shared__ int sN;
  const int tid = threadIdx.x;
  const int q = A.list[first + blockIdx.x];
  if (A.verdict[q]) return;                      // (uniform)
  const int s = A.slot[q];
  const int2 row = M.p_obs[s], ir = X.p_idx[s];
  if (tid < kWave) {
    const int n = compact_kept(M, X, Z, row, ir, row.y < LLD_LANDMARK_MAX_OBS ? row.y : LLD_LANDMARK_MAX_OBS, tid, kept, src);   // the host refuses a longer row
    if (tid == 0) sN = n;
  }
  __syncthreads();
  const int N = sN;
  if (N == 0) return;
  for (int k = tid; k < 2 * N; k += kBlock) rows[k] = reinterpret_cast<const uint4*>(Z.kdesc_pool + src[k >> 1])[k & 1];
  __syncthreads();
  const int key = lld_dd::point_block(rows, N, tid, red);
  const int w = key & 0xffff;
  if (tid < 8) M.p_desc[8 * (size_t)s + tid] = reinterpret_cast<const uint32_t*>(rows + 2 * w)[tid];
  if (tid == 0) { A.o_best[q] = kept[w]; A.o_med[q] = key >> 16; A.o_upd[q] |= kDesc; }
}

// ------------------------------------------------------------------------------------------------ points: UpdateNormalAndDepth
__global__ __launch_bounds__(kBlock) void rf_normal_kernel(MapDev M, MapBa Y, RfArgs A) {
  const int g = threadIdx.x / kGroup, gl = threadIdx.x % kGroup;
  for (int base = blockIdx.x * kGroups; base < A.n; base += gridDim.x * kGroups) {         // uniform over the workgroup
    const int q = base + g;
    const bool on = q < A.n && A.verdict[q] == 0;
    int s = 0; int2 row = make_int2(0, 0);
    float px = 0.f, py = 0.f, pz = 0.f;
    if (on) { s = A.slot[q]; row = M.p_obs[s]; px = M.p_pos[3 * (size_t)s]; py = M.p_pos[3 * (size_t)s + 1]; pz = M.p_pos[3 * (size_t)s + 2]; }
    const int len = on ? row.y : 0;              // every stored observer counts: bad keyframes are not skipped (:348-357)
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int j0 = 0; j0 < len; j0 += kGroup) {
      const int j = j0 + gl;
      float tx = 0.f, ty = 0.f, tz = 0.f; int keep = 0;
      if (j < len) { keep = 1; lld_nd::term(px, py, pz, Y.k_ow + 3 * (size_t)M.obs_pool[row.x + j], tx, ty, tz); }
      lld_nd::add_in_order<kGroup>(keep, tx, ty, tz, nx, ny, nz);
    }
    if (on && gl == 0) {
      lld_nd::finish(lld_nd::Out{M.p_nrm, M.p_mind, M.p_maxd}, s, px, py, pz, nx, ny, nz, len, Y.k_ow + 3 * (size_t)A.t_ref[q], A.level_scale, A.t_level[q],
                     A.n_levels);
      A.o_upd[q] |= kNormal;
    }
  }
}

// one lane per word of a descriptor: q = i / 8
__global__ void rf_points_out_kernel(MapDev M, RfArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)A.n * 8) return;
  const int q = (int)(i >> 3), w = (int)(i & 7);
  const size_t s = (size_t)A.slot[q];
  A.o_desc[i] = M.p_desc[8 * s + w];
  if (w < 3) A.o_nrm[3 * (size_t)q + w] = M.p_nrm[3 * s + w];
  if (w == 3) A.o_mind[q] = M.p_mind[s];
  if (w == 4) A.o_maxd[q] = M.p_maxd[s];
}

// ------------------------------------------------------------------------------------------------ lines
// grid: n, block 64; dynamic LDS: 64 * (dim | 1) floats of rows, 64 * 64 floats of distances, then kept[64] and src[64]
__global__ __launch_bounds__(kWave) void rf_line_wave(MapDev M, MapBa Y, MapDesc Z, RfLineArgs A) {
  extern __shared__ __align__(16) float rf_smem[];
  const int dim = M.dim, stride = M.dim | 1;
  float* rows = rf_smem;
  float* dist = rf_smem + kWave * stride;        // dist[j * 64 + i] = (float)cv::norm(row i - row j)
  int* kept = reinterpret_cast<int*>(dist + kWave * kWave);
  int* src = kept + kWave;
  const int lane = threadIdx.x;
  const int q = blockIdx.x;
  const int s = A.slot[q];
  int2 row = make_int2(0, 0), ir = make_int2(0, 0);
  if (A.has_ba && M.l_bad[s] == 0) { row = Y.l_obs[s]; ir = Y.l_idx[s]; }
  if (row.y <= 0) {                              // mbBad or never set, observations.empty()
    if (lane == 0) { A.o_best[q] = -1; A.o_med[q] = -1; A.o_upd[q] = 0; }
    return;
  }
  const int len = row.y < kWave ? row.y : kWave; // the host refuses a longer row
  bool keep = false, missing = false; int off = 0;
  if (ir.y == row.y && lane < len) {
    const int kf = Y.lobs_pool[row.x + lane], idx = Y.lidx_pool[ir.x + lane];
    keep = M.k_bad[kf] == 0;
    if (keep) {
      const int2 dr = A.has_desc ? Z.k_ldesc[kf] : make_int2(0, 0);
      missing = (long long)dim * idx + dim > dr.y;
      if (!missing) off = dr.x + dim * idx;
    }
  }
  const uint8_t flags = (uint8_t)((ir.y != row.y ? kNoIndex : 0) | (__ballot(missing) ? kNoDesc : 0));
  const unsigned long long m = __ballot(keep);
  const int N = __popcll(m);
  if (flags || N == 0) {
    if (lane == 0) { A.o_best[q] = -1; A.o_med[q] = -1; A.o_upd[q] = flags; }
    return;
  }
  if (keep) { const int r = __popcll(m & ((1ull << lane) - 1ull)); kept[r] = lane; src[r] = off; }
  __syncthreads();
  for (int r = 0; r < N; ++r) {
    const int32_t* from = Z.kldesc_pool + src[r];
    for (int k = lane; k < dim; k += kWave) rows[r * stride + k] = __int_as_float(from[k]);
  }
  __syncthreads();
  const int2 best = lld_dd::line(rows, dist, N, dim, stride, lane);
  const int mi = best.x, bi = best.y;
  for (int k = lane; k < dim; k += kWave) M.l_desc[(size_t)s * dim + k] = rows[bi * stride + k];
  if (lane == 0) { A.o_best[q] = kept[bi]; A.o_med[q] = mi; A.o_upd[q] = kDesc; }
}

__global__ void rf_lines_out_kernel(MapDev M, RfLineArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)A.n * M.dim) return;
  const int q = (int)(i / M.dim), c = (int)(i % M.dim);
  A.o_desc[i] = M.l_desc[(size_t)A.slot[q] * M.dim + c];
}

// ------------------------------------------------------------------------------------------------ lld_map_download_points / _lines
struct DlArgs { int32_t n; const int32_t* slot; float* pos; float* nrm; float* mind; float* maxd; uint32_t* desc; uint8_t* state; };
__global__ void rf_download_points_kernel(MapDev M, DlArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)A.n * 8) return;
  const int q = (int)(i >> 3), w = (int)(i & 7);
  const size_t s = (size_t)A.slot[q];
  A.desc[i] = M.p_desc[8 * s + w];
  if (w < 3) { A.pos[3 * (size_t)q + w] = M.p_pos[3 * s + w]; A.nrm[3 * (size_t)q + w] = M.p_nrm[3 * s + w]; }
  if (w == 3) { A.mind[q] = M.p_mind[s]; A.maxd[q] = M.p_maxd[s]; }
  if (w == 4) A.state[q] = M.p_state[s];
}
__global__ void rf_download_lines_kernel(MapDev M, int n, const int32_t* slot, float* desc, uint8_t* bad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * M.dim) return;
  const int q = (int)(i / M.dim), c = (int)(i % M.dim);
  const size_t s = (size_t)slot[q];
  desc[i] = M.l_desc[s * M.dim + c];
  if (c == 0) bad[q] = M.l_bad[s];
}

// ------------------------------------------------------------------------------------------------ host
using lld_map_dev::slots_ok;

}  // namespace

int lld_map_dev::refresh_descriptors_queue(hipStream_t sm, const lld_map* m, const DescRefresh& R) {
  if (R.n <= 0) return LLD_OK;
  RfArgs A{};
  A.n = R.n; A.want_desc = 1; A.has_ext = m->d_ext != nullptr; A.has_ba = m->d_ba != nullptr; A.has_desc = m->d_desc != nullptr;
  A.slot = R.slot; A.list = R.list; A.p_ref = m->d_ref;
  A.verdict = R.verdict; A.t_ref = R.t_ref; A.t_level = R.t_level; A.o_best = R.o_best; A.o_med = R.o_med; A.o_upd = R.o_upd;
  const dim3 grouped((unsigned)std::min<size_t>(std::max<size_t>(((size_t)R.n + kGroups - 1) / kGroups, 1), 2048));
  hipLaunchKernelGGL(rf_check_kernel, grouped, dim3(kBlock), 0, sm, m->D, m->X, m->Y, m->Z, A);
  if (R.n_wave) hipLaunchKernelGGL(rf_point_wave, dim3(R.n_wave), dim3(kWave), 0, sm, m->D, m->X, m->Z, A, 0);
  if (R.n - R.n_wave) hipLaunchKernelGGL(rf_point_block, dim3(R.n - R.n_wave), dim3(kBlock), 0, sm, m->D, m->X, m->Z, A, R.n_wave);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

extern "C" {

int lld_map_refresh_points(lld_map* m, const lld_map_refresh_points_in* in, lld_map_refresh_points_out* out) {
  if (!m || !in || !out) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  const int32_t n = in->n;
  const bool want_desc = (in->flags & LLD_LANDMARK_DESCRIPTOR) != 0, want_norm = (in->flags & LLD_LANDMARK_NORMAL_DEPTH) != 0;
  if (n < 0) return LLD_ERR_INVALID;
  if ((in->flags & ~(uint32_t)(LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH)) || !(want_desc || want_norm)) return LLD_ERR_INVALID;
  if (n == 0) return LLD_OK;
  if (!in->slot || !out->updated) return LLD_ERR_INVALID;
  if (want_norm && (!in->level_scale || in->n_levels < 1 || in->n_levels > LLD_ORB_MAX_LEVELS)) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_pt, m->epoch, n, in->slot)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (m->obs.len[in->slot[i]] > LLD_LANDMARK_MAX_OBS) return LLD_ERR_UNSUPPORTED;
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  const size_t nn = (size_t)n;
  UploadBlock B;
  const auto u_slot = B.take<int32_t>(nn), u_list = B.take<int32_t>(nn); const auto u_ls = B.take<float>(LLD_ORB_MAX_LEVELS);
  B.end_upload();
  const auto r_desc = B.take<uint32_t>(nn, 8); const auto r_best = B.take<int32_t>(nn), r_med = B.take<int32_t>(nn);
  const auto r_nrm = B.take<float>(nn, 3), r_min = B.take<float>(nn), r_max = B.take<float>(nn); const auto r_upd = B.take<uint8_t>(nn);
  B.end_download();
  const auto t_v = B.take<uint8_t>(nn); const auto t_ref = B.take<int32_t>(nn), t_lv = B.take<int32_t>(nn);
  int st = m->rf.grow(ctx->stream, B.travel_bytes(), B.size); if (st) return st;
  B.bind(m->rf.h, m->rf.d);

  // the two launch lists of the descriptor part, by the stored row's length (the host's lengths are the device's)
  B.stage(u_slot, in->slot);
  int32_t* list = B.host(u_list);
  int n_wave = 0;
  for (int i = 0; i < n; i++) if (m->obs.len[in->slot[i]] <= kWave) list[n_wave++] = i;
  for (int i = 0, k = n_wave; i < n; i++) if (m->obs.len[in->slot[i]] > kWave) list[k++] = i;
  const int n_block = n - n_wave;
  std::memset(B.host(u_ls), 0, LLD_ORB_MAX_LEVELS * sizeof(float));
  if (want_norm) std::memcpy(B.host(u_ls), in->level_scale, (size_t)in->n_levels * sizeof(float));

  RfArgs A{};
  A.n = n; A.n_levels = want_norm ? in->n_levels : 0; A.want_desc = want_desc; A.want_norm = want_norm;
  A.has_ext = m->d_ext != nullptr; A.has_ba = m->d_ba != nullptr; A.has_desc = m->d_desc != nullptr;
  A.slot = B.dev(u_slot); A.list = B.dev(u_list); A.level_scale = B.dev(u_ls); A.p_ref = m->d_ref;
  A.verdict = B.dev(t_v); A.t_ref = B.dev(t_ref); A.t_level = B.dev(t_lv);
  A.o_desc = B.dev(r_desc); A.o_best = B.dev(r_best); A.o_med = B.dev(r_med); A.o_nrm = B.dev(r_nrm); A.o_mind = B.dev(r_min); A.o_maxd = B.dev(r_max);
  A.o_upd = B.dev(r_upd);

  st = round_trip(ctx->stream, B, out->phase_ms, [&](hipStream_t sm) {
    const dim3 grouped((unsigned)std::min<size_t>(std::max<size_t>((nn + kGroups - 1) / kGroups, 1), 2048));
    hipLaunchKernelGGL(rf_check_kernel, grouped, dim3(kBlock), 0, sm, m->D, m->X, m->Y, m->Z, A);
    if (want_desc && n_wave) hipLaunchKernelGGL(rf_point_wave, dim3(n_wave), dim3(kWave), 0, sm, m->D, m->X, m->Z, A, 0);
    if (want_desc && n_block) hipLaunchKernelGGL(rf_point_block, dim3(n_block), dim3(kBlock), 0, sm, m->D, m->X, m->Z, A, n_wave);
    if (want_norm) hipLaunchKernelGGL(rf_normal_kernel, grouped, dim3(kBlock), 0, sm, m->D, m->Y, A);
    hipLaunchKernelGGL(rf_points_out_kernel, blocks(nn * 8, kBlock), dim3(kBlock), 0, sm, m->D, A);
    return LLD_OK;
  });
  if (st) { m->poisoned = true; return st; }                           // what the tables hold is not known
  const uint8_t* upd = B.host(r_upd);
  bool wrote = false;
  for (size_t i = 0; i < nn; i++) wrote = wrote || (upd[i] & (kDesc | kNormal));
  if (wrote) { m->mutations++; m->win.valid = false; }
  copy_out(out->desc, B, r_desc, nn * 8); copy_out(out->best_obs, B, r_best, nn); copy_out(out->best_median, B, r_med, nn);
  copy_out(out->normal, B, r_nrm, nn * 3); copy_out(out->min_distance, B, r_min, nn); copy_out(out->max_distance, B, r_max, nn);
  copy_out(out->updated, B, r_upd, nn);
  return LLD_OK;
}

int lld_map_refresh_lines(lld_map* m, const lld_map_refresh_lines_in* in, lld_map_refresh_lines_out* out) {
  if (!m || !in || !out) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  const int32_t n = in->n;
  if (n < 0) return LLD_ERR_INVALID;
  if (n == 0) return LLD_OK;
  if (!in->slot || !out->updated) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_ln, m->epoch, n, in->slot)) return LLD_ERR_INVALID;
  if (m->d_ba) for (int i = 0; i < n; i++) if (m->lobs.len[in->slot[i]] > LLD_LANDMARK_MAX_LINE_OBS) return LLD_ERR_UNSUPPORTED;
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  const size_t nn = (size_t)n, dim = (size_t)m->lim.line_dim;
  UploadBlock B;
  const auto u_slot = B.take<int32_t>(nn);
  B.end_upload();
  const auto r_desc = B.take<float>(nn, dim); const auto r_best = B.take<int32_t>(nn), r_med = B.take<int32_t>(nn); const auto r_upd = B.take<uint8_t>(nn);
  B.end_download();
  int st = m->rf.grow(ctx->stream, B.travel_bytes(), B.size); if (st) return st;
  B.bind(m->rf.h, m->rf.d);
  B.stage(u_slot, in->slot);

  RfLineArgs A{};
  A.n = n; A.has_ba = m->d_ba != nullptr; A.has_desc = m->d_desc != nullptr; A.slot = B.dev(u_slot);
  A.o_desc = B.dev(r_desc); A.o_best = B.dev(r_best); A.o_med = B.dev(r_med); A.o_upd = B.dev(r_upd);
  const size_t lds = ((size_t)kWave * (dim | 1) + (size_t)kWave * kWave + 2 * kWave) * sizeof(float);     // at most 49.9 KB: line_dim <= 128

  st = round_trip(ctx->stream, B, out->phase_ms, [&](hipStream_t sm) {
    hipLaunchKernelGGL(rf_line_wave, dim3(n), dim3(kWave), lds, sm, m->D, m->Y, m->Z, A);
    hipLaunchKernelGGL(rf_lines_out_kernel, blocks(nn * dim, kBlock), dim3(kBlock), 0, sm, m->D, A);
    return LLD_OK;
  });
  if (st) { m->poisoned = true; return st; }
  const uint8_t* upd = B.host(r_upd);
  bool wrote = false;
  for (size_t i = 0; i < nn; i++) wrote = wrote || (upd[i] & kDesc);
  if (wrote) { m->mutations++; m->win.valid = false; }
  copy_out(out->desc, B, r_desc, nn * dim); copy_out(out->best_obs, B, r_best, nn); copy_out(out->best_median, B, r_med, nn); copy_out(out->updated, B, r_upd, nn);
  return LLD_OK;
}

int lld_map_download_points(lld_map* m, int32_t n, const int32_t* slot, float* pos, float* normal, float* min_distance, float* max_distance, uint32_t* desc,
                            uint8_t* state) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (slot[i] < 0 || slot[i] >= m->lim.max_points) return LLD_ERR_INVALID;
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const size_t nn = (size_t)n;
  UploadBlock B;
  const auto u_slot = B.take<int32_t>(nn);
  B.end_upload();
  const auto r_pos = B.take<float>(nn, 3), r_nrm = B.take<float>(nn, 3), r_min = B.take<float>(nn), r_max = B.take<float>(nn); const auto r_desc = B.take<uint32_t>(nn, 8);
  const auto r_state = B.take<uint8_t>(nn);
  B.end_download();
  int st;
  void* hb; st = lld_ctx_pinned(ctx, B.size, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind((char*)hb, (char*)db);
  B.stage(u_slot, slot);
  const DlArgs A{n, B.dev(u_slot), B.dev(r_pos), B.dev(r_nrm), B.dev(r_min), B.dev(r_max), B.dev(r_desc), B.dev(r_state)};
  st = round_trip(ctx->stream, B, nullptr, [&](hipStream_t sm) {
    hipLaunchKernelGGL(rf_download_points_kernel, blocks(nn * 8, kBlock), dim3(kBlock), 0, sm, m->D, A);
    return LLD_OK;
  });
  if (st) return st;
  copy_out(pos, B, r_pos, nn * 3); copy_out(normal, B, r_nrm, nn * 3); copy_out(min_distance, B, r_min, nn); copy_out(max_distance, B, r_max, nn);
  copy_out(desc, B, r_desc, nn * 8); copy_out(state, B, r_state, nn);
  return LLD_OK;
}

int lld_map_download_lines(lld_map* m, int32_t n, const int32_t* slot, float* desc, uint8_t* bad) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (slot[i] < 0 || slot[i] >= m->lim.max_lines) return LLD_ERR_INVALID;
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const size_t nn = (size_t)n, dim = (size_t)m->lim.line_dim;
  UploadBlock B;
  const auto u_slot = B.take<int32_t>(nn);
  B.end_upload();
  const auto r_desc = B.take<float>(nn, dim); const auto r_bad = B.take<uint8_t>(nn);
  B.end_download();
  int st;
  void* hb; st = lld_ctx_pinned(ctx, B.size, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind((char*)hb, (char*)db);
  B.stage(u_slot, slot);
  st = round_trip(ctx->stream, B, nullptr, [&](hipStream_t sm) {
    hipLaunchKernelGGL(rf_download_lines_kernel, blocks(nn * dim, kBlock), dim3(kBlock), 0, sm, m->D, n, B.dev(u_slot), B.dev(r_desc), B.dev(r_bad));
    return LLD_OK;
  });
  if (st) return st;
  copy_out(desc, B, r_desc, nn * dim); copy_out(bad, B, r_bad, nn);
  return LLD_OK;
}

}  // extern "C"
