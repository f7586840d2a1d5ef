// lld_normal_depth.h — MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:330-371) for the kernels that run it: the term of one observation, the
// camera centre it reads and the final write, once.  lm_normal_wave (lld_landmark.hip: a wavefront per point) and the packed kernels of
// lld_map_correct.hip (several points per wavefront) differ only in how the terms reach the lane that sums them; the sum itself is
// `normal = normal + term` in observation order in all of them.  The kernels on the resident map (ap_refresh_kernel of lld_map_apply.hip,
// rf_check_kernel / rf_normal_kernel of lld_map_refresh.hip) sum rows in which some entries do not count (add_in_order) and look the
// reference keyframe's level up in the map's own rows (ref_level).  The numerics are those include/lld_amd.h states for lld_mappoint_refresh.
// Device only.  The including file is compiled under `#pragma clang fp contract(off)`: every operation here is one IEEE operation.
#ifndef LLD_NORMAL_DEPTH_H
#define LLD_NORMAL_DEPTH_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lld_wave.h"

namespace lld_nd {

// Which camera centre an observation reads.  rank == nullptr: always `older` (one table: lld_mappoint_refresh, and the essential graph's
// write-back, whose centres are all new).  Otherwise LoopClosing::CorrectLoop's interleaving (src/LoopClosing.cc:474-518): a point owned by
// rank k reads the corrected centre of a keyframe whose own rank is strictly below k (its SetPose has run), and the old one otherwise.
struct Centres { const float* older; const float* newer; const int32_t* rank; };

__device__ __forceinline__ const float* centre(const Centres& C, int kf, int k) {
  if (C.rank != nullptr && C.rank[kf] < k) return C.newer + 3 * (size_t)kf;
  return C.older + 3 * (size_t)kf;
}

// cv::norm of a 3-vector of floats: the squares summed in double in index order, the square root in double
__device__ __forceinline__ double norm3(float x, float y, float z) {
  double s = (double)x * (double)x;
  s += (double)y * (double)y;
  s += (double)z * (double)z;
  return __dsqrt_rn(s);
}

// normali/cv::norm(normali) of one observation: normali = mWorldPos - Owi (:354), Mat / double (:355)
__device__ __forceinline__ void term(float px, float py, float pz, const float* ow, float& tx, float& ty, float& tz) {
  const float dx = px - ow[0], dy = py - ow[1], dz = pz - ow[2];
  const float inv = (float)(1.0 / norm3(dx, dy, dz));
  tx = dx * inv; ty = dy * inv; tz = dz * inv;
}

// One step of the sum over a row that aligned groups of W lanes walk W entries at a time: lane l of the group holds the term of entry
// j0 + l and keep = 1, or keep = 0 for an entry that does not count (erased, or past the row's end).  Every lane of the group adds the kept
// terms in lane order: normal = normal + normali/cv::norm(normali), the same sequence of additions in every lane.
template <int W>
__device__ __forceinline__ void add_in_order(int keep, float tx, float ty, float tz, float& nx, float& ny, float& nz) {
  for (int l = 0; l < W; l++) {
    const int k = lld_wave::group_bcast<W>(keep, l);
    const float ax = lld_wave::group_bcast<W>(tx, l), ay = lld_wave::group_bcast<W>(ty, l), az = lld_wave::group_bcast<W>(tz, l);
    if (k) { nx = nx + ax; ny = ny + ay; nz = nz + az; }
  }
}

// The level of the final write: pRefKF->mvKeysUn[observations[pRefKF]].octave (:361), or -1 when the tables do not hold it.  ref is the
// reference keyframe's slot, ref_at its position in the point's row of `len` entries (>= len: it is no observer, and operator[] inserts 0),
// idx_row the keypoint indices parallel to that row.  k_oct / oct_pool: the keyframes' octave rows; k_feat: the keyframe's features were set.
__device__ __forceinline__ int ref_level(int ref, int ref_at, int len, const int32_t* idx_row, const int2* k_oct, const int32_t* oct_pool,
                                         const uint8_t* k_feat, int n_levels) {
  const int idx = ref_at < len ? idx_row[ref_at] : 0;
  const int2 orow = k_oct[ref];
  if (!k_feat[ref] || idx >= orow.y) return -1;
  const int level = oct_pool[orow.x + idx];
  return level >= 0 && level < n_levels ? level : -1;
}

struct Out { float* normal; float* min_distance; float* max_distance; };

// :359-369 from the finished sum (nx, ny, nz) of n terms; owr = the reference keyframe's centre
__device__ __forceinline__ void finish(const Out& O, int p, float px, float py, float pz, float nx, float ny, float nz, int n, const float* owr,
                                       const float* level_scale, int ref_level, int n_levels) {
  const float invn = (float)(1.0 / (double)n);                                  // normal/n (:369)
  O.normal[3 * (size_t)p] = nx * invn; O.normal[3 * (size_t)p + 1] = ny * invn; O.normal[3 * (size_t)p + 2] = nz * invn;
  const float dist = (float)norm3(px - owr[0], py - owr[1], pz - owr[2]);       // PC = Pos - pRefKF->GetCameraCenter() (:359-360)
  const float mx = dist * level_scale[ref_level];                               // (:367)
  O.max_distance[p] = mx;
  O.min_distance[p] = __fdiv_rn(mx, level_scale[n_levels - 1]);                 // (:368)
}

}  // namespace lld_nd

#endif
