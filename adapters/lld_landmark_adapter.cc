// lld_landmark_adapter.cc — see lld_landmark_adapter.h.
#include "lld_landmark_adapter.h"

#include <cstring>
#include <map>

namespace lld_adapter {

namespace {
// the keyframe table of one call: an index per keyframe in first-met order
struct KfTable {
  std::map<KeyFrame*, int32_t> index;
  std::vector<KeyFrame*> kfs;
  int32_t of(KeyFrame* pKF) {
    std::map<KeyFrame*, int32_t>::const_iterator it = index.find(pKF);
    if (it != index.end()) return it->second;
    const int32_t i = (int32_t)kfs.size();
    index[pKF] = i; kfs.push_back(pKF);
    return i;
  }
};
}  // namespace

int RefreshMapPoints(const lld_amd::Context& ctx, const std::vector<MapPoint*>& vpMapPoints, unsigned flags) {
  const size_t n = vpMapPoints.size();
  if (n == 0) return 0;
  const bool want_desc = (flags & LLD_LANDMARK_DESCRIPTOR) != 0, want_norm = (flags & LLD_LANDMARK_NORMAL_DEPTH) != 0;
  lld_amd::MapPointBatch b;
  KfTable T;
  KeyFrame* scales = nullptr;
  b.obs_start.assign(1, 0); b.bad.resize(n); b.pos.assign(3 * n, 0.f); b.ref_kf.assign(n, 0); b.ref_level.assign(n, 0);
  for (size_t i = 0; i < n; ++i) {
    MapPoint* pMP = vpMapPoints[i];
    // mbBad returns at once in both routines (:251-252, :338-339); an entry the caller left empty is treated alike
    b.bad[i] = (!pMP || pMP->isBad() || (want_norm && !pMP->mpRefKF)) ? 1 : 0;
    if (!b.bad[i]) {
      std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
      for (std::map<KeyFrame*, size_t>::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
        KeyFrame* pKF = mit->first;
        b.obs_kf.push_back(T.of(pKF));
        if (want_desc) {
          const uint32_t* row = pKF->mDescriptors.ptr<uint32_t>((int)mit->second);   // pKF->mDescriptors.row(mit->second) (:266)
          b.obs_desc.insert(b.obs_desc.end(), row, row + 8);
        }
      }
      if (want_norm && !observations.empty()) {
        KeyFrame* pRefKF = pMP->mpRefKF;
        const float* P = pMP->mWorldPos.ptr<float>();
        b.pos[3 * i] = P[0]; b.pos[3 * i + 1] = P[1]; b.pos[3 * i + 2] = P[2];
        b.ref_kf[i] = T.of(pRefKF);
        b.ref_level[i] = pRefKF->mvKeysUn[observations[pRefKF]].octave;   // operator[]: an absent pRefKF yields keypoint 0 (:361)
        if (!scales) scales = pRefKF;
      }
    }
    b.obs_start.push_back((int32_t)b.obs_kf.size());
  }
  b.kf_bad.resize(T.kfs.size()); b.kf_ow.resize(3 * T.kfs.size());
  for (size_t k = 0; k < T.kfs.size(); ++k) {
    b.kf_bad[k] = T.kfs[k]->isBad() ? 1 : 0;
    const lld_slam::Mat Ow = T.kfs[k]->GetCameraCenter();
    for (int r = 0; r < 3; ++r) b.kf_ow[3 * k + r] = Ow.empty() ? 0.f : Ow.at<float>(r);
  }
  if (scales) b.level_scale.assign(scales->mvScaleFactors.begin(), scales->mvScaleFactors.begin() + scales->mnScaleLevels);
  else b.level_scale.assign(1, 1.f);          // nothing reads it: every point is skipped
  lld_amd::MapPointRefreshOutput o;
  lld_amd::MapPointRefresh(ctx, b, flags, o);
  int written = 0;
  for (size_t i = 0; i < n; ++i) {
    MapPoint* pMP = vpMapPoints[i];
    if (!o.updated[i]) continue;
    written++;
    if (o.updated[i] & LLD_LANDMARK_DESCRIPTOR) {             // mDescriptor = vDescriptors[BestIdx].clone() (:305)
      lld_slam::MatU8 d(1, 32);
      std::memcpy(d.ptr<unsigned char>(), &o.desc[8 * i], 32);
      pMP->mDescriptor = d;
    }
    if (o.updated[i] & LLD_LANDMARK_NORMAL_DEPTH) {           // :367-369
      pMP->mfMaxDistance = o.max_distance[i];
      pMP->mfMinDistance = o.min_distance[i];
      pMP->mNormalVector = lld_slam::Mat(3, 1, &o.normal[3 * i]);
    }
  }
  return written;
}

int ComputeDistinctiveDescriptors(const lld_amd::Context& ctx, const std::vector<MapLine*>& vpMapLines) {
  const size_t n = vpMapLines.size();
  if (n == 0) return 0;
  lld_amd::MapLineBatch b;
  KfTable T;
  b.dim = 0;
  b.obs_start.assign(1, 0); b.bad.resize(n);
  for (size_t i = 0; i < n; ++i) {
    MapLine* pML = vpMapLines[i];
    b.bad[i] = (!pML || pML->isBad()) ? 1 : 0;
    if (!b.bad[i]) {
      const std::map<KeyFrame*, size_t> observations = pML->GetObservations();
      for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
        KeyFrame* pKF = mit->first;
        if (b.dim == 0) b.dim = pKF->mDescriptorsLines.cols;
        b.obs_kf.push_back(T.of(pKF));
        const float* row = pKF->mDescriptorsLines.ptr<float>((int)mit->second);   // pKF->mDescriptorsLines.row(mit->second) (:159)
        b.obs_desc.insert(b.obs_desc.end(), row, row + b.dim);
      }
    }
    b.obs_start.push_back((int32_t)b.obs_kf.size());
  }
  if (b.dim == 0) return 0;                    // no observation anywhere: every line returns early
  b.kf_bad.resize(T.kfs.size());
  for (size_t k = 0; k < T.kfs.size(); ++k) b.kf_bad[k] = T.kfs[k]->isBad() ? 1 : 0;
  lld_amd::MapLineDistinctiveOutput o;
  lld_amd::MapLineDistinctive(ctx, b, o);
  int written = 0;
  for (size_t i = 0; i < n; ++i) {
    if (!o.updated[i]) continue;
    written++;
    vpMapLines[i]->mDescriptor = lld_slam::Mat(1, b.dim, &o.desc[(size_t)b.dim * i]);   // mDescriptor = vDescriptors[BestIdx].clone() (:199)
  }
  return written;
}

}  // namespace lld_adapter
