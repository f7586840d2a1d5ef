// lld_map_adapter.cc — see lld_map_adapter.h.  Each Update* gathers the listed objects' rows into flat arrays and makes one lld_map_set_* call
// (two for MapPoints: the fixed rows and the observation rows).
#include "lld_map_adapter.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>

namespace lld_adapter {

using lld_slam::KeyFrame;
using lld_slam::MapLine;
using lld_slam::MapPoint;

namespace {
void check(int status, const char* what) {
  if (status != LLD_OK) throw std::runtime_error(std::string(what) + ": " + lld_status_string(status));
}
// the slot of an object that a row names: its mnId when it fits the table, else -1 (the row then holds no object there)
template <class T> int32_t slot_of(const T* p, int32_t limit) { return (p && (int64_t)p->mnId < (int64_t)limit) ? (int32_t)p->mnId : -1; }
template <class T> void remember(std::vector<T*>& table, T* p, int32_t limit, const char* what) {
  if ((int64_t)p->mnId >= (int64_t)limit) throw std::runtime_error(std::string(what) + ": mnId beyond the map's limit");
  table[p->mnId] = p;
}
}  // namespace

MapOnDevice::MapOnDevice(lld_ctx* ctx, const lld_map_limits& limits) : limits_(limits) {
  check(lld_map_create(ctx, &limits, &m_), "lld_map_create");
  kf_.assign(limits.max_keyframes, nullptr); pt_.assign(limits.max_points, nullptr); ln_.assign(limits.max_lines > 0 ? limits.max_lines : 0, nullptr);
}

MapOnDevice::~MapOnDevice() { if (m_) lld_map_destroy(m_); }

void MapOnDevice::Upload(lld_slam::Map* pMap) {
  check(lld_map_clear(m_), "lld_map_clear");
  std::fill(kf_.begin(), kf_.end(), nullptr); std::fill(pt_.begin(), pt_.end(), nullptr); std::fill(ln_.begin(), ln_.end(), nullptr);
  UpdateKeyFrames(pMap->GetAllKeyFrames());
  UpdatePoints(pMap->GetAllMapPoints());
  UpdateLines(pMap->GetAllMapLines());
}

void MapOnDevice::UpdatePoints(const std::vector<MapPoint*>& points) {
  const size_t n = points.size();
  if (!n) return;
  std::vector<int32_t> slot(n), start(1, 0), obs, idx, nobs(n); std::vector<float> pos(3 * n), nrm(3 * n), mind(n), maxd(n); std::vector<uint32_t> desc(8 * n, 0u); std::vector<uint8_t> bad(n);
  for (size_t i = 0; i < n; i++) {
    MapPoint* pMP = points[i];
    remember(pt_, pMP, limits_.max_points, "MapOnDevice::UpdatePoints");
    slot[i] = (int32_t)pMP->mnId; bad[i] = pMP->isBad();
    const lld_slam::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal();
    for (int k = 0; k < 3; k++) { pos[3 * i + k] = P.at<float>(k); nrm[3 * i + k] = Pn.empty() ? 0.f : Pn.at<float>(k); }
    mind[i] = pMP->GetMinDistance(); maxd[i] = pMP->GetMaxDistance();          // as lld_map_points takes them (FrameOnDevice::TrackLocalMap's gather)
    const lld_slam::MatU8 d = pMP->GetDescriptor();
    if (!d.empty()) std::memcpy(&desc[8 * i], d.ptr<unsigned char>(), 32);
    const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
    for (std::map<KeyFrame*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it) {
      const int32_t s = slot_of(it->first, limits_.max_keyframes);
      if (s >= 0) { obs.push_back(s); idx.push_back((int32_t)it->second); }
    }
    start.push_back((int32_t)obs.size());
    nobs[i] = pMP->Observations();
  }
  obs.push_back(0); idx.push_back(0);                                          // (never read: a non-null pointer for an empty list)
  check(lld_map_set_points(m_, (int32_t)n, slot.data(), pos.data(), nrm.data(), mind.data(), maxd.data(), desc.data(), bad.data()), "lld_map_set_points");
  if (covis_) check(lld_map_set_observations_indexed(m_, (int32_t)n, slot.data(), start.data(), obs.data(), idx.data(), nobs.data()), "lld_map_set_observations_indexed");
  else check(lld_map_set_observations(m_, (int32_t)n, slot.data(), start.data(), obs.data()), "lld_map_set_observations");
  if (!refresh_) return;
  std::vector<int32_t> ref(n);
  for (size_t i = 0; i < n; i++) ref[i] = slot_of(points[i]->mpRefKF, limits_.max_keyframes);       // -1: none, or one the table cannot hold
  check(lld_map_set_point_refs(m_, (int32_t)n, slot.data(), ref.data()), "lld_map_set_point_refs");
}

int MapOnDevice::RefreshMapPoints(const std::vector<MapPoint*>& vpMapPoints, unsigned flags) {
  if (!refresh_) throw std::runtime_error("MapOnDevice::RefreshMapPoints: EnableRefresh before Upload");
  std::vector<MapPoint*> pts; std::vector<int32_t> slots;
  const KeyFrame* scales = nullptr;
  for (size_t i = 0; i < vpMapPoints.size(); i++) {
    MapPoint* pMP = vpMapPoints[i];
    if (!pMP) continue;
    if (PointOf(slot_of(pMP, limits_.max_points)) != pMP) throw std::runtime_error("MapOnDevice::RefreshMapPoints: a point the map does not hold");
    pts.push_back(pMP); slots.push_back((int32_t)pMP->mnId);
    if (!scales && !pMP->isBad() && pMP->mpRefKF) scales = pMP->mpRefKF;
  }
  const size_t n = pts.size();
  if (!n) return 0;
  std::vector<float> level_scale(1, 1.f);                               // (read only when some point has a reference keyframe)
  if (scales) level_scale.assign(scales->mvScaleFactors.begin(), scales->mvScaleFactors.begin() + scales->mnScaleLevels);
  lld_map_refresh_points_in in; std::memset(&in, 0, sizeof in);
  in.n = (int32_t)n; in.flags = flags; in.n_levels = (int32_t)level_scale.size(); in.slot = slots.data(); in.level_scale = level_scale.data();
  std::vector<uint32_t> desc(8 * n); std::vector<float> nrm(3 * n), mind(n), maxd(n); std::vector<uint8_t> upd(n);
  lld_map_refresh_points_out out; std::memset(&out, 0, sizeof out);
  out.desc = desc.data(); out.normal = nrm.data(); out.min_distance = mind.data(); out.max_distance = maxd.data(); out.updated = upd.data();
  check(lld_map_refresh_points(m_, &in, &out), "lld_map_refresh_points");
  int written = 0;
  for (size_t i = 0; i < n; i++) {
    if (!(upd[i] & (LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH))) continue;
    written++;
    if (upd[i] & LLD_LANDMARK_DESCRIPTOR) {                             // mDescriptor = vDescriptors[BestIdx].clone() (MapPoint.cc:305)
      lld_slam::MatU8 d(1, 32);
      std::memcpy(d.ptr<unsigned char>(), &desc[8 * i], 32);
      pts[i]->mDescriptor = d;
    }
    if (upd[i] & LLD_LANDMARK_NORMAL_DEPTH) {                           // :367-369
      pts[i]->mfMaxDistance = maxd[i]; pts[i]->mfMinDistance = mind[i];
      pts[i]->mNormalVector = lld_slam::Mat(3, 1, &nrm[3 * i]);
    }
  }
  return written;
}

int MapOnDevice::ComputeDistinctiveDescriptors(const std::vector<MapLine*>& vpMapLines) {
  if (!refresh_) throw std::runtime_error("MapOnDevice::ComputeDistinctiveDescriptors: EnableRefresh before Upload");
  std::vector<MapLine*> lns; std::vector<int32_t> slots;
  for (size_t i = 0; i < vpMapLines.size(); i++) {
    MapLine* pML = vpMapLines[i];
    if (!pML) continue;
    if (LineOf(slot_of(pML, limits_.max_lines)) != pML) throw std::runtime_error("MapOnDevice::ComputeDistinctiveDescriptors: a line the map does not hold");
    lns.push_back(pML); slots.push_back((int32_t)pML->mnId);
  }
  const size_t n = lns.size(), dim = limits_.line_dim;
  if (!n) return 0;
  lld_map_refresh_lines_in in; std::memset(&in, 0, sizeof in);
  in.n = (int32_t)n; in.slot = slots.data();
  std::vector<float> desc(dim * n); std::vector<uint8_t> upd(n);
  lld_map_refresh_lines_out out; std::memset(&out, 0, sizeof out);
  out.desc = desc.data(); out.updated = upd.data();
  check(lld_map_refresh_lines(m_, &in, &out), "lld_map_refresh_lines");
  int written = 0;
  for (size_t i = 0; i < n; i++) {
    if (!(upd[i] & LLD_LANDMARK_DESCRIPTOR)) continue;
    written++;
    lns[i]->mDescriptor = lld_slam::Mat(1, (int)dim, &desc[dim * i]);   // mDescriptor = vDescriptors[BestIdx].clone() (MapLine.cc:199)
  }
  return written;
}

int MapOnDevice::Fuse(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, float th, KeyFrame* pSourceKF) {
  if (!refresh_) throw std::runtime_error("MapOnDevice::Fuse: EnableRefresh before Upload");
  if (KeyFrameOf(slot_of(pKF, limits_.max_keyframes)) != pKF) throw std::runtime_error("MapOnDevice::Fuse: a keyframe the map does not hold");
  const size_t n = vpMapPoints.size();
  if (!n) return 0;
  std::vector<int32_t> slots(n, -1);
  for (size_t i = 0; i < n; i++) {
    MapPoint* pMP = vpMapPoints[i];
    if (!pMP) continue;
    if (PointOf(slot_of(pMP, limits_.max_points)) != pMP) throw std::runtime_error("MapOnDevice::Fuse: a point the map does not hold");
    slots[i] = (int32_t)pMP->mnId;
  }
  lld_map_fuse_in in; std::memset(&in, 0, sizeof in);
  in.target = (int32_t)pKF->mnId; in.n_points = (int32_t)n; in.th = th;
  in.point_slot = pSourceKF ? nullptr : slots.data(); in.source_keyframe = pSourceKF ? slot_of(pSourceKF, limits_.max_keyframes) : -1;
  const lld_slam::Mat Rcw = pKF->GetRotation(), tcw = pKF->GetTranslation(), Ow = pKF->GetCameraCenter();
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) in.view.Rcw[3 * r + c] = Rcw.at<float>(r, c);
    in.view.tcw[r] = tcw.at<float>(r); in.view.Ow[r] = Ow.at<float>(r);
  }
  in.view.fx = pKF->fx; in.view.fy = pKF->fy; in.view.cx = pKF->cx; in.view.cy = pKF->cy; in.view.bf = pKF->mbf;
  in.view.min_x = (float)pKF->mnMinX; in.view.max_x = (float)pKF->mnMaxX; in.view.min_y = (float)pKF->mnMinY; in.view.max_y = (float)pKF->mnMaxY;
  in.view.log_scale_factor = pKF->mfLogScaleFactor; in.view.n_levels = pKF->mnScaleLevels;
  in.grid_min_x = (float)pKF->mnMinX; in.grid_min_y = (float)pKF->mnMinY; in.grid_width_inv = pKF->mfGridElementWidthInv; in.grid_height_inv = pKF->mfGridElementHeightInv;
  in.grid_cols = 64; in.grid_rows = 48;                                  // FRAME_GRID_COLS, FRAME_GRID_ROWS (Frame.h:43-44)
  in.n_levels = pKF->mnScaleLevels; in.level_scale = pKF->mvScaleFactors.data(); in.level_inv_sigma2 = pKF->mvInvLevelSigma2.data();
  std::vector<int32_t> match(n), other(n), surv(n); std::vector<uint8_t> action(n);
  lld_map_fuse_out out; std::memset(&out, 0, sizeof out);
  out.match = match.data(); out.action = action.data(); out.other = other.data(); out.survivor = surv.data(); out.survivor_capacity = (int32_t)n;
  check(lld_map_fuse(m_, &in, &out), "lld_map_fuse");
  // the objects follow, in list order (src/ORBmatcher.cc:934-954)
  for (size_t i = 0; i < n; i++) {
    MapPoint* pMP = vpMapPoints[i];
    switch (action[i]) {
      case LLD_MAP_FUSE_ADDED: pMP->AddObservation(pKF, (size_t)match[i]); pKF->AddMapPoint(pMP, (size_t)match[i]); break;
      case LLD_MAP_FUSE_CANDIDATE_REPLACED: pMP->Replace(PointOf(other[i])); break;
      case LLD_MAP_FUSE_HOLDER_REPLACED: PointOf(other[i])->Replace(pMP); break;
      default: break;
    }
  }
  if (out.n_survivors > 0) {                                             // ComputeDistinctiveDescriptors of MapPoint::Replace (MapPoint.cc:212): the map holds it
    std::vector<uint32_t> desc(8 * (size_t)out.n_survivors);
    check(lld_map_download_points(m_, out.n_survivors, surv.data(), nullptr, nullptr, nullptr, nullptr, desc.data(), nullptr), "lld_map_download_points");
    for (int32_t k = 0; k < out.n_survivors; k++) {
      lld_slam::MatU8 d(1, 32);
      std::memcpy(d.ptr<unsigned char>(), &desc[8 * (size_t)k], 32);
      PointOf(surv[k])->mDescriptor = d;
    }
  }
  return out.n_fused;
}

int MapOnDevice::SearchInNeighbors(KeyFrame* pKF) {
  const std::vector<KeyFrame*> vpNeighKFs = pKF->GetBestCovisibilityKeyFrames(10);
  std::vector<KeyFrame*> vpTargetKFs;
  for (size_t i = 0; i < vpNeighKFs.size(); i++) {                        // :463-480
    KeyFrame* pKFi = vpNeighKFs[i];
    if (pKFi->isBad() || pKFi->mnFuseTargetForKF == pKF->mnId) continue;
    vpTargetKFs.push_back(pKFi);
    pKFi->mnFuseTargetForKF = pKF->mnId;
    const std::vector<KeyFrame*> vpSecondNeighKFs = pKFi->GetBestCovisibilityKeyFrames(5);
    for (size_t j = 0; j < vpSecondNeighKFs.size(); j++) {
      KeyFrame* pKFi2 = vpSecondNeighKFs[j];
      if (pKFi2->isBad() || pKFi2->mnFuseTargetForKF == pKF->mnId || pKFi2->mnId == pKF->mnId) continue;
      vpTargetKFs.push_back(pKFi2);
    }
  }
  int n = 0;
  std::vector<MapPoint*> vpMapPointMatches = pKF->GetMapPointMatches();
  for (size_t i = 0; i < vpTargetKFs.size(); i++) n += Fuse(vpTargetKFs[i], vpMapPointMatches, 3.0f, i == 0 ? pKF : nullptr);      // :486-491
  std::vector<MapPoint*> vpFuseCandidates;                               // :494-513
  for (size_t i = 0; i < vpTargetKFs.size(); i++) {
    const std::vector<MapPoint*> vpMapPointsKFi = vpTargetKFs[i]->GetMapPointMatches();
    for (size_t j = 0; j < vpMapPointsKFi.size(); j++) {
      MapPoint* pMP = vpMapPointsKFi[j];
      if (!pMP || pMP->isBad() || pMP->mnFuseCandidateForKF == pKF->mnId) continue;
      pMP->mnFuseCandidateForKF = pKF->mnId;
      vpFuseCandidates.push_back(pMP);
    }
  }
  n += Fuse(pKF, vpFuseCandidates, 3.0f);                                // :515
  vpMapPointMatches = pKF->GetMapPointMatches();                         // :519-531
  std::vector<MapPoint*> live;
  for (size_t i = 0; i < vpMapPointMatches.size(); i++)
    if (vpMapPointMatches[i] && !vpMapPointMatches[i]->isBad() && std::find(live.begin(), live.end(), vpMapPointMatches[i]) == live.end()) live.push_back(vpMapPointMatches[i]);
  RefreshMapPoints(live, LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH);
  UpdateConnections(std::vector<KeyFrame*>(1, pKF));                     // :534
  return n;
}

void MapOnDevice::UpdateKeyFrames(const std::vector<KeyFrame*>& keyframes) {
  const size_t n = keyframes.size();
  if (!n) return;
  std::vector<int32_t> slot(n), parent(n), cs(1, 0), cv, hs(1, 0), hv, ps(1, 0), pv, ls(1, 0), lv; std::vector<uint64_t> key(n); std::vector<uint8_t> bad(n);
  for (size_t i = 0; i < n; i++) {
    KeyFrame* pKF = keyframes[i];
    remember(kf_, pKF, limits_.max_keyframes, "MapOnDevice::UpdateKeyFrames");
    slot[i] = (int32_t)pKF->mnId; key[i] = (uint64_t)reinterpret_cast<uintptr_t>(pKF); bad[i] = pKF->isBad();
    parent[i] = slot_of(pKF->GetParent(), limits_.max_keyframes);
    const std::vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
    for (size_t j = 0; j < vNeighs.size(); j++) { const int32_t s = slot_of(vNeighs[j], limits_.max_keyframes); if (s >= 0) cv.push_back(s); }
    cs.push_back((int32_t)cv.size());
    const std::set<KeyFrame*> spChilds = pKF->GetChilds();
    for (std::set<KeyFrame*>::const_iterator it = spChilds.begin(); it != spChilds.end(); ++it) { const int32_t s = slot_of(*it, limits_.max_keyframes); if (s >= 0) hv.push_back(s); }
    hs.push_back((int32_t)hv.size());
    const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
    for (size_t j = 0; j < vpMPs.size(); j++) pv.push_back(slot_of(vpMPs[j], limits_.max_points));
    ps.push_back((int32_t)pv.size());
    const std::vector<MapLine*> vpMLs = pKF->GetMapLineMatches();
    for (size_t j = 0; j < vpMLs.size(); j++) lv.push_back(slot_of(vpMLs[j], limits_.max_lines));
    ls.push_back((int32_t)lv.size());
  }
  cv.push_back(0); hv.push_back(0); pv.push_back(-1); lv.push_back(-1);       // (never read: non-null pointers for empty lists)
  check(lld_map_set_keyframes(m_, (int32_t)n, slot.data(), key.data(), bad.data(), parent.data(), cs.data(), cv.data(), hs.data(), hv.data(), ps.data(), pv.data(),
                              ls.data(), lv.data()), "lld_map_set_keyframes");
  if (!covis_) return;
  // one octave and one depth per entry of the point row just sent
  std::vector<int32_t> oct; std::vector<float> dep, thd(n);
  for (size_t i = 0; i < n; i++) {
    const KeyFrame* pKF = keyframes[i];
    for (int32_t j = 0; j < ps[i + 1] - ps[i]; j++) {
      oct.push_back((size_t)j < pKF->mvKeysUn.size() ? pKF->mvKeysUn[j].octave : 0);
      dep.push_back((size_t)j < pKF->mvDepth.size() ? pKF->mvDepth[j] : -1.f);
    }
    thd[i] = pKF->mThDepth;
  }
  oct.push_back(0); dep.push_back(0.f);
  check(lld_map_set_keyframe_keypoints(m_, (int32_t)n, slot.data(), ps.data(), oct.data(), dep.data(), thd.data()), "lld_map_set_keyframe_keypoints");
  if (!ba_) return;
  // mnId, pose, and one (u, v, uR) per entry of the point row, one keyline with its stereo partner per entry of the line row
  std::vector<uint64_t> id(n); std::vector<float> Tcw(16 * n), uvr, left, right; std::vector<int32_t> loct;
  for (size_t i = 0; i < n; i++) {
    const KeyFrame* pKF = keyframes[i];
    id[i] = pKF->mnId;
    const lld_slam::Mat T = pKF->GetPose();
    std::memcpy(&Tcw[16 * i], T.ptr<float>(), 64);
    for (int32_t j = 0; j < ps[i + 1] - ps[i]; j++) {
      const bool has = (size_t)j < pKF->mvKeysUn.size();
      uvr.push_back(has ? pKF->mvKeysUn[j].pt.x : 0.f); uvr.push_back(has ? pKF->mvKeysUn[j].pt.y : 0.f);
      uvr.push_back((size_t)j < pKF->mvuRight.size() ? pKF->mvuRight[j] : -1.f);
    }
    for (int32_t j = 0; j < ls[i + 1] - ls[i]; j++) {
      const bool has = (size_t)j < pKF->mvLinesLeft.size();
      const lld_slam::KeyLine kl = has ? pKF->mvLinesLeft[j] : lld_slam::KeyLine();
      left.push_back(kl.startPointX); left.push_back(kl.startPointY); left.push_back(kl.endPointX); left.push_back(kl.endPointY);
      const int match = has && (size_t)j < pKF->line_matches.size() ? pKF->line_matches[j] : -1;
      if (match >= 0) {
        const lld_slam::KeyLine& kr = pKF->mvLinesRight[match];
        right.push_back(kr.startPointX); right.push_back(kr.startPointY); right.push_back(kr.endPointX); right.push_back(kr.endPointY);
        loct.push_back(kl.octave); loct.push_back(kr.octave);
      } else {
        for (int k = 0; k < 4; k++) right.push_back(-1.f);                      // kl_empty (Optimizer.cc:1203-1209)
        loct.push_back(kl.octave); loct.push_back(0);
      }
    }
  }
  uvr.push_back(0.f); left.push_back(0.f); right.push_back(0.f); loct.push_back(0);
  check(lld_map_set_keyframe_features(m_, (int32_t)n, slot.data(), id.data(), Tcw.data(), ps.data(), uvr.data(), ls.data(), left.data(), right.data(), loct.data()),
        "lld_map_set_keyframe_features");
  if (!refresh_) return;
  // mDescriptors.row(j) per entry of the point row, mDescriptorsLines.row(j) per entry of the line row (zeros where the keyframe has no such row)
  const size_t dim = limits_.line_dim;
  std::vector<uint32_t> kd(8 * (size_t)ps[n] + 1, 0u); std::vector<float> kl(dim * (size_t)ls[n] + 1, 0.f);
  for (size_t i = 0; i < n; i++) {
    const KeyFrame* pKF = keyframes[i];
    for (int32_t j = 0; j < ps[i + 1] - ps[i] && j < pKF->mDescriptors.rows; j++) std::memcpy(&kd[8 * (size_t)(ps[i] + j)], pKF->mDescriptors.ptr<unsigned char>(j), 32);
    if (pKF->mDescriptorsLines.rows > 0 && (size_t)pKF->mDescriptorsLines.cols != dim)
      throw std::runtime_error("MapOnDevice::UpdateKeyFrames: line descriptors of another length than line_dim");
    for (int32_t j = 0; j < ls[i + 1] - ls[i] && j < pKF->mDescriptorsLines.rows; j++) std::memcpy(&kl[dim * (size_t)(ls[i] + j)], pKF->mDescriptorsLines.ptr<float>(j), dim * 4);
  }
  check(lld_map_set_keyframe_descriptors(m_, (int32_t)n, slot.data(), ps.data(), kd.data()), "lld_map_set_keyframe_descriptors");
  check(lld_map_set_keyframe_line_descriptors(m_, (int32_t)n, slot.data(), ls.data(), kl.data()), "lld_map_set_keyframe_line_descriptors");
}

void MapOnDevice::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, lld_slam::Map* pMap, double gamma, LbaTrace* trace) {
  LbaTrace local_trace;
  LbaTrace& tr = trace ? *trace : local_trace;
  tr = LbaTrace();
  if (!ba_) throw std::runtime_error("MapOnDevice::LocalBundleAdjustment: EnableBundleAdjustment before Upload");
  // ---- :938-950  the list that travels: pKF, then its covisible keyframes in their order
  const std::vector<KeyFrame*> vNeighKFs = pKF->GetVectorCovisibleKeyFrames();
  std::vector<int32_t> slots(1, slot_of(pKF, limits_.max_keyframes));
  pKF->mnBALocalForKF = pKF->mnId;
  for (size_t i = 0; i < vNeighKFs.size(); i++) { vNeighKFs[i]->mnBALocalForKF = pKF->mnId; slots.push_back(slot_of(vNeighKFs[i], limits_.max_keyframes)); }
  for (size_t i = 0; i < slots.size(); i++)
    if (KeyFrameOf(slots[i]) != (i ? vNeighKFs[i - 1] : pKF)) throw std::runtime_error("MapOnDevice::LocalBundleAdjustment: a keyframe the map does not hold");
  lld_ba_params p; lld_ba_params_default(&p); p.gamma = gamma;
  // ---- :953-1329  window, graph, optimize(5), classification, optimize(15): one call
  const lld_amd::DeviceMap::LocalBaResult solved = lld_amd::DeviceMap::LocalBaOn(m_, slots, lld_camera{pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf}, pKF->mvInvLevelSigma2, &p, pbStopFlag);
  const lld_ba_result& res = solved.result; const lld_map_ba_ids& ids = solved.ids;
  if (ids.status) throw std::runtime_error("MapOnDevice::LocalBundleAdjustment: the map lacks feature data (EnableBundleAdjustment before Upload)");
  const lld_ba_window& w = ids.window;
  std::vector<KeyFrame*>& cams = tr.cams;
  for (int32_t c = 0; c < w.n_cams; c++) cams.push_back(kf_[ids.cam_slot[c]]);
  for (int32_t k = 0; k < w.n_points; k++) { tr.points.push_back(pt_[ids.point_slot[k]]); tr.points.back()->mnBALocalForKF = pKF->mnId; }
  for (int32_t k = 0; k < w.n_lines; k++) { tr.lines.push_back(ln_[ids.line_slot[k]]); tr.lines.back()->mnBALocalForKF = pKF->mnId; }
  for (int32_t c = ids.n_local_cams; c < w.n_cams; c++) cams[c]->mnBAFixedForKF = pKF->mnId;
  for (int32_t k = 0; k < ids.n_marked_bad; k++) if (KeyFrame* kf = KeyFrameOf(ids.marked_bad_slot[k])) kf->mnBAFixedForKF = pKF->mnId;   // marked, never a camera
  for (int32_t k = 0; k < w.n_points; k++)
    for (int32_t e = w.pt_obs_start[k]; e < w.pt_obs_start[k + 1]; e++) tr.pt_obs_owner.push_back(std::make_pair(cams[w.pt_obs_cam[e]], tr.points[k]));
  for (int32_t k = 0; k < w.n_lines; k++)
    for (int32_t e = w.ln_obs_start[k]; e < w.ln_obs_start[k + 1]; e++) tr.ln_obs_owner.push_back(std::make_pair(cams[w.ln_obs_cam[e]], tr.lines[k]));
  if (trace) {
    lld_amd::BAWindow& g = tr.window; lld_amd::BAOutput& o = tr.output;
    const size_t nc = w.n_cams, np = w.n_points, npo = w.n_pt_obs, nl = w.n_lines, nlo = w.n_ln_obs;
    g.cam = w.cam; g.n_free_cams = w.n_free_cams;
    g.cam_qt.assign(w.cam_qt, w.cam_qt + 7 * nc); g.pt_xyz.assign(w.pt_xyz, w.pt_xyz + 3 * np); g.pt_obs_start.assign(w.pt_obs_start, w.pt_obs_start + np + 1);
    g.pt_obs_cam.assign(w.pt_obs_cam, w.pt_obs_cam + npo); g.pt_obs_uvr.assign(w.pt_obs_uvr, w.pt_obs_uvr + 3 * npo);
    g.pt_obs_inv_sigma2.assign(w.pt_obs_inv_sigma2, w.pt_obs_inv_sigma2 + npo);
    g.line_x0.assign(w.line_x0, w.line_x0 + 3 * nl); g.line_dir.assign(w.line_dir, w.line_dir + 3 * nl); g.ln_obs_start.assign(w.ln_obs_start, w.ln_obs_start + nl + 1);
    g.ln_obs_cam.assign(w.ln_obs_cam, w.ln_obs_cam + nlo); g.ln_obs_left.assign(w.ln_obs_left, w.ln_obs_left + 4 * nlo);
    g.ln_obs_right.assign(w.ln_obs_right, w.ln_obs_right + 4 * nlo); g.ln_obs_octave.assign(w.ln_obs_octave, w.ln_obs_octave + 2 * nlo);
    o.cam_qt.assign(res.cam_qt, res.cam_qt + 7 * nc); o.pt_xyz.assign(res.pt_xyz, res.pt_xyz + 3 * np); o.line_x0.assign(res.line_x0, res.line_x0 + 3 * nl);
    o.line_dir.assign(res.line_dir, res.line_dir + 3 * nl); o.pt_obs_outlier.assign(res.pt_obs_outlier, res.pt_obs_outlier + npo);
    o.ln_edge_outlier.assign(res.ln_edge_outlier, res.ln_edge_outlier + 2 * nlo); o.line_removed.assign(res.line_removed, res.line_removed + nl);
  }
  tr.output.stats = res.stats;
  tr.solved = true;
  if (res.stats.aborted && res.stats.lm_iterations[0] == 0 && res.stats.lm_trials[0] == 0) {      // :1220-1222 return before optimising: the map is not touched
    tr.returned_before_optimising = true;
    return;
  }
  // ---- :1278-1329  erase lists
  for (size_t k = 0; k < tr.pt_obs_owner.size(); k++) if (res.pt_obs_outlier[k]) tr.vToErase.push_back(tr.pt_obs_owner[k]);
  for (size_t k = 0; k < tr.ln_obs_owner.size(); k++)
    for (int si = 0; si < 2; si++) if (res.ln_edge_outlier[2 * k + si]) tr.vToEraseLines.push_back(tr.ln_obs_owner[k]);   // once per outlier edge
  std::set<KeyFrame*> lost;                                             // keyframes whose match rows change
  {
    // ---- :1334-1386  write-back under the map mutex
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (size_t i = 0; i < tr.vToErase.size(); i++) {
      KeyFrame* pKFi = tr.vToErase[i].first; MapPoint* pMPi = tr.vToErase[i].second;
      pKFi->EraseMapPointMatch(pMPi);
      pMPi->EraseObservation(pKFi);
      lost.insert(pKFi);
    }
    for (size_t i = 0; i < tr.vToEraseLines.size(); i++) {
      KeyFrame* pKFi = tr.vToEraseLines[i].first; MapLine* pMLi = tr.vToEraseLines[i].second;
      pKFi->EraseMapLineMatch(pMLi);
      pMLi->EraseObservation(pKFi);
      lost.insert(pKFi);
    }
    for (int32_t c = 0; c < ids.n_local_cams; c++) {                   // every local keyframe, the fixed mnId == 0 one included
      float T[16];
      lld_se3_to_tcw_f32(res.cam_qt + 7 * (size_t)c, T);
      cams[c]->SetPose(lld_slam::Mat(4, 4, T));
    }
    for (size_t k = 0; k < tr.points.size(); k++) {
      lld_slam::Mat X(3, 1);
      for (int c = 0; c < 3; c++) X.at<float>(c) = (float)res.pt_xyz[3 * k + c];
      tr.points[k]->SetWorldPos(X);
      tr.points[k]->UpdateNormalAndDepth();
    }
    for (size_t k = 0; k < tr.lines.size(); k++) {
      if (res.line_removed[k]) continue;
      tr.lines[k]->SetMinimalPos(lld_slam::Vector3d(res.line_x0[3 * k], res.line_x0[3 * k + 1], res.line_x0[3 * k + 2]),
                                 lld_slam::Vector3d(res.line_dir[3 * k], res.line_dir[3 * k + 1], res.line_dir[3 * k + 2]));
    }
  }
  // ---- the map follows the objects (res and ids are not read beyond this point: the setters do not touch them, but nothing needs them)
  // This push-back re-sends every window point's whole row although only a position and a normal moved.  lld_map_ba_apply does the loops
  // above on the device's tables and needs no push-back, but this adapter stays on the setters: the object doubles of lld_slam_objects.h
  // do not model nObs, SetBadFlag's cascade or UpdateNormalAndDepth, so the objects could not follow what the device decides.  Making
  // them do so changes what the doubles compute and belongs in a change of its own.
  const int32_t n_local = ids.n_local_cams;
  std::vector<KeyFrame*> rows(lost.begin(), lost.end());
  std::vector<int32_t> pose_slot; std::vector<float> pose;
  for (int32_t c = 0; c < n_local; c++) {
    if (lost.count(cams[c])) continue;                                  // its whole row travels below, the pose with it
    pose_slot.push_back((int32_t)cams[c]->mnId);
    const lld_slam::Mat T = cams[c]->GetPose();
    pose.insert(pose.end(), T.ptr<float>(), T.ptr<float>() + 16);
  }
  UpdateKeyFrames(rows);
  if (!pose_slot.empty()) check(lld_map_set_keyframe_poses(m_, (int32_t)pose_slot.size(), pose_slot.data(), pose.data()), "lld_map_set_keyframe_poses");
  UpdatePoints(tr.points);
  UpdateLines(tr.lines);
}

void MapOnDevice::SetCovisibles(const std::vector<KeyFrame*>& keyframes) {
  const size_t n = keyframes.size();
  if (!n) return;
  std::vector<int32_t> slot(n), cs(1, 0), cv;
  for (size_t i = 0; i < n; i++) {
    slot[i] = (int32_t)keyframes[i]->mnId;
    const std::vector<KeyFrame*> vNeighs = keyframes[i]->GetBestCovisibilityKeyFrames(10);
    for (size_t j = 0; j < vNeighs.size(); j++) { const int32_t s = slot_of(vNeighs[j], limits_.max_keyframes); if (s >= 0) cv.push_back(s); }
    cs.push_back((int32_t)cv.size());
  }
  cv.push_back(0);
  check(lld_map_set_covisibles(m_, (int32_t)n, slot.data(), cs.data(), cv.data()), "lld_map_set_covisibles");
}

namespace {
// One lld_map_covisibility call with lists that hold the totals: a guess first, then what the library reports.
struct CovisResult {
  std::vector<int32_t> conn_start, conn_kf, conn_weight, ordered_start, ordered_kf, ordered_weight, n_max, kf_max, n_mps, n_redundant;
  std::vector<uint8_t> updated, redundant, status;
};
void covisibility(lld_map* m, const std::vector<int32_t>& slots, uint32_t flags, bool monocular, CovisResult& r) {
  const size_t nq = slots.size();
  lld_map_covisibility_in in; std::memset(&in, 0, sizeof in);
  in.n_queries = (int32_t)nq; in.monocular = monocular ? 1 : 0; in.flags = flags; in.kf_slot = slots.data();
  lld_covisibility_params_default(&in.params);
  r.conn_start.assign(nq + 1, 0); r.ordered_start.assign(nq + 1, 0); r.n_max.assign(nq, 0); r.kf_max.assign(nq, -1); r.updated.assign(nq, 0);
  r.n_mps.assign(nq, 0); r.n_redundant.assign(nq, 0); r.redundant.assign(nq, 0); r.status.assign(nq, 0);
  size_t cap_c = 64 * nq, cap_o = 64 * nq;
  for (int attempt = 0;; attempt++) {
    r.conn_kf.assign(cap_c + 1, 0); r.conn_weight.assign(cap_c + 1, 0); r.ordered_kf.assign(cap_o + 1, 0); r.ordered_weight.assign(cap_o + 1, 0);
    lld_map_covisibility_out out; std::memset(&out, 0, sizeof out);
    lld_covisibility_out& L = out.lists;
    L.conn_capacity = (int32_t)cap_c; L.ordered_capacity = (int32_t)cap_o; L.n_conn = L.n_ordered = -1;
    L.conn_start = r.conn_start.data(); L.conn_kf = r.conn_kf.data(); L.conn_weight = r.conn_weight.data(); L.ordered_start = r.ordered_start.data();
    L.ordered_kf = r.ordered_kf.data(); L.ordered_weight = r.ordered_weight.data(); L.n_max = r.n_max.data(); L.kf_max = r.kf_max.data(); L.updated = r.updated.data();
    L.n_mps = r.n_mps.data(); L.n_redundant = r.n_redundant.data(); L.redundant = r.redundant.data();
    out.status = r.status.data();
    const int st = lld_map_covisibility(m, &in, &out);
    if (st == LLD_ERR_INVALID && attempt == 0 && L.n_conn >= 0 && ((size_t)L.n_conn > cap_c || (size_t)L.n_ordered > cap_o)) { cap_c = L.n_conn; cap_o = L.n_ordered; continue; }
    check(st, "lld_map_covisibility");
    return;
  }
}
}  // namespace

int MapOnDevice::UpdateConnections(const std::vector<KeyFrame*>& vpKFs, std::vector<KeyFrame*>* overflowed) {
  std::vector<KeyFrame*> queries; std::vector<int32_t> slots;
  for (size_t i = 0; i < vpKFs.size(); i++) {
    if (!vpKFs[i]) continue;
    if (KeyFrameOf(slot_of(vpKFs[i], limits_.max_keyframes)) != vpKFs[i]) throw std::runtime_error("MapOnDevice::UpdateConnections: a keyframe the map does not hold");
    queries.push_back(vpKFs[i]); slots.push_back((int32_t)vpKFs[i]->mnId);
  }
  if (queries.empty()) return 0;
  CovisResult o;
  covisibility(m_, slots, LLD_COVIS_CONNECTIONS | LLD_MAP_COVIS_WRITE_COV, false, o);
  std::set<KeyFrame*> touched, tree;                                   // received AddConnection; parent or children changed
  std::vector<KeyFrame*> over;
  int written = 0;
  for (size_t q = 0; q < queries.size(); q++) {
    // more covisible keyframes than the device answers for: nothing was written for this one, neither here nor in the map
    if (o.status[q]) { over.push_back(queries[q]); continue; }
    if (!o.updated[q]) continue;                                       // if(KFcounter.empty()) return;   (:346-347)
    KeyFrame* pKF = queries[q];
    written++;
    const int32_t s = o.ordered_start[q], e = o.ordered_start[q + 1];
    // (mit->first)->AddConnection(this, mit->second) for the counters >= th, or for pKFmax (:364-375): the ordered list holds exactly these
    for (int32_t j = s; j < e; j++) { KeyFrame* pN = kf_[o.ordered_kf[j]]; if (!pN) continue; pN->AddConnection(pKF, o.ordered_weight[j]); touched.insert(pN); }
    std::map<KeyFrame*, int> KFcounter;
    for (int32_t j = o.conn_start[q]; j < o.conn_start[q + 1]; j++) if (kf_[o.conn_kf[j]]) KFcounter[kf_[o.conn_kf[j]]] = o.conn_weight[j];
    pKF->mConnectedKeyFrameWeights = KFcounter;                        // :390-392
    pKF->mvpOrderedConnectedKeyFrames.clear(); pKF->mvOrderedWeights.clear();
    for (int32_t j = s; j < e; j++) if (kf_[o.ordered_kf[j]]) { pKF->mvpOrderedConnectedKeyFrames.push_back(kf_[o.ordered_kf[j]]); pKF->mvOrderedWeights.push_back(o.ordered_weight[j]); }
    if (pKF->mbFirstConnection && pKF->mnId != 0 && !pKF->mvpOrderedConnectedKeyFrames.empty()) {      // :394-399
      pKF->mpParent = pKF->mvpOrderedConnectedKeyFrames.front();
      pKF->mpParent->AddChild(pKF);
      pKF->mbFirstConnection = false;
      tree.insert(pKF); tree.insert(pKF->mpParent);
    }
  }
  // the map: the queries' own cov rows are written already (a query that is also a neighbour is sent again: the objects hold the final lists)
  std::vector<KeyFrame*> rows, cov;
  for (std::set<KeyFrame*>::const_iterator it = tree.begin(); it != tree.end(); ++it) rows.push_back(*it);
  for (std::set<KeyFrame*>::const_iterator it = touched.begin(); it != touched.end(); ++it) if (!tree.count(*it)) cov.push_back(*it);
  UpdateKeyFrames(rows);
  SetCovisibles(cov);
  // objects and map agree about every keyframe that was applied; the others are the caller's (pKF->UpdateConnections(), then UpdateKeyFrames)
  if (overflowed) *overflowed = over;
  else if (!over.empty()) throw std::runtime_error("MapOnDevice::UpdateConnections: more covisible keyframes than LLD_MAP_COVIS_MAX_CONNECTED");
  return written;
}

std::vector<KeyFrame*> MapOnDevice::KeyFrameCulling(KeyFrame* pCurrentKF, bool bMonocular, int* n_calls) {
  const std::vector<KeyFrame*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
  std::vector<KeyFrame*> flagged;
  int calls = 0;
  size_t at = 0;
  while (at < vpLocalKeyFrames.size()) {
    std::vector<size_t> where; std::vector<int32_t> slots;             // position in vpLocalKeyFrames of each query
    for (size_t i = at; i < vpLocalKeyFrames.size(); i++) {
      KeyFrame* pKF = vpLocalKeyFrames[i];
      if (pKF->mnId == 0) continue;                                    // :644-645
      if (KeyFrameOf(slot_of(pKF, limits_.max_keyframes)) != pKF) throw std::runtime_error("MapOnDevice::KeyFrameCulling: a keyframe the map does not hold");
      where.push_back(i); slots.push_back((int32_t)pKF->mnId);
    }
    if (slots.empty()) break;
    CovisResult o;
    covisibility(m_, slots, LLD_COVIS_CULLING, bMonocular, o);
    calls++;
    for (size_t q = 0; q < slots.size(); q++) if (o.status[q]) throw std::runtime_error("MapOnDevice::KeyFrameCulling: the map lacks keypoint data (EnableCovisibility before Upload)");
    at = vpLocalKeyFrames.size();
    for (size_t q = 0; q < slots.size(); q++) {
      if (!o.redundant[q]) continue;                                   // if(nRedundantObservations>0.9*nMPs)   (:694)
      KeyFrame* pKF = vpLocalKeyFrames[where[q]];
      // what SetBadFlag is about to change: its MapPoints lose an observation, its neighbours a connection
      std::set<MapPoint*> pts; std::vector<KeyFrame*> neighbours;
      const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
      for (size_t j = 0; j < vpMPs.size(); j++) if (vpMPs[j] && PointOf(slot_of(vpMPs[j], limits_.max_points)) == vpMPs[j]) pts.insert(vpMPs[j]);
      for (std::map<KeyFrame*, int>::const_iterator it = pKF->mConnectedKeyFrameWeights.begin(); it != pKF->mConnectedKeyFrameWeights.end(); ++it)
        if (KeyFrameOf(slot_of(it->first, limits_.max_keyframes)) == it->first) neighbours.push_back(it->first);
      // ... and the spanning tree is repaired (KeyFrame.cc:505-560): its children get new parents, those parents new children, its own
      // parent loses a child
      const std::set<KeyFrame*> spChilds = pKF->GetChilds();
      KeyFrame* pOldParent = pKF->GetParent();
      pKF->SetBadFlag();                                               // :695: observations are erased, the later counts are stale
      flagged.push_back(pKF);
      std::set<KeyFrame*> rows;                                        // whole rows: bad flag, parent, children (and the cov row with them)
      rows.insert(pKF);
      if (pOldParent) rows.insert(pOldParent);
      for (std::set<KeyFrame*>::const_iterator it = spChilds.begin(); it != spChilds.end(); ++it) { rows.insert(*it); if ((*it)->GetParent()) rows.insert((*it)->GetParent()); }
      std::vector<KeyFrame*> vRows, vCov;
      for (std::set<KeyFrame*>::const_iterator it = rows.begin(); it != rows.end(); ++it) if (KeyFrameOf(slot_of(*it, limits_.max_keyframes)) == *it) vRows.push_back(*it);
      for (size_t j = 0; j < neighbours.size(); j++) if (!rows.count(neighbours[j])) vCov.push_back(neighbours[j]);
      UpdatePoints(std::vector<MapPoint*>(pts.begin(), pts.end()));
      UpdateKeyFrames(vRows);
      SetCovisibles(vCov);
      at = where[q] + 1;
      break;
    }
  }
  if (n_calls) *n_calls = calls;
  return flagged;
}

void MapOnDevice::UpdateLines(const std::vector<MapLine*>& lines) {
  const size_t n = lines.size(), dim = limits_.line_dim;
  if (!n) return;
  std::vector<int32_t> slot(n); std::vector<double> x0(3 * n), dir(3 * n), x1(3 * n), x2(3 * n); std::vector<float> desc(n * dim, 0.f); std::vector<uint8_t> bad(n);
  for (size_t i = 0; i < n; i++) {
    MapLine* pML = lines[i];
    remember(ln_, pML, limits_.max_lines, "MapOnDevice::UpdateLines");
    slot[i] = (int32_t)pML->mnId; bad[i] = pML->isBad();
    lld_slam::Vector3d a, d, p1, p2;
    pML->GetMinimalPos(&a, &d); pML->GetMainPoints3D(&p1, &p2);
    for (int k = 0; k < 3; k++) { x0[3 * i + k] = a(k); dir[3 * i + k] = d(k); x1[3 * i + k] = p1(k); x2[3 * i + k] = p2(k); }
    lld_slam::Mat ml_desc;
    pML->GetDescriptor(&ml_desc);
    if (!ml_desc.empty()) {
      if ((size_t)ml_desc.cols != dim) throw std::runtime_error("MapOnDevice::UpdateLines: a descriptor of another length than line_dim");
      std::memcpy(&desc[i * dim], ml_desc.ptr<float>(), dim * 4);
    }
  }
  check(lld_map_set_lines(m_, (int32_t)n, slot.data(), x0.data(), dir.data(), x1.data(), x2.data(), desc.data(), bad.data()), "lld_map_set_lines");
  if (!ba_) return;
  std::vector<int32_t> start(1, 0), obs, idx, nobs(n);
  for (size_t i = 0; i < n; i++) {
    const std::map<KeyFrame*, size_t> observations = lines[i]->GetObservations();
    for (std::map<KeyFrame*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it) {
      const int32_t s = slot_of(it->first, limits_.max_keyframes);
      if (s >= 0) { obs.push_back(s); idx.push_back((int32_t)it->second); }
    }
    start.push_back((int32_t)obs.size());
    nobs[i] = lines[i]->Observations();
  }
  obs.push_back(0); idx.push_back(0);
  check(lld_map_set_line_observations(m_, (int32_t)n, slot.data(), start.data(), obs.data(), idx.data(), nobs.data()), "lld_map_set_line_observations");
}

}  // namespace lld_adapter
