// lld_map_adapter.cc — see lld_map_adapter.h.  Each Update* gathers the listed objects' rows into flat arrays and makes one lld_map_set_* call
// (two for MapPoints: the fixed rows and the observation rows).
#include "lld_map_adapter.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
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
  std::vector<int32_t> slot(n), start(1, 0), obs; std::vector<float> pos(3 * n), nrm(3 * n), mind(n), maxd(n); std::vector<uint32_t> desc(8 * n, 0u); std::vector<uint8_t> bad(n);
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
      if (s >= 0) obs.push_back(s);
    }
    start.push_back((int32_t)obs.size());
  }
  obs.push_back(0);                                                            // (never read: a non-null pointer for an empty list)
  check(lld_map_set_points(m_, (int32_t)n, slot.data(), pos.data(), nrm.data(), mind.data(), maxd.data(), desc.data(), bad.data()), "lld_map_set_points");
  check(lld_map_set_observations(m_, (int32_t)n, slot.data(), start.data(), obs.data()), "lld_map_set_observations");
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
}

}  // namespace lld_adapter
