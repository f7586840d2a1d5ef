// lld_covisibility_adapter.cc — see lld_covisibility_adapter.h.
#include "lld_covisibility_adapter.h"

#include <algorithm>
#include <functional>
#include <map>

namespace lld_adapter {

namespace {

// The observation table of one call: every map point the queried keyframes hold, each once, with its observations in std::map
// order; the keyframes met are numbered by pointer order afterwards.
struct Table {
  std::map<MapPoint*, int32_t> point_index;
  std::vector<MapPoint*> points;
  std::vector<KeyFrame*> obs_owner;            // per observation, before the slots are known
  std::vector<KeyFrame*> slots;                // sorted by std::less<KeyFrame*>
  lld_amd::CovisibilityBatch b;

  int32_t of(MapPoint* pMP, bool culling) {
    std::map<MapPoint*, int32_t>::const_iterator it = point_index.find(pMP);
    if (it != point_index.end()) return it->second;
    const int32_t i = (int32_t)points.size();
    point_index[pMP] = i; points.push_back(pMP);
    b.point_bad.push_back(pMP->isBad() ? 1 : 0);
    if (culling) b.point_nobs.push_back(pMP->Observations());
    const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
    for (std::map<KeyFrame*, size_t>::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
      obs_owner.push_back(mit->first);
      if (culling) b.obs_octave.push_back(mit->first->mvKeysUn[mit->second].octave);
    }
    b.obs_start.push_back((int32_t)obs_owner.size());
    return i;
  }

  void add_query(KeyFrame* pKF, bool culling) {
    const std::vector<MapPoint*> vpMP = pKF->GetMapPointMatches();
    for (size_t i = 0; i < vpMP.size(); i++) {
      MapPoint* pMP = vpMP[i];
      if (!pMP) continue;
      b.q_point.push_back(of(pMP, culling));
      if (culling) { b.q_octave.push_back(pKF->mvKeysUn[i].octave); b.q_depth.push_back(i < pKF->mvDepth.size() ? pKF->mvDepth[i] : -1.f); }
    }
    b.q_start.push_back((int32_t)b.q_point.size());
    if (culling) b.q_th_depth.push_back(pKF->mThDepth);
    queries.push_back(pKF);
  }

  void finish() {
    slots = queries;
    slots.insert(slots.end(), obs_owner.begin(), obs_owner.end());
    std::sort(slots.begin(), slots.end(), std::less<KeyFrame*>());
    slots.erase(std::unique(slots.begin(), slots.end()), slots.end());
    b.n_kf = (int32_t)slots.size();
    b.obs_kf.resize(obs_owner.size());
    for (size_t o = 0; o < obs_owner.size(); ++o) b.obs_kf[o] = slot(obs_owner[o]);
    b.query_kf.resize(queries.size());
    for (size_t q = 0; q < queries.size(); ++q) b.query_kf[q] = slot(queries[q]);
  }

  int32_t slot(KeyFrame* pKF) const {
    return (int32_t)(std::lower_bound(slots.begin(), slots.end(), pKF, std::less<KeyFrame*>()) - slots.begin());
  }

  std::vector<KeyFrame*> queries;
  Table() { b.obs_start.assign(1, 0); b.q_start.assign(1, 0); }
};

}  // namespace

int UpdateConnections(const lld_amd::Context& ctx, const std::vector<KeyFrame*>& vpKFs, float* phase_ms) {
  Table T;
  for (size_t i = 0; i < vpKFs.size(); ++i) if (vpKFs[i]) T.add_query(vpKFs[i], false);
  if (T.queries.empty()) return 0;
  T.finish();
  lld_amd::CovisibilityOutput o;
  lld_amd::Covisibility(ctx, T.b, LLD_COVIS_CONNECTIONS, o, phase_ms != nullptr);
  if (phase_ms) for (int k = 0; k < 3; ++k) phase_ms[k] = o.phase_ms[k];
  int written = 0;
  for (size_t q = 0; q < T.queries.size(); ++q) {
    if (!o.updated[q]) continue;                                       // if(KFcounter.empty()) return;   (:346-347)
    KeyFrame* pKF = T.queries[q];
    written++;
    const int32_t s = o.ordered_start[q], e = o.ordered_start[q + 1];
    // (mit->first)->AddConnection(this, mit->second) for the counters >= th, or for pKFmax (:364-375): the ordered list holds
    // exactly these keyframes
    for (int32_t j = s; j < e; ++j) T.slots[o.ordered_kf[j]]->AddConnection(pKF, o.ordered_weight[j]);
    std::map<KeyFrame*, int> KFcounter;
    for (int32_t j = o.conn_start[q]; j < o.conn_start[q + 1]; ++j) KFcounter[T.slots[o.conn_kf[j]]] = o.conn_weight[j];
    pKF->mConnectedKeyFrameWeights = KFcounter;                        // :390-392
    pKF->mvpOrderedConnectedKeyFrames.clear(); pKF->mvOrderedWeights.clear();
    for (int32_t j = s; j < e; ++j) { pKF->mvpOrderedConnectedKeyFrames.push_back(T.slots[o.ordered_kf[j]]); pKF->mvOrderedWeights.push_back(o.ordered_weight[j]); }
    if (pKF->mbFirstConnection && pKF->mnId != 0) {                    // :394-399
      pKF->mpParent = pKF->mvpOrderedConnectedKeyFrames.front();
      pKF->mpParent->AddChild(pKF);
      pKF->mbFirstConnection = false;
    }
  }
  return written;
}

std::vector<KeyFrame*> KeyFrameCulling(const lld_amd::Context& ctx, KeyFrame* pCurrentKF, bool bMonocular, int* n_calls, float* phase_ms) {
  const std::vector<KeyFrame*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
  std::vector<KeyFrame*> flagged;
  int calls = 0;
  if (phase_ms) phase_ms[0] = phase_ms[1] = phase_ms[2] = 0.f;
  size_t at = 0;
  while (at < vpLocalKeyFrames.size()) {
    Table T;
    T.b.monocular = bMonocular;
    std::vector<size_t> where;                                         // position in vpLocalKeyFrames of each query
    for (size_t i = at; i < vpLocalKeyFrames.size(); ++i) {
      if (vpLocalKeyFrames[i]->mnId == 0) continue;                    // :644-645
      T.add_query(vpLocalKeyFrames[i], true); where.push_back(i);
    }
    if (T.queries.empty()) break;
    T.finish();
    lld_amd::CovisibilityOutput o;
    lld_amd::Covisibility(ctx, T.b, LLD_COVIS_CULLING, o, phase_ms != nullptr);
    if (phase_ms) for (int k = 0; k < 3; ++k) phase_ms[k] += o.phase_ms[k];
    calls++;
    at = vpLocalKeyFrames.size();
    for (size_t q = 0; q < T.queries.size(); ++q) {
      if (!o.redundant[q]) continue;                                   // if(nRedundantObservations>0.9*nMPs)   (:694)
      T.queries[q]->SetBadFlag();                                      // :695: observations are erased, the later counts are stale
      flagged.push_back(T.queries[q]);
      at = where[q] + 1;
      break;
    }
  }
  if (n_calls) *n_calls = calls;
  return flagged;
}

}  // namespace lld_adapter
