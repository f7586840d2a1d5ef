// covisibility_harness: KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling through the object adapter
// (adapters/lld_covisibility_adapter.cc) on KeyFrame / MapPoint test doubles.
//   covisibility_harness scene.bin            run both and print the members
//   covisibility_harness scene.bin --time N   time both (N repetitions) against the same loops on the host alone
// scene.bin (little endian): int32 n_kf, n_points, monocular, n_update, current;
//   per keyframe: int32 mnId; float mThDepth; int32 n_keys; n_keys x (int32 octave, float depth, float uright, int32 point or -1);
//   int32 update[n_update]: the keyframes UpdateConnections is called for, in order.
// Every keypoint with a point adds the observation (MapPoint::AddObservation).  The keyframes live in one array, so pointer order is
// index order.  KeyFrameCulling runs for keyframe `current` after the update.
// Output: "U written"; per keyframe "K k parent first | slot:weight ... | ordered kf:weight ..."; "C calls flagged..."; per point
//   "P p bad nObs n_observations".
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../adapters/lld_covisibility_adapter.h"

using namespace lld_slam;

template <class T> static bool rd(FILE* f, T* x, size_t n = 1) { return n == 0 || fread(x, sizeof(T), n, f) == n; }

// ---- the same two routines with nothing but the objects and their std::maps (timing only)
static void HostUpdateConnections(KeyFrame* pKF) {
  std::map<KeyFrame*, int> counter;
  const std::vector<MapPoint*> vpMP = pKF->GetMapPointMatches();
  for (size_t i = 0; i < vpMP.size(); i++) {
    if (!vpMP[i] || vpMP[i]->isBad()) continue;
    const std::map<KeyFrame*, size_t> obs = vpMP[i]->GetObservations();
    for (std::map<KeyFrame*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it)
      if (it->first->mnId != pKF->mnId) counter[it->first]++;
  }
  if (counter.empty()) return;
  int nmax = 0; KeyFrame* best = nullptr;
  std::vector<std::pair<int, KeyFrame*> > pairs;
  for (std::map<KeyFrame*, int>::iterator it = counter.begin(); it != counter.end(); ++it) {
    if (it->second > nmax) { nmax = it->second; best = it->first; }
    if (it->second >= 15) { pairs.push_back(std::make_pair(it->second, it->first)); it->first->AddConnection(pKF, it->second); }
  }
  if (pairs.empty()) { pairs.push_back(std::make_pair(nmax, best)); best->AddConnection(pKF, nmax); }
  std::sort(pairs.begin(), pairs.end());
  pKF->mConnectedKeyFrameWeights = counter;
  pKF->mvpOrderedConnectedKeyFrames.clear(); pKF->mvOrderedWeights.clear();
  for (size_t i = pairs.size(); i-- > 0;) { pKF->mvpOrderedConnectedKeyFrames.push_back(pairs[i].second); pKF->mvOrderedWeights.push_back(pairs[i].first); }
  if (pKF->mbFirstConnection && pKF->mnId != 0) { pKF->mpParent = pKF->mvpOrderedConnectedKeyFrames.front(); pKF->mpParent->AddChild(pKF); pKF->mbFirstConnection = false; }
}

static int HostCullingCount(KeyFrame* pCurrentKF, bool mono) {          // the verdicts only: nothing is flagged, so it can be repeated
  const std::vector<KeyFrame*> local = pCurrentKF->GetVectorCovisibleKeyFrames();
  int n_redundant_kfs = 0;
  for (size_t k = 0; k < local.size(); k++) {
    KeyFrame* pKF = local[k];
    if (pKF->mnId == 0) continue;
    const std::vector<MapPoint*> vpMP = pKF->GetMapPointMatches();
    int n_mps = 0, n_red = 0;
    for (size_t i = 0; i < vpMP.size(); i++) {
      MapPoint* pMP = vpMP[i];
      if (!pMP || pMP->isBad()) continue;
      if (!mono && (pKF->mvDepth[i] > pKF->mThDepth || pKF->mvDepth[i] < 0)) continue;
      n_mps++;
      if (pMP->Observations() <= 3) continue;
      const int level = pKF->mvKeysUn[i].octave;
      const std::map<KeyFrame*, size_t> obs = pMP->GetObservations();
      int n = 0;
      for (std::map<KeyFrame*, size_t>::const_iterator it = obs.begin(); it != obs.end() && n < 3; ++it)
        if (it->first != pKF && it->first->mvKeysUn[it->second].octave <= level + 1) n++;
      if (n >= 3) n_red++;
    }
    if (n_red > 0.9 * n_mps) n_redundant_kfs++;
  }
  return n_redundant_kfs;
}

template <class F> static double median_ms(int reps, F f) {
  std::vector<double> t;
  for (int r = 0; r < reps; ++r) {
    const std::chrono::steady_clock::time_point a = std::chrono::steady_clock::now();
    f();
    t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count());
  }
  std::sort(t.begin(), t.end());
  return t[t.size() / 2];
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: covisibility_harness scene.bin [--time reps]\n"); return 2; }
  const int reps = (argc >= 4 && !std::strcmp(argv[2], "--time")) ? atoi(argv[3]) : 0;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_kf, n_points, mono, n_update, current;
  if (!rd(f, &n_kf) || !rd(f, &n_points) || !rd(f, &mono) || !rd(f, &n_update) || !rd(f, &current)) return 2;
  if (n_kf < 1 || n_points < 0 || n_update < 0 || current < 0 || current >= n_kf) return 2;
  std::vector<KeyFrame> kfs(n_kf);
  std::vector<MapPoint> pts(n_points);
  for (int k = 0; k < n_kf; ++k) {
    KeyFrame& K = kfs[k];
    int32_t id, nk;
    if (!rd(f, &id) || !rd(f, &K.mThDepth) || !rd(f, &nk) || nk < 0) return 2;
    K.mnId = (unsigned long)id; K.N = nk;
    K.mvKeysUn.resize(nk); K.mvDepth.resize(nk); K.mvuRight.resize(nk); K.mvpMapPoints.assign(nk, nullptr);
    for (int i = 0; i < nk; ++i) {
      int32_t oct, p;
      if (!rd(f, &oct) || !rd(f, &K.mvDepth[i]) || !rd(f, &K.mvuRight[i]) || !rd(f, &p) || p >= n_points) return 2;
      K.mvKeysUn[i].octave = oct;
      if (p >= 0) { K.mvpMapPoints[i] = &pts[p]; pts[p].AddObservation(&K, (size_t)i); }
    }
  }
  for (int p = 0; p < n_points; ++p) pts[p].mnId = p;
  std::vector<int32_t> upd(n_update);
  if (!rd(f, upd.data(), upd.size())) return 2;
  fclose(f);
  std::vector<KeyFrame*> vpKFs;
  for (int i = 0; i < n_update; ++i) { if (upd[i] < 0 || upd[i] >= n_kf) return 2; vpKFs.push_back(&kfs[upd[i]]); }
  try {
    lld_amd::Context ctx(0);
    if (reps > 0) {
      // the members are the same after either route and after every repetition (AddConnection with an unchanged weight returns
      // at once), so the two routes are timed on the same state; the culling is timed on its verdicts alone
      float ph[3];
      lld_adapter::UpdateConnections(ctx, vpKFs);
      const double host_u = median_ms(reps, [&] { for (size_t i = 0; i < vpKFs.size(); ++i) HostUpdateConnections(vpKFs[i]); });
      std::vector<float> p0, p1, p2;
      const double dev_u = median_ms(reps, [&] { lld_adapter::UpdateConnections(ctx, vpKFs, ph); p0.push_back(ph[0]); p1.push_back(ph[1]); p2.push_back(ph[2]); });
      std::sort(p0.begin(), p0.end()); std::sort(p1.begin(), p1.end()); std::sort(p2.begin(), p2.end());
      printf("{\"case\": \"UpdateConnections\", \"keyframes\": %d, \"host_loop_ms\": %.4f, \"adapter_ms\": %.4f, \"upload_ms\": %.4f, \"kernels_ms\": %.4f, \"download_ms\": %.4f}\n",
             n_update, host_u, dev_u, p0[p0.size() / 2], p1[p1.size() / 2], p2[p2.size() / 2]);
      KeyFrame* cur = &kfs[current];
      int verdicts = 0;
      const double host_c = median_ms(reps, [&] { verdicts = HostCullingCount(cur, mono != 0); });
      if (verdicts != 0) { fprintf(stderr, "covisibility_harness: the timing scene must cull nothing (%d redundant)\n", verdicts); return 1; }
      p0.clear(); p1.clear(); p2.clear();
      int calls = 0; size_t n_flagged = 0;
      lld_adapter::KeyFrameCulling(ctx, cur, mono != 0, &calls);
      const double dev_c = median_ms(reps, [&] { n_flagged += lld_adapter::KeyFrameCulling(ctx, cur, mono != 0, &calls, ph).size(); p0.push_back(ph[0]); p1.push_back(ph[1]); p2.push_back(ph[2]); });
      std::sort(p0.begin(), p0.end()); std::sort(p1.begin(), p1.end()); std::sort(p2.begin(), p2.end());
      printf("{\"case\": \"KeyFrameCulling\", \"keyframes\": %d, \"flagged\": %d, \"host_loop_ms\": %.4f, \"adapter_ms\": %.4f, \"upload_ms\": %.4f, \"kernels_ms\": %.4f, \"download_ms\": %.4f}\n",
             (int)cur->mvpOrderedConnectedKeyFrames.size(), (int)n_flagged, host_c, dev_c, p0[p0.size() / 2], p1[p1.size() / 2], p2[p2.size() / 2]);
      return 0;
    }
    const int written = lld_adapter::UpdateConnections(ctx, vpKFs);
    printf("U %d\n", written);
    for (int k = 0; k < n_kf; ++k) {
      const KeyFrame& K = kfs[k];
      printf("K %d %d %d |", k, K.mpParent ? (int)(K.mpParent - kfs.data()) : -1, K.mbFirstConnection ? 1 : 0);
      for (std::map<KeyFrame*, int>::const_iterator it = K.mConnectedKeyFrameWeights.begin(); it != K.mConnectedKeyFrameWeights.end(); ++it)
        printf(" %d:%d", (int)(it->first - kfs.data()), it->second);
      printf(" |");
      for (size_t i = 0; i < K.mvpOrderedConnectedKeyFrames.size(); ++i)
        printf(" %d:%d", (int)(K.mvpOrderedConnectedKeyFrames[i] - kfs.data()), K.mvOrderedWeights[i]);
      printf("\n");
    }
    int calls = 0;
    const std::vector<KeyFrame*> flagged = lld_adapter::KeyFrameCulling(ctx, &kfs[current], mono != 0, &calls);
    printf("C %d", calls);
    for (size_t i = 0; i < flagged.size(); ++i) printf(" %d", (int)(flagged[i] - kfs.data()));
    printf("\n");
    for (int p = 0; p < n_points; ++p) printf("P %d %d %d %d\n", p, pts[p].isBad() ? 1 : 0, pts[p].Observations(), (int)pts[p].mObservations.size());
  } catch (const std::exception& e) {
    fprintf(stderr, "covisibility_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
