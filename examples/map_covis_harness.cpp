// map_covis_harness: KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling on the resident map - adapters/lld_map_adapter.cc's
// MapOnDevice::UpdateConnections / KeyFrameCulling (lld_map_covisibility: no gather, no upload of the map) - on KeyFrame / MapPoint test doubles
// that a MapOnDevice mirrors.
//   map_covis_harness scene.bin           run both and print the members (the line format of covisibility_harness); then "M k | slot:weight ..":
//                                         the connections the device counts on the mirrored map for every keyframe that is left; then
//                                         "R1 k parent | cov .. | children .." per keyframe: the links the map held after UpdateConnections
//                                         (lld_map_download_links), and "R2 ..": after the culling walk
//   map_covis_harness scene.bin time N    time both against the same loops on the host alone: two identical copies of the graph, the routes
//                                         alternating, N repetitions, host-clock medians and quartiles.  The map is current before every timed
//                                         window and the pushes back into it (cov rows, tree changes) are inside the window.
// scene.bin: the blob of tests/covis_scenes.py World.blob (see covisibility_harness.cpp).  A keyframe's slot is its mnId, which the scenes
// number by index, so pointer order is slot order here; the device orders by order_key = the pointer value all the same.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../adapters/lld_map_adapter.h"
#include "../include/lld_amd.hpp"

using namespace lld_slam;

template <class T> static bool rd(FILE* f, T* x, size_t n = 1) { return n == 0 || fread(x, sizeof(T), n, f) == n; }

struct Graph {
  std::vector<KeyFrame> kfs; std::vector<MapPoint> pts; std::vector<int32_t> upd;
  int32_t mono = 0, current = 0; long n_obs = 0, n_keys = 0;
  std::vector<KeyFrame*> all() { std::vector<KeyFrame*> v; for (size_t k = 0; k < kfs.size(); k++) v.push_back(&kfs[k]); return v; }
  std::vector<MapPoint*> points() { std::vector<MapPoint*> v; for (size_t p = 0; p < pts.size(); p++) v.push_back(&pts[p]); return v; }
  std::vector<KeyFrame*> list() { std::vector<KeyFrame*> v; for (size_t i = 0; i < upd.size(); i++) v.push_back(&kfs[upd[i]]); return v; }
};

static bool load(const char* path, Graph& G) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  int32_t n_kf, n_points, n_update;
  if (!rd(f, &n_kf) || !rd(f, &n_points) || !rd(f, &G.mono) || !rd(f, &n_update) || !rd(f, &G.current)) return false;
  if (n_kf < 1 || n_points < 0 || n_update < 0 || G.current < 0 || G.current >= n_kf) return false;
  G.kfs.resize(n_kf); G.pts.resize(n_points);
  for (int p = 0; p < n_points; ++p) { G.pts[p].mnId = p; G.pts[p].mWorldPos = Mat(3, 1); G.pts[p].mNormalVector = Mat(3, 1); }
  for (int k = 0; k < n_kf; ++k) {
    KeyFrame& K = G.kfs[k];
    int32_t id, nk;
    if (!rd(f, &id) || !rd(f, &K.mThDepth) || !rd(f, &nk) || nk < 0 || id != k) return false;      // slot = mnId = index
    K.mnId = (unsigned long)id; K.N = nk;
    K.mvKeysUn.resize(nk); K.mvDepth.resize(nk); K.mvuRight.resize(nk); K.mvpMapPoints.assign(nk, nullptr);
    G.n_keys += nk;
    for (int i = 0; i < nk; ++i) {
      int32_t oct, p;
      if (!rd(f, &oct) || !rd(f, &K.mvDepth[i]) || !rd(f, &K.mvuRight[i]) || !rd(f, &p) || p >= n_points) return false;
      K.mvKeysUn[i].octave = oct;
      if (p >= 0) { K.mvpMapPoints[i] = &G.pts[p]; G.pts[p].AddObservation(&K, (size_t)i); }
    }
  }
  for (int p = 0; p < n_points; ++p) G.n_obs += (long)G.pts[p].mObservations.size();
  G.upd.resize(n_update);
  if (!rd(f, G.upd.data(), G.upd.size())) return false;
  for (int i = 0; i < n_update; ++i) if (G.upd[i] < 0 || G.upd[i] >= n_kf) return false;
  fclose(f);
  return true;
}

static lld_map_limits limits_of(const Graph& G) {
  lld_map_limits L; std::memset(&L, 0, sizeof L);
  L.max_keyframes = (int32_t)G.kfs.size(); L.max_points = (int32_t)G.pts.size() + 1; L.max_lines = 0; L.line_dim = 8;
  L.max_observations = (int32_t)G.n_obs + 64; L.max_kf_points = (int32_t)G.n_keys + 64; L.max_kf_lines = 0; L.max_children = 2 * (int32_t)G.kfs.size() + 8;
  L.max_local_points = (int32_t)G.pts.size() + 16; L.max_local_lines = 0;
  return L;
}

// ---- the same two routines with nothing but the objects and their std::maps (timing only; as in covisibility_harness.cpp)
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

struct Stat { double q1, med, q3; };
static Stat stat(std::vector<double> t) {
  std::sort(t.begin(), t.end());
  const Stat s = {t[t.size() / 4], t[t.size() / 2], t[(3 * t.size()) / 4]};
  return s;
}
template <class A, class B> static void alternate(int reps, A resident, B host, const char* name, int keyframes) {
  std::vector<double> ta, tb;
  typedef std::chrono::steady_clock clk;
  for (int r = 0; r < reps; ++r) {
    clk::time_point a = clk::now(); resident(); ta.push_back(std::chrono::duration<double, std::milli>(clk::now() - a).count());
    a = clk::now(); host(); tb.push_back(std::chrono::duration<double, std::milli>(clk::now() - a).count());
  }
  const Stat x = stat(ta), y = stat(tb);
  printf("{\"case\": \"%s\", \"keyframes\": %d, \"reps\": %d, \"resident_ms\": %.4f, \"resident_q1\": %.4f, \"resident_q3\": %.4f, \"host_loop_ms\": %.4f, \"host_q1\": %.4f, \"host_q3\": %.4f}\n",
         name, keyframes, reps, x.med, x.q1, x.q3, y.med, y.q1, y.q3);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: map_covis_harness scene.bin [time reps]\n"); return 2; }
  const int reps = (argc >= 4 && !std::strcmp(argv[2], "time")) ? atoi(argv[3]) : 0;
  Graph G, H;                                                            // H: the identical copy the host loops run on (timing only)
  if (!load(argv[1], G) || (reps > 0 && !load(argv[1], H))) { fprintf(stderr, "map_covis_harness: cannot read %s\n", argv[1]); return 2; }
  const int n_kf = (int)G.kfs.size();
  try {
    lld_amd::Context ctx(0);
    lld_adapter::MapOnDevice mod(ctx.get(), limits_of(G));
    mod.EnableCovisibility();
    mod.UpdateKeyFrames(G.all()); mod.UpdatePoints(G.points());
    std::vector<KeyFrame*> vpKFs = G.list();
    if (reps > 0) {
      // the members are the same after either route and after every repetition, so every window starts from the same graph and the same map
      std::vector<KeyFrame*> hostKFs = H.list();
      mod.UpdateConnections(vpKFs);
      for (size_t i = 0; i < hostKFs.size(); ++i) HostUpdateConnections(hostKFs[i]);
      alternate(reps, [&] { mod.UpdateConnections(vpKFs); }, [&] { for (size_t i = 0; i < hostKFs.size(); ++i) HostUpdateConnections(hostKFs[i]); }, "UpdateConnections",
                (int)vpKFs.size());
      std::vector<KeyFrame*> one(1, vpKFs.back()); KeyFrame* hone = hostKFs.back();
      alternate(reps, [&] { mod.UpdateConnections(one); }, [&] { HostUpdateConnections(hone); }, "UpdateConnections_one", 1);
      KeyFrame* cur = &G.kfs[G.current]; KeyFrame* hcur = &H.kfs[H.current];
      int verdicts = HostCullingCount(hcur, H.mono != 0);
      if (verdicts != 0) { fprintf(stderr, "map_covis_harness: the timing scene must cull nothing (%d redundant)\n", verdicts); return 1; }
      size_t n_flagged = 0;
      alternate(reps, [&] { n_flagged += mod.KeyFrameCulling(cur, G.mono != 0).size(); }, [&] { verdicts += HostCullingCount(hcur, H.mono != 0); }, "KeyFrameCulling",
                (int)cur->mvpOrderedConnectedKeyFrames.size());
      if (n_flagged || verdicts) { fprintf(stderr, "map_covis_harness: the routes disagree with the host's verdicts\n"); return 1; }
      return 0;
    }
    const int written = mod.UpdateConnections(vpKFs);
    printf("U %d\n", written);
    for (int k = 0; k < n_kf; ++k) {
      const KeyFrame& K = G.kfs[k];
      printf("K %d %d %d |", k, K.mpParent ? (int)(K.mpParent - G.kfs.data()) : -1, K.mbFirstConnection ? 1 : 0);
      for (std::map<KeyFrame*, int>::const_iterator it = K.mConnectedKeyFrameWeights.begin(); it != K.mConnectedKeyFrameWeights.end(); ++it)
        printf(" %d:%d", (int)(it->first - G.kfs.data()), it->second);
      printf(" |");
      for (size_t i = 0; i < K.mvpOrderedConnectedKeyFrames.size(); ++i) printf(" %d:%d", (int)(K.mvpOrderedConnectedKeyFrames[i] - G.kfs.data()), K.mvOrderedWeights[i]);
      printf("\n");
    }
    // what the map holds of every keyframe's links (lld_map_download_links reads k_parent, k_cov and the child rows on the device)
    std::vector<int32_t> every;
    for (int k = 0; k < n_kf; ++k) every.push_back(k);
    std::string links;
    auto read_links = [&](const char* tag) {
      const lld_amd::DeviceMap::Links l = lld_amd::DeviceMap::DownloadLinksOn(mod.get(), every);
      for (int k = 0; k < n_kf; ++k) {
        links += std::string(tag) + " " + std::to_string(k) + " " + std::to_string(l.parent[k]) + " |";
        for (int32_t j = l.cov_start[k]; j < l.cov_start[k + 1]; ++j) links += " " + std::to_string(l.cov[j]);
        links += " |";
        std::vector<int32_t> ch(l.child.begin() + l.child_start[k], l.child.begin() + l.child_start[k + 1]);
        std::sort(ch.begin(), ch.end());
        for (size_t j = 0; j < ch.size(); ++j) links += " " + std::to_string(ch[j]);
        links += "\n";
      }
    };
    read_links("R1");                                                    // after UpdateConnections
    int calls = 0;
    const std::vector<KeyFrame*> flagged = mod.KeyFrameCulling(&G.kfs[G.current], G.mono != 0, &calls);
    read_links("R2");                                                    // after the culling walk
    printf("C %d", calls);
    for (size_t i = 0; i < flagged.size(); ++i) printf(" %d", (int)(flagged[i] - G.kfs.data()));
    printf("\n");
    for (size_t p = 0; p < G.pts.size(); ++p) printf("P %d %d %d %d\n", (int)p, G.pts[p].isBad() ? 1 : 0, G.pts[p].Observations(), (int)G.pts[p].mObservations.size());
    // the mirrored map after both routines, read back through the device: every keyframe that is not bad counts the connections its object holds
    std::vector<int32_t> live;
    for (int k = 0; k < n_kf; ++k) if (!G.kfs[k].isBad()) live.push_back(k);
    lld_amd::DeviceMap::CovisibilityResult r = lld_amd::DeviceMap::CovisibilityOn(mod.get(), live, LLD_COVIS_CONNECTIONS, false);
    for (size_t q = 0; q < live.size(); ++q) {
      printf("M %d |", live[q]);
      for (int32_t j = r.conn_start[q]; j < r.conn_start[q + 1]; ++j) printf(" %d:%d", r.conn_kf[j], r.conn_weight[j]);
      printf("\n");
    }
    fputs(links.c_str(), stdout);
  } catch (const std::exception& e) {
    fprintf(stderr, "map_covis_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
