// map_fuse_harness — ORBmatcher::Fuse and LocalMapping::SearchInNeighbors on the resident map, on objects: adapters/lld_map_adapter.cc's
// MapOnDevice::Fuse / SearchInNeighbors on one object graph (A) and adapters/lld_matcher_adapter.cc's ORBmatcher::Fuse / the reference's loop
// (src/LocalMapping.cc:455-535 with lld_landmark_adapter and lld_covisibility_adapter behind it) on an identical one (B).
//   map_fuse_harness fuse scene.bin        one Fuse(target, candidates, th): both graphs printed member by member ("A ..." / "B ..."), then
//                                          graph A's map as the device holds it ("T ...")
//   map_fuse_harness neighbors scene.bin   SearchInNeighbors(target) likewise
//   map_fuse_harness time scene.bin reps   host clock of both SearchInNeighbors routes, B followed by MapOnDevice::UpdatePoints /
//                                          UpdateKeyFrames (its results sent back into a map); the graphs are loaded again before every
//                                          repetition (not timed): the routine changes them
// The scene file is written by tests/test_gpu_map_fuse_cpp.py (object_scene): keyframe s is slot s and, the graph's keyframes lying in one
// array, std::map<KeyFrame*, size_t> iterates in slot order.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../adapters/lld_covisibility_adapter.h"
#include "../adapters/lld_landmark_adapter.h"
#include "../adapters/lld_map_adapter.h"
#include "../adapters/lld_matcher_adapter.h"
#include "../include/lld_amd.hpp"

using namespace lld_slam;

struct Graph {
  int32_t n_kf = 0, n_pts = 0, n_levels = 0, target = 0, n_cand = 0; float th = 3.f;
  std::vector<KeyFrame> kfs; std::vector<MapPoint> pts; std::vector<uint8_t> exists;
  std::vector<KeyFrame*> vpKFs; std::vector<MapPoint*> vpMapPoints, cand;
};
template <class T> static bool rd(FILE* f, T* x, size_t n = 1) { return n == 0 || fread(x, sizeof(T), n, f) == n; }

static bool load(const char* path, Graph& G) {
  G = Graph();
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  float cam[5], bounds[4], grid_inv[2], lsf;
  if (!rd(f, &G.n_kf) || !rd(f, &G.n_pts) || !rd(f, &G.n_levels) || !rd(f, &G.target) || !rd(f, &G.n_cand) || !rd(f, &G.th) || !rd(f, cam, 5) || !rd(f, bounds, 4) ||
      !rd(f, grid_inv, 2) || !rd(f, &lsf)) return false;
  std::vector<float> scale(G.n_levels), sigma2(G.n_levels), inv_sigma2(G.n_levels);
  if (!rd(f, scale.data(), scale.size()) || !rd(f, inv_sigma2.data(), inv_sigma2.size())) return false;
  for (int l = 0; l < G.n_levels; l++) sigma2[l] = scale[l] * scale[l];
  G.kfs.resize(G.n_kf); G.pts.resize(G.n_pts); G.exists.assign(G.n_pts, 0);
  std::vector<std::vector<int32_t> > rows(G.n_kf), cov(G.n_kf);
  for (int k = 0; k < G.n_kf; ++k) {
    KeyFrame& K = G.kfs[k];
    int32_t bad, nk, nc; float T[16], ow[3];
    if (!rd(f, &bad) || !rd(f, T, 16) || !rd(f, ow, 3) || !rd(f, &nk)) return false;
    K.mnId = k; K.mbBad = bad != 0; K.Tcw = Mat(4, 4, T); K.Ow = Mat(3, 1, ow);
    K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mbf = cam[4];
    K.mnMinX = (int)bounds[0]; K.mnMaxX = (int)bounds[1]; K.mnMinY = (int)bounds[2]; K.mnMaxY = (int)bounds[3];
    K.mfGridElementWidthInv = grid_inv[0]; K.mfGridElementHeightInv = grid_inv[1];
    K.mnScaleLevels = G.n_levels; K.mfScaleFactor = scale.size() > 1 ? scale[1] : 1.f; K.mfLogScaleFactor = lsf;
    K.mvScaleFactors = scale; K.mvLevelSigma2 = sigma2; K.mvInvLevelSigma2 = inv_sigma2;
    K.N = nk; K.mvKeysUn.resize(nk); K.mvKeys.resize(nk); K.mvuRight.resize(nk); K.mvDepth.assign(nk, -1.f); K.mDescriptors = MatU8(nk, 32); K.mvpMapPoints.assign(nk, nullptr);
    rows[k].resize(nk);
    for (int i = 0; i < nk; ++i) {
      float uvr[3]; int32_t oct;
      if (!rd(f, uvr, 3) || !rd(f, &oct) || !rd(f, K.mDescriptors.ptr<uint32_t>(i), 8) || !rd(f, &rows[k][i])) return false;
      K.mvKeysUn[i].pt.x = uvr[0]; K.mvKeysUn[i].pt.y = uvr[1]; K.mvKeysUn[i].octave = oct; K.mvKeys[i] = K.mvKeysUn[i]; K.mvuRight[i] = uvr[2];
    }
    if (!rd(f, &nc)) return false;
    cov[k].resize(nc);
    if (!rd(f, cov[k].data(), (size_t)nc)) return false;
    G.vpKFs.push_back(&K);
  }
  for (int k = 0; k < G.n_kf; ++k) {
    for (size_t j = 0; j < cov[k].size(); j++) { G.kfs[k].mvpOrderedConnectedKeyFrames.push_back(&G.kfs[cov[k][j]]); G.kfs[k].mvOrderedWeights.push_back((int)(cov[k].size() - j)); }
    for (size_t i = 0; i < rows[k].size(); i++) if (rows[k][i] >= 0) G.kfs[k].mvpMapPoints[i] = &G.pts[rows[k][i]];
  }
  for (int i = 0; i < G.n_pts; ++i) {
    MapPoint& P = G.pts[i];
    int32_t ex, bad, nobs, ref, no; float pos[3], nrm[3], mn, mx;
    P.mDescriptor = MatU8(1, 32); P.mnId = i;
    if (!rd(f, &ex) || !rd(f, &bad) || !rd(f, pos, 3) || !rd(f, nrm, 3) || !rd(f, &mn) || !rd(f, &mx) || !rd(f, P.mDescriptor.ptr<uint32_t>(), 8) || !rd(f, &nobs) || !rd(f, &ref) ||
        !rd(f, &no)) return false;
    G.exists[i] = ex != 0; P.mbBad = bad != 0; P.mWorldPos = Mat(3, 1, pos); P.mNormalVector = Mat(3, 1, nrm); P.mfMinDistance = mn; P.mfMaxDistance = mx; P.nObs = nobs;
    P.mpRefKF = ref >= 0 ? &G.kfs[ref] : nullptr; P.mnFound = 1 + i % 5; P.mnVisible = 2 + i % 7;
    for (int o = 0; o < no; ++o) {
      int32_t kf, idx;
      if (!rd(f, &kf) || !rd(f, &idx)) return false;
      P.mObservations[&G.kfs[kf]] = (size_t)idx;
    }
    if (ex) G.vpMapPoints.push_back(&P);
  }
  for (int i = 0; i < G.n_cand; ++i) {
    int32_t s;
    if (!rd(f, &s)) return false;
    G.cand.push_back(s >= 0 ? &G.pts[s] : nullptr);
  }
  fclose(f);
  return true;
}

static lld_map_limits limits_of(const Graph& G) {
  size_t kp = 0, ob = 0;
  for (const KeyFrame& K : G.kfs) kp += K.mvpMapPoints.size();
  for (const MapPoint& P : G.pts) ob += P.mObservations.size();
  lld_map_limits L{};
  L.max_keyframes = G.n_kf + 1; L.max_points = G.n_pts + 1; L.max_lines = 1; L.line_dim = 8; L.max_observations = (int32_t)(2 * ob + kp) + 64;
  L.max_kf_points = (int32_t)kp + 8; L.max_kf_lines = 8; L.max_children = G.n_kf + 8; L.max_local_points = 64; L.max_local_lines = 16;
  return L;
}

static void hex(const void* v, int n) {
  unsigned u;
  for (int q = 0; q < n; ++q) { std::memcpy(&u, (const char*)v + 4 * q, 4); std::printf(" %08x", u); }
}
// every member the routines write, of every MapPoint and KeyFrame
static void print(const char* tag, const Graph& G, int ret) {
  std::printf("%s R %d\n", tag, ret);
  for (int i = 0; i < G.n_pts; ++i) {
    const MapPoint& P = G.pts[i];
    if (!G.exists[i]) continue;
    std::printf("%s P %d %d %d %d %d %ld %lu %zu", tag, i, (int)P.mbBad, P.nObs, P.mnFound, P.mnVisible, P.mpReplaced ? (long)P.mpReplaced->mnId : -1L, P.mnFuseCandidateForKF, P.mObservations.size());
    for (std::map<KeyFrame*, size_t>::const_iterator it = P.mObservations.begin(); it != P.mObservations.end(); ++it) std::printf(" %lu %zu", it->first->mnId, it->second);
    std::printf("\n%s D %d", tag, i);
    hex(P.mDescriptor.ptr<uint32_t>(), 8); hex(P.mNormalVector.ptr<float>(), 3); hex(&P.mfMinDistance, 1); hex(&P.mfMaxDistance, 1);
    std::printf("\n");
  }
  for (int k = 0; k < G.n_kf; ++k) {
    const KeyFrame& K = G.kfs[k];
    std::printf("%s K %d %lu %ld %zu", tag, k, K.mnFuseTargetForKF, K.mpParent ? (long)K.mpParent->mnId : -1L, K.mvpMapPoints.size());
    for (size_t i = 0; i < K.mvpMapPoints.size(); i++) std::printf(" %ld", K.mvpMapPoints[i] ? (long)K.mvpMapPoints[i]->mnId : -1L);
    std::printf("\n%s C %d %zu", tag, k, K.mvpOrderedConnectedKeyFrames.size());
    for (size_t i = 0; i < K.mvpOrderedConnectedKeyFrames.size(); i++) std::printf(" %lu %d", K.mvpOrderedConnectedKeyFrames[i]->mnId, K.mvOrderedWeights[i]);
    std::printf("\n");
  }
}
// graph A's map as the device holds it
static int print_map(lld_map* m, const Graph& G) {
  const int np = G.n_pts, nk = G.n_kf;
  std::vector<int32_t> ps(np), ks(nk);
  for (int i = 0; i < np; ++i) ps[i] = i;
  for (int k = 0; k < nk; ++k) ks[k] = k;
  const int kinds[3] = {LLD_MAP_ROWS_POINT_OBS, LLD_MAP_ROWS_POINT_IDX, LLD_MAP_ROWS_KF_POINTS};
  for (int q = 0; q < 3; q++) {
    const std::vector<int32_t>& sl = q < 2 ? ps : ks;
    std::vector<int32_t> start(sl.size() + 1, 0);
    (void)lld_map_download_rows(m, kinds[q], (int32_t)sl.size(), sl.data(), start.data(), 0, nullptr);
    std::vector<int32_t> data((size_t)start.back() + 1);
    if (lld_map_download_rows(m, kinds[q], (int32_t)sl.size(), sl.data(), start.data(), start.back(), data.data()) != LLD_OK) return 1;
    for (size_t i = 0; i < sl.size(); i++) {
      std::printf("T %d %zu %d", q, i, start[i + 1] - start[i]);
      for (int j = start[i]; j < start[i + 1]; j++) std::printf(" %d", data[j]);
      std::printf("\n");
    }
  }
  std::vector<int32_t> cnt(np + 1); std::vector<uint32_t> d(8 * (size_t)np + 1); std::vector<uint8_t> st(np + 1); std::vector<float> nrm(3 * (size_t)np + 1), mn(np + 1), mx(np + 1);
  if (lld_map_download_point_counts(m, np, ps.data(), cnt.data()) != LLD_OK) return 1;
  if (lld_map_download_points(m, np, ps.data(), nullptr, nrm.data(), mn.data(), mx.data(), d.data(), st.data()) != LLD_OK) return 1;
  for (int i = 0; i < np; ++i) { std::printf("T 3 %d %d %d", i, cnt[i], (int)st[i]); hex(&d[8 * (size_t)i], 8); hex(&nrm[3 * (size_t)i], 3); hex(&mn[i], 1); hex(&mx[i], 1); std::printf("\n"); }
  return 0;
}
static void upload(lld_adapter::MapOnDevice& M, Graph& G) {
  M.EnableRefresh();
  M.UpdateKeyFrames(G.vpKFs); M.UpdatePoints(G.vpMapPoints);
}

// LocalMapping::SearchInNeighbors (src/LocalMapping.cc:455-535, nn = 10) on objects with the gathering adapters
static int host_search_in_neighbors(const lld_amd::Context& ctx, KeyFrame* pKF) {
  const std::vector<KeyFrame*> vpNeighKFs = pKF->GetBestCovisibilityKeyFrames(10);
  std::vector<KeyFrame*> vpTargetKFs;
  for (size_t i = 0; i < vpNeighKFs.size(); i++) {
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
  lld_adapter::ORBmatcher matcher(ctx.get());
  int n = 0;
  std::vector<MapPoint*> vpMapPointMatches = pKF->GetMapPointMatches();
  for (size_t i = 0; i < vpTargetKFs.size(); i++) n += matcher.Fuse(vpTargetKFs[i], vpMapPointMatches);
  std::vector<MapPoint*> vpFuseCandidates;
  for (size_t i = 0; i < vpTargetKFs.size(); i++) {
    const std::vector<MapPoint*> v = vpTargetKFs[i]->GetMapPointMatches();
    for (size_t j = 0; j < v.size(); j++) {
      MapPoint* pMP = v[j];
      if (!pMP || pMP->isBad() || pMP->mnFuseCandidateForKF == pKF->mnId) continue;
      pMP->mnFuseCandidateForKF = pKF->mnId;
      vpFuseCandidates.push_back(pMP);
    }
  }
  n += matcher.Fuse(pKF, vpFuseCandidates);
  vpMapPointMatches = pKF->GetMapPointMatches();
  std::vector<MapPoint*> live; std::set<MapPoint*> seen;
  for (size_t i = 0; i < vpMapPointMatches.size(); i++)
    if (vpMapPointMatches[i] && !vpMapPointMatches[i]->isBad() && seen.insert(vpMapPointMatches[i]).second) live.push_back(vpMapPointMatches[i]);
  lld_adapter::RefreshMapPoints(ctx, live, LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH);
  lld_adapter::UpdateConnections(ctx, std::vector<KeyFrame*>(1, pKF));
  return n;
}

static int run(const char* path, bool neighbors) {
  Graph A, B;
  if (!load(path, A) || !load(path, B)) return 2;
  try {
    lld_amd::Context ctx(0);
    lld_adapter::MapOnDevice M(ctx.get(), limits_of(A));
    upload(M, A);
    int ra, rb;
    if (neighbors) {
      ra = M.SearchInNeighbors(&A.kfs[A.target]);
      rb = host_search_in_neighbors(ctx, &B.kfs[B.target]);
    } else {
      ra = M.Fuse(&A.kfs[A.target], A.cand, A.th);
      lld_adapter::ORBmatcher matcher(ctx.get());
      rb = matcher.Fuse(&B.kfs[B.target], B.cand, B.th);
    }
    print("A", A, ra); print("B", B, rb);
    return print_map(M.get(), A);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "map_fuse_harness: %s\n", e.what());
    return 1;
  }
}

static int time_routes(const char* path, int reps) {
  try {
    lld_amd::Context ctx(0);
    std::vector<double> ta, tb;
    int ra = 0, rb = 0;
    for (int r = -3; r < reps; ++r) {
      Graph A, B;
      if (!load(path, A) || !load(path, B)) return 2;
      lld_adapter::MapOnDevice MA(ctx.get(), limits_of(A)), MB(ctx.get(), limits_of(B));
      upload(MA, A); upload(MB, B);
      lld_ctx_synchronize(ctx.get());
      const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
      ra = MA.SearchInNeighbors(&A.kfs[A.target]);
      lld_ctx_synchronize(ctx.get());
      const std::chrono::steady_clock::time_point t1 = std::chrono::steady_clock::now();
      rb = host_search_in_neighbors(ctx, &B.kfs[B.target]);
      MB.UpdatePoints(B.vpMapPoints); MB.UpdateKeyFrames(B.vpKFs);
      lld_ctx_synchronize(ctx.get());
      const std::chrono::steady_clock::time_point t2 = std::chrono::steady_clock::now();
      if (r >= 0) { ta.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); tb.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count()); }
    }
    std::printf("{\"fused_map\": %d, \"fused_adapter\": %d, \"map_route_ms\": [", ra, rb);
    for (size_t i = 0; i < ta.size(); i++) std::printf("%s%.4f", i ? ", " : "", ta[i]);
    std::printf("], \"adapter_and_update_ms\": [");
    for (size_t i = 0; i < tb.size(); i++) std::printf("%s%.4f", i ? ", " : "", tb[i]);
    std::printf("]}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "map_fuse_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "fuse")) return run(argv[2], false);
  if (argc == 3 && !std::strcmp(argv[1], "neighbors")) return run(argv[2], true);
  if (argc == 4 && !std::strcmp(argv[1], "time")) return time_routes(argv[2], std::atoi(argv[3]));
  std::fprintf(stderr, "usage: map_fuse_harness fuse scene.bin | neighbors scene.bin | time scene.bin reps\n");
  return 2;
}
