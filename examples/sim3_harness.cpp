// sim3_harness: LoopClosing::ComputeSim3's RANSAC rounds (LoopClosing.cc:289-342, without the SearchBySim3 / OptimizeSim3 part)
// through the object adapter (adapters/lld_sim3_adapter.cc) on live KeyFrame / MapPoint test doubles, then lld_amd::Sim3Solver's
// iterate + find on candidate 0.
//   sim3_harness scene.bin
// scene.bin (little endian): int32 n_cand, n1, n_levels, max_rounds, n_it, fix_scale; float sigma2[n_levels];
//   KF1: float fx, fy, cx, cy, Tcw[12] (3x4 row-major); n1 x int32 octave; n1 x (int32 state: 0 NULL, 1 good, 2 isBad,
//   3 not observed by KF1; float x, y, z unless NULL);
//   per candidate: uint32 seed; float fx, fy, cx, cy, Tcw[12]; int32 n2; n2 x int32 octave; then n1 x (int32 state: 0 NULL
//   match, 1 good, 2 isBad, 3 not observed by the candidate; unless NULL: int32 index in the candidate, float x, y, z).
// Output, one line per call: "R round cand has_pose no_more n_inliers" then the 12 T12 floats and the best scale as hex bits,
// then the indices i1 set in vbInliers; then "S ..." / "F ..." for candidate 0's single-solver iterate(n_it) and find().
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../adapters/lld_sim3_adapter.h"

using namespace lld_slam;

template <class T> static bool rd(FILE* f, T* x, size_t n = 1) { return fread(x, sizeof(T), n, f) == n; }

static void print(const char* tag, int round, int cand, bool has, bool no_more, int n_in, const float* T, float s,
                  const std::vector<bool>& inl) {
  printf("%s %d %d %d %d %d", tag, round, cand, has ? 1 : 0, no_more ? 1 : 0, n_in);
  unsigned u;
  for (int q = 0; q < 12; ++q) { std::memcpy(&u, T + q, 4); printf(" %08x", u); }
  std::memcpy(&u, &s, 4); printf(" %08x", u);
  for (size_t k = 0; k < inl.size(); ++k) if (inl[k]) printf(" %zu", k);
  printf("\n");
}

// fx, fy, cx, cy, Tcw[12], then (n_kp < 0: an int32 count first) the keypoints' octaves.
static bool read_keyframe(FILE* f, KeyFrame& kf, const std::vector<float>& sigma2, int n_kp) {
  float cam[4], T[12];
  if (!rd(f, cam, 4) || !rd(f, T, 12)) return false;
  if (n_kp < 0 && !rd(f, &n_kp)) return false;
  kf.fx = cam[0]; kf.fy = cam[1]; kf.cx = cam[2]; kf.cy = cam[3];
  kf.mK = Mat(3, 3);
  kf.mK.at<float>(0, 0) = cam[0]; kf.mK.at<float>(1, 1) = cam[1]; kf.mK.at<float>(0, 2) = cam[2]; kf.mK.at<float>(1, 2) = cam[3];
  kf.mK.at<float>(2, 2) = 1.f;
  Mat Tcw(4, 4);
  for (int q = 0; q < 12; ++q) Tcw.at<float>(q / 4, q % 4) = T[q];
  Tcw.at<float>(3, 3) = 1.f;
  kf.SetPose(Tcw);
  kf.mvLevelSigma2 = sigma2;
  kf.mvKeysUn.resize(n_kp);
  kf.mvuRight.assign(n_kp, -1.f);
  kf.mvpMapPoints.assign(n_kp, nullptr);
  for (int i = 0; i < n_kp; ++i) {
    int32_t oct;
    if (!rd(f, &oct)) return false;
    kf.mvKeysUn[i].octave = oct;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: sim3_harness scene.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[6];
  if (!rd(f, hdr, 6)) return 2;
  const int n_cand = hdr[0], n1 = hdr[1], n_levels = hdr[2], max_rounds = hdr[3], n_it = hdr[4];
  const bool fix_scale = hdr[5] != 0;
  std::vector<float> sigma2(n_levels);
  if (!rd(f, sigma2.data(), n_levels)) return 2;
  std::vector<std::unique_ptr<MapPoint> > owned;
  auto point = [&](const float* xyz, int state) {
    owned.emplace_back(new MapPoint());
    owned.back()->mWorldPos = Mat(3, 1, xyz);
    owned.back()->mbBad = state == 2;
    return owned.back().get();
  };
  KeyFrame KF1;
  if (!read_keyframe(f, KF1, sigma2, n1)) return 2;
  for (int i = 0; i < n1; ++i) {
    int32_t state;
    float xyz[3];
    if (!rd(f, &state)) return 2;
    if (state == 0) continue;
    if (!rd(f, xyz, 3)) return 2;
    MapPoint* p = point(xyz, state);
    if (state != 3) p->AddObservation(&KF1, i);
    KF1.AddMapPoint(p, i);
  }
  std::vector<std::unique_ptr<KeyFrame> > cands;
  std::vector<KeyFrame*> pcands;
  std::vector<std::vector<MapPoint*> > matches(n_cand, std::vector<MapPoint*>(n1, nullptr));
  std::vector<uint32_t> seeds(n_cand);
  for (int c = 0; c < n_cand; ++c) {
    if (!rd(f, &seeds[c])) return 2;
    cands.emplace_back(new KeyFrame());
    KeyFrame& kf = *cands.back();
    if (!read_keyframe(f, kf, sigma2, -1)) return 2;
    pcands.push_back(&kf);
    for (int i = 0; i < n1; ++i) {
      int32_t state, idx2;
      float xyz[3];
      if (!rd(f, &state)) return 2;
      if (state == 0) continue;
      if (!rd(f, &idx2) || !rd(f, xyz, 3)) return 2;
      MapPoint* p = point(xyz, state);
      if (state != 3) p->AddObservation(&kf, idx2);
      matches[c][i] = p;
    }
  }
  fclose(f);
  try {
    lld_amd::Context ctx(0);
    lld_adapter::Sim3Solvers solvers(ctx, &KF1, pcands, matches, fix_scale, lld_amd::Sim3SolverBatch::defaults(), seeds);
    std::vector<uint8_t> live(n_cand, 1);
    std::vector<Mat> Scm; std::vector<bool> no_more; std::vector<std::vector<bool> > inl; std::vector<int> n_in;
    for (int r = 0; r < max_rounds; ++r) {
      bool any = false;
      for (int c = 0; c < n_cand; ++c) any = any || live[c];
      if (!any) break;
      solvers.iterate(n_it, live, Scm, no_more, inl, n_in);
      for (int c = 0; c < n_cand; ++c) {
        if (!live[c]) continue;
        float T[12] = {0};
        if (!Scm[c].empty())
          for (int q = 0; q < 12; ++q) T[q] = Scm[c].at<float>(q / 4, q % 4);
        print("R", r, c, !Scm[c].empty(), no_more[c], n_in[c], T, solvers.GetEstimatedScale(c), inl[c]);
        if (no_more[c]) live[c] = 0;
      }
    }
    lld_amd::Sim3Solver one(ctx, lld_adapter::GatherSim3(&KF1, pcands[0], matches[0], fix_scale, seeds[0]));
    bool bNoMore = false; std::vector<bool> v; int n = 0; float T[12];
    bool has = one.iterate(n_it, bNoMore, v, n, T);
    print("S", 0, 0, has, bNoMore, n, T, one.GetEstimatedScale(), v);
    has = one.find(v, n, T);
    print("F", 0, 0, has, false, n, T, one.GetEstimatedScale(), v);
  } catch (const std::exception& e) {
    fprintf(stderr, "sim3_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
