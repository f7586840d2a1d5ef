// pnp_harness: Tracking::Relocalization's PnP rounds (Tracking.cc:1894-1916, without the PoseOptimization part) through the
// object adapter (adapters/lld_pnp_adapter.cc) on live Frame / MapPoint test doubles, then lld_amd::PnPsolver's iterate + find on
// candidate 0.
//   pnp_harness scene.bin
// scene.bin (little endian): int32 n_cand, n_kp, n_levels, max_rounds, n_it; float fx, fy, cx, cy; float sigma2[n_levels];
//   n_kp x (float u, v; int32 octave); per candidate: uint32 seed, then n_kp x (int32 state: 0 NULL, 1 good, 2 isBad;
//   float x, y, z unless NULL).
// Output, one line per call: "R round cand has_pose no_more n_inliers iterations" then the 12 Tcw floats as hex bits and the
// inlier keypoint indices; then "S ..." / "F ..." for candidate 0's single-solver iterate(5) and find().
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../adapters/lld_pnp_adapter.h"

using namespace lld_slam;

template <class T> static bool rd(FILE* f, T* x, size_t n = 1) { return fread(x, sizeof(T), n, f) == n; }

static void print(const char* tag, int round, int cand, bool has, bool no_more, int n_in, int its, const float* T, const std::vector<bool>& inl) {
  printf("%s %d %d %d %d %d %d", tag, round, cand, has ? 1 : 0, no_more ? 1 : 0, n_in, its);
  for (int q = 0; q < 12; ++q) { unsigned u; std::memcpy(&u, T + q, 4); printf(" %08x", u); }
  for (size_t k = 0; k < inl.size(); ++k) if (inl[k]) printf(" %zu", k);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: pnp_harness scene.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[5]; float cam[4];
  if (!rd(f, hdr, 5) || !rd(f, cam, 4)) return 2;
  const int n_cand = hdr[0], n_kp = hdr[1], n_levels = hdr[2], max_rounds = hdr[3], n_it = hdr[4];
  Frame F;
  F.fx = cam[0]; F.fy = cam[1]; F.cx = cam[2]; F.cy = cam[3];
  F.mvLevelSigma2.resize(n_levels);
  if (!rd(f, F.mvLevelSigma2.data(), n_levels)) return 2;
  F.mvKeysUn.resize(n_kp);
  for (int i = 0; i < n_kp; ++i) {
    float uv[2]; int32_t oct;
    if (!rd(f, uv, 2) || !rd(f, &oct)) return 2;
    F.mvKeysUn[i].pt.x = uv[0]; F.mvKeysUn[i].pt.y = uv[1]; F.mvKeysUn[i].octave = oct;
  }
  std::vector<std::unique_ptr<MapPoint> > owned;
  std::vector<std::vector<MapPoint*> > matches(n_cand, std::vector<MapPoint*>(n_kp, nullptr));
  std::vector<uint32_t> seeds(n_cand);
  for (int c = 0; c < n_cand; ++c) {
    if (!rd(f, &seeds[c])) return 2;
    for (int i = 0; i < n_kp; ++i) {
      int32_t state;
      if (!rd(f, &state)) return 2;
      if (state == 0) continue;
      float xyz[3];
      if (!rd(f, xyz, 3)) return 2;
      owned.emplace_back(new MapPoint());
      owned.back()->mWorldPos = Mat(3, 1, xyz);
      owned.back()->mbBad = state == 2;
      matches[c][i] = owned.back().get();
    }
  }
  fclose(f);
  try {
    lld_amd::Context ctx(0);
    lld_adapter::PnPsolvers solvers(ctx, F, matches, lld_amd::PnPsolverBatch::defaults(), seeds);
    std::vector<uint8_t> live(n_cand, 1);
    std::vector<Mat> Tcw; std::vector<bool> no_more; std::vector<std::vector<bool> > inl; std::vector<int> n_in;
    std::vector<int> its(n_cand, 0);
    for (int r = 0; r < max_rounds; ++r) {
      bool any = false;
      for (int c = 0; c < n_cand; ++c) any = any || live[c];
      if (!any) break;
      solvers.iterate(n_it, live, Tcw, no_more, inl, n_in);
      for (int c = 0; c < n_cand; ++c) {
        if (!live[c]) continue;
        float T[12] = {0};
        if (!Tcw[c].empty())
          for (int q = 0; q < 12; ++q) T[q] = Tcw[c].at<float>(q / 4, q % 4);
        print("R", r, c, !Tcw[c].empty(), no_more[c], n_in[c], -1, T, inl[c]);
        if (no_more[c]) live[c] = 0;
      }
    }
    lld_amd::PnPsolver one(ctx, lld_adapter::GatherPnP(F, matches[0], seeds[0]));
    bool bNoMore = false; std::vector<bool> v; int n = 0; float T[12];
    bool has = one.iterate(n_it, bNoMore, v, n, T);
    print("S", 0, 0, has, bNoMore, n, -1, T, v);
    has = one.find(v, n, T);
    print("F", 0, 0, has, false, n, -1, T, v);
  } catch (const std::exception& e) {
    fprintf(stderr, "pnp_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
