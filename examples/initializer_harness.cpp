// initializer_harness: Tracking::MonocularInitialization's Initialize (Tracking.cc:626-630) through lld_amd::Initializer and
// through the object adapter (adapters/lld_initializer_adapter.cc) on Frame test doubles.
//   initializer_harness scene.bin
// scene.bin (little endian): float K[9]; float sigma; int32 iterations; uint32 seed; int32 n1, n2, n_calls; n1 x (float x, y);
//   per call: n2 x (float x, y) of the current frame, n1 x int32 vMatches12.
// Output per call: "C call success model best_index n_matches win_H win_F n_inliers_H n_inliers_F" then as hex bits SH SF,
//   H21 (9), F21 (9), R21 (9), t21 (3), parallax (8), then n_good (8) in decimal; "H ..." / "F ..." the indices set in the
//   inlier masks; "T ..." the indices set in vbTriangulated; "P ..." vP3D (3*n1 hex).  Then the adapter: "A call ret untouched"
//   with R21 (9) t21 (3) as hex, "AT ..." its vbTriangulated indices, "AP ..." its vP3D; `untouched` is 1 when both frames still
//   hold exactly what they held before the call and, on failure, the four outputs kept their sentinel values.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../adapters/lld_initializer_adapter.h"

using namespace lld_slam;

template <class T> static bool rd(FILE* f, T* x, size_t n = 1) { return fread(x, sizeof(T), n, f) == n; }

static void hex(const float* v, int n) {
  unsigned u;
  for (int q = 0; q < n; ++q) { std::memcpy(&u, v + q, 4); printf(" %08x", u); }
}

static Frame make_frame(const float* K, const std::vector<float>& xy) {
  Frame F;
  F.mK = Mat(3, 3, K);
  F.fx = K[0]; F.fy = K[4]; F.cx = K[2]; F.cy = K[5];
  F.N = (int)(xy.size() / 2);
  F.mvKeysUn.resize(F.N);
  for (int i = 0; i < F.N; ++i) { F.mvKeysUn[i].pt.x = xy[2 * i]; F.mvKeysUn[i].pt.y = xy[2 * i + 1]; }
  F.mvKeys = F.mvKeysUn;
  return F;
}

static bool same_frame(const Frame& a, const Frame& b) {
  if (a.mvKeysUn.size() != b.mvKeysUn.size() || a.N != b.N || !a.mTcw.empty() || a.n_set_pose != b.n_set_pose) return false;
  for (size_t i = 0; i < a.mvKeysUn.size(); ++i)
    if (std::memcmp(&a.mvKeysUn[i].pt, &b.mvKeysUn[i].pt, sizeof(Point2f)) != 0) return false;
  return std::memcmp(a.mK.ptr<float>(), b.mK.ptr<float>(), 9 * sizeof(float)) == 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: initializer_harness scene.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  float K[9], sigma; int32_t iterations, n1, n2, n_calls; uint32_t seed;
  if (!rd(f, K, 9) || !rd(f, &sigma) || !rd(f, &iterations) || !rd(f, &seed) || !rd(f, &n1) || !rd(f, &n2) || !rd(f, &n_calls)) return 2;
  std::vector<float> k1(2 * (size_t)n1);
  if (!rd(f, k1.data(), k1.size())) return 2;
  std::vector<std::vector<float> > k2(n_calls, std::vector<float>(2 * (size_t)n2));
  std::vector<std::vector<int> > m12(n_calls, std::vector<int>(n1));
  for (int c = 0; c < n_calls; ++c)
    if (!rd(f, k2[c].data(), k2[c].size()) || !rd(f, m12[c].data(), m12[c].size())) return 2;
  fclose(f);
  try {
    lld_amd::Context ctx(0);
    lld_amd::Initializer ini(ctx, K, k1, sigma, iterations, seed);
    const Frame F1 = make_frame(K, k1), F1copy = F1;
    lld_adapter::Initializer adapter(ctx, F1, sigma, iterations, seed);
    for (int c = 0; c < n_calls; ++c) {
      const lld_amd::InitializerOutput o = ini.Run(k2[c], m12[c]);
      const lld_initializer_result& r = o.r;
      printf("C %d %d %d %d %d %d %d %d %d", c, r.success, r.model, r.best_index, r.n_matches, r.win_H, r.win_F, r.n_inliers_H, r.n_inliers_F);
      hex(&r.SH, 1); hex(&r.SF, 1); hex(r.H21, 9); hex(r.F21, 9); hex(r.R21, 9); hex(r.t21, 3); hex(r.parallax, 8);
      for (int q = 0; q < 8; ++q) printf(" %d", r.n_good[q]);
      printf("\nH");
      for (size_t i = 0; i < o.inlier_H.size(); ++i) if (o.inlier_H[i]) printf(" %zu", i);
      printf("\nF");
      for (size_t i = 0; i < o.inlier_F.size(); ++i) if (o.inlier_F[i]) printf(" %zu", i);
      printf("\nT");
      for (size_t i = 0; i < o.triangulated.size(); ++i) if (o.triangulated[i]) printf(" %zu", i);
      printf("\nP"); hex(o.p3d.data(), (int)o.p3d.size()); printf("\n");
      // the adapter on Frame objects; sentinels show what a failed call leaves behind
      const Frame F2 = make_frame(K, k2[c]), F2copy = F2;
      Mat R21(1, 1), t21(1, 1);
      R21.at<float>(0) = -7.f; t21.at<float>(0) = -8.f;
      std::vector<Point3f> vP3D(2, Point3f(1.f, 2.f, 3.f));
      std::vector<bool> vbTriangulated(3, true);
      const bool ret = adapter.Initialize(F2, m12[c], R21, t21, vP3D, vbTriangulated);
      bool untouched = same_frame(F1, F1copy) && same_frame(F2, F2copy);
      if (!ret)
        untouched = untouched && R21.rows == 1 && R21.at<float>(0) == -7.f && t21.rows == 1 && t21.at<float>(0) == -8.f &&
                    vP3D.size() == 2 && vP3D[1].z == 3.f && vbTriangulated.size() == 3 && vbTriangulated[2];
      printf("A %d %d %d", c, ret ? 1 : 0, untouched ? 1 : 0);
      if (ret) { hex(R21.ptr<float>(), 9); hex(t21.ptr<float>(), 3); }
      printf("\nAT");
      if (ret) for (size_t i = 0; i < vbTriangulated.size(); ++i) if (vbTriangulated[i]) printf(" %zu", i);
      printf("\nAP");
      if (ret) for (size_t i = 0; i < vP3D.size(); ++i) { const float p[3] = {vP3D[i].x, vP3D[i].y, vP3D[i].z}; hex(p, 3); }
      printf("\n");
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "initializer_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
