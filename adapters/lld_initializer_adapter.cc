// lld_initializer_adapter.cc — see lld_initializer_adapter.h.
#include "lld_initializer_adapter.h"

namespace lld_adapter {

static std::vector<float> keys_xy(const Frame& F) {
  std::vector<float> xy(2 * F.mvKeysUn.size());
  for (size_t i = 0; i < F.mvKeysUn.size(); ++i) { xy[2 * i] = F.mvKeysUn[i].pt.x; xy[2 * i + 1] = F.mvKeysUn[i].pt.y; }
  return xy;
}

Initializer::Initializer(const lld_amd::Context& ctx, const Frame& ReferenceFrame, float sigma, int iterations, uint32_t seed)
    : ini_(ctx, ReferenceFrame.mK.ptr<float>(), keys_xy(ReferenceFrame), sigma, iterations, seed) {}

bool Initializer::Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, Mat& R21, Mat& t21,
                             std::vector<Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
  float R[9], t[3];
  std::vector<float> p3d;
  std::vector<bool> tri;
  if (!ini_.Initialize(keys_xy(CurrentFrame), vMatches12, R, t, p3d, tri)) return false;
  R21 = Mat(3, 3, R);                                                        // R.copyTo(R21), t.copyTo(t21) (:530-531, :723-724)
  t21 = Mat(3, 1, t);
  vP3D.resize(tri.size());                                                   // vP3D = vP3Di: mvKeys1.size() entries (:809)
  for (size_t i = 0; i < tri.size(); ++i) vP3D[i] = Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
  vbTriangulated = tri;
  return true;
}

}  // namespace lld_adapter
