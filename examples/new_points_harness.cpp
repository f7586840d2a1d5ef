// new_points_harness: LocalMapping::CreateNewMapPoints through the object adapter (adapters/lld_localmapping_adapter.cc) on
// KeyFrame / MapPoint / Map test doubles: the sequential neighbour loop, ComputeF12, the SearchForTriangulation adapter, one
// lld_new_points_triangulate call per neighbour, the reference's bookkeeping and one landmark refresh at the end.
//   new_points_harness scene.bin
// scene.bin (little endian): int32 n_kf, n_levels, monocular, stop_at; float scale_factor, scale[n_levels], sigma2[n_levels];
//   per keyframe: float Tcw[16], fx, fy, cx, cy, mb, mbf; int32 n_keys;
//     n_keys x (float x, y, raw_x, raw_y, ur, depth; int32 octave; uint32 desc[8]);
//     int32 n_nodes; n_nodes x (int32 node, int32 count, int32 idx[count])     (mFeatVec)
// Keyframe 0 is mpCurrentKeyFrame, the others its covisibles in order.  CheckNewKeyFrames() returns true from its stop_at-th call
// on (1-based; 0: never).  The keyframes live in one array, so a std::map<KeyFrame*,size_t> iterates in keyframe index order.
// Output: "F k" and F12 of neighbour k (9 hex words) for every neighbour; "R nnew early"; per neighbour visited "N k skipped
//   n_matches n_new"; per created point in mlpRecentAddedMapPoints order "P kf1 kf2 idx1 idx2" and as hex bits mWorldPos (3),
//   mDescriptor (8), mNormalVector (3), mfMinDistance, mfMaxDistance.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <list>
#include <vector>

#include "../adapters/lld_localmapping_adapter.h"

using namespace lld_slam;

template <class T> static bool rd(FILE* f, T* x, size_t n = 1) { return n == 0 || fread(x, sizeof(T), n, f) == n; }

static void hex(const void* v, int n) {
  unsigned u;
  for (int q = 0; q < n; ++q) { std::memcpy(&u, (const char*)v + 4 * q, 4); printf(" %08x", u); }
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: new_points_harness scene.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_kf, n_levels, monocular, stop_at; float scale_factor;
  if (!rd(f, &n_kf) || !rd(f, &n_levels) || !rd(f, &monocular) || !rd(f, &stop_at) || !rd(f, &scale_factor)) return 2;
  std::vector<float> scale(n_levels), sigma2(n_levels), inv_sigma2(n_levels);
  if (!rd(f, scale.data(), scale.size()) || !rd(f, sigma2.data(), sigma2.size())) return 2;
  for (int l = 0; l < n_levels; ++l) inv_sigma2[l] = 1.0f / sigma2[l];
  std::vector<KeyFrame> kfs(n_kf);
  for (int k = 0; k < n_kf; ++k) {
    KeyFrame& K = kfs[k];
    float T[16], c[6]; int32_t nk, nn;
    if (!rd(f, T, 16) || !rd(f, c, 6) || !rd(f, &nk)) return 2;
    K.mnId = k; K.Tcw = Mat(4, 4, T);
    { Frame tmp; tmp.SetPose(K.Tcw); K.Ow = tmp.mOw; }                         // Ow = -Rwc*tcw (KeyFrame.cc:85)
    K.fx = c[0]; K.fy = c[1]; K.cx = c[2]; K.cy = c[3]; K.mb = c[4]; K.mbf = c[5];
    K.invfx = 1.0f / K.fx; K.invfy = 1.0f / K.fy;
    K.mK = Mat(3, 3);
    K.mK.at<float>(0, 0) = K.fx; K.mK.at<float>(1, 1) = K.fy; K.mK.at<float>(0, 2) = K.cx; K.mK.at<float>(1, 2) = K.cy; K.mK.at<float>(2, 2) = 1.f;
    K.mnScaleLevels = n_levels; K.mfScaleFactor = scale_factor; K.mfLogScaleFactor = std::log(scale_factor);
    K.mvScaleFactors = scale; K.mvLevelSigma2 = sigma2; K.mvInvLevelSigma2 = inv_sigma2;
    K.mnMinX = 0; K.mnMinY = 0; K.mnMaxX = 1241; K.mnMaxY = 376;
    K.mfGridElementWidthInv = 64.0f / 1241.0f; K.mfGridElementHeightInv = 48.0f / 376.0f;
    K.N = nk; K.mvKeysUn.resize(nk); K.mvKeys.resize(nk); K.mvuRight.resize(nk); K.mvDepth.resize(nk); K.mDescriptors = MatU8(nk, 32);
    K.mvpMapPoints.assign(nk, nullptr);
    for (int i = 0; i < nk; ++i) {
      float v[6]; int32_t oct;
      if (!rd(f, v, 6) || !rd(f, &oct) || !rd(f, K.mDescriptors.ptr<uint32_t>(i), 8)) return 2;
      K.mvKeysUn[i].pt.x = v[0]; K.mvKeysUn[i].pt.y = v[1]; K.mvKeysUn[i].octave = oct;
      K.mvKeys[i].pt.x = v[2]; K.mvKeys[i].pt.y = v[3]; K.mvKeys[i].octave = oct;
      K.mvuRight[i] = v[4]; K.mvDepth[i] = v[5];
    }
    if (!rd(f, &nn)) return 2;
    for (int q = 0; q < nn; ++q) {
      int32_t node, cnt;
      if (!rd(f, &node) || !rd(f, &cnt)) return 2;
      std::vector<int32_t> idx(cnt);
      if (!rd(f, idx.data(), idx.size())) return 2;
      K.mFeatVec[(unsigned)node].assign(idx.begin(), idx.end());
    }
  }
  fclose(f);
  for (int k = 1; k < n_kf; ++k) kfs[0].mvpOrderedConnectedKeyFrames.push_back(&kfs[k]);
  try {
    lld_amd::Context ctx(0);
    KeyFrame* cur = &kfs[0];
    for (int k = 1; k < n_kf; ++k) {
      KeyFrame* nb = &kfs[k];
      const Mat F12 = lld_adapter::ComputeF12(cur, nb);
      printf("F %d", k); hex(F12.ptr<float>(), 9); printf("\n");
    }
    Map map;
    std::list<MapPoint*> recent;
    lld_adapter::NewPointsTrace tr;
    int calls = 0;
    const int nnew = lld_adapter::CreateNewMapPoints(ctx, cur, &map, monocular != 0, recent,
                                                     [&]() { ++calls; return stop_at > 0 && calls >= stop_at; }, &tr);
    printf("R %d %d\n", nnew, tr.returned_early ? 1 : 0);
    for (size_t k = 0; k < tr.skipped.size(); ++k) printf("N %d %d %d %d\n", (int)k + 1, tr.skipped[k], tr.n_matches[k], tr.n_new[k]);
    if ((int)recent.size() != nnew || (int)map.mspMapPoints.size() != nnew) { fprintf(stderr, "bookkeeping: %d created, %d recent, %d in the map\n", nnew, (int)recent.size(), (int)map.mspMapPoints.size()); return 1; }
    for (std::list<MapPoint*>::const_iterator it = recent.begin(); it != recent.end(); ++it) {
      MapPoint* P = *it;
      const std::map<KeyFrame*, size_t> obs = P->GetObservations();
      if (obs.size() != 2 || !obs.count(cur) || P->mpRefKF != cur) { fprintf(stderr, "a new point without its two observations\n"); return 1; }
      KeyFrame* other = nullptr;
      for (std::map<KeyFrame*, size_t>::const_iterator o = obs.begin(); o != obs.end(); ++o) if (o->first != cur) other = o->first;
      const size_t idx1 = obs.find(cur)->second, idx2 = obs.find(other)->second;
      if (cur->GetMapPoint(idx1) != P || other->GetMapPoint(idx2) != P) { fprintf(stderr, "AddMapPoint missing\n"); return 1; }
      printf("P %lu %lu %d %d", cur->mnId, other->mnId, (int)idx1, (int)idx2);
      hex(P->mWorldPos.ptr<float>(), 3); hex(P->mDescriptor.ptr<uint32_t>(), 8); hex(P->mNormalVector.ptr<float>(), 3);
      hex(&P->mfMinDistance, 1); hex(&P->mfMaxDistance, 1);
      printf("\n");
    }
    for (std::list<MapPoint*>::iterator it = recent.begin(); it != recent.end(); ++it) delete *it;
  } catch (const std::exception& e) {
    fprintf(stderr, "new_points_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
