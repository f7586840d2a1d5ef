// landmark_harness: LocalMapping's per-landmark refresh (MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth,
// MapLine::ComputeDistinctiveDescriptors) through the object adapter (adapters/lld_landmark_adapter.cc) on KeyFrame / MapPoint /
// MapLine test doubles.
//   landmark_harness scene.bin
// scene.bin (little endian): int32 n_kf, n_levels, n_points, n_lines, dim, flags; float level_scale[n_levels];
//   per keyframe: int32 bad; float Ow[3]; int32 n_keys; n_keys x (int32 octave, uint32 desc[8]); int32 n_klines; n_klines x float[dim];
//   per point: int32 bad; float pos[3]; int32 ref_kf; uint32 desc[8]; float normal[3], min, max (the values before the call);
//     int32 n_obs; n_obs x (int32 kf, int32 idx);
//   per line: int32 bad; float desc[dim] (before the call); int32 n_obs; n_obs x (int32 kf, int32 idx).
// The keyframes live in one array, so the std::map<KeyFrame*,size_t> of a landmark iterates in keyframe index order.
// Output: "R points_written lines_written"; per point "P i" and as hex bits mDescriptor (8), mNormalVector (3), mfMinDistance,
//   mfMaxDistance after the call; per line "L i" and mDescriptor (dim) as hex bits.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../adapters/lld_landmark_adapter.h"

using namespace lld_slam;

template <class T> static bool rd(FILE* f, T* x, size_t n = 1) { return n == 0 || fread(x, sizeof(T), n, f) == n; }

static void hex(const void* v, int n) {
  unsigned u;
  for (int q = 0; q < n; ++q) { std::memcpy(&u, (const char*)v + 4 * q, 4); printf(" %08x", u); }
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: landmark_harness scene.bin\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n_kf, n_levels, n_points, n_lines, dim, flags;
  if (!rd(f, &n_kf) || !rd(f, &n_levels) || !rd(f, &n_points) || !rd(f, &n_lines) || !rd(f, &dim) || !rd(f, &flags)) return 2;
  std::vector<float> scale(n_levels);
  if (!rd(f, scale.data(), scale.size())) return 2;
  std::vector<KeyFrame> kfs(n_kf);
  for (int k = 0; k < n_kf; ++k) {
    KeyFrame& K = kfs[k];
    int32_t bad, nk, nl; float ow[3];
    if (!rd(f, &bad) || !rd(f, ow, 3) || !rd(f, &nk)) return 2;
    K.mnId = k; K.mbBad = bad != 0; K.Ow = Mat(3, 1, ow);
    K.mnScaleLevels = n_levels; K.mvScaleFactors = scale;
    K.mvKeysUn.resize(nk); K.mDescriptors = MatU8(nk, 32);
    for (int i = 0; i < nk; ++i) {
      int32_t oct;
      if (!rd(f, &oct) || !rd(f, K.mDescriptors.ptr<uint32_t>(i), 8)) return 2;
      K.mvKeysUn[i].octave = oct;
    }
    if (!rd(f, &nl)) return 2;
    K.mDescriptorsLines = Mat(nl, dim);
    if (!rd(f, K.mDescriptorsLines.ptr<float>(), (size_t)nl * dim)) return 2;
  }
  std::vector<MapPoint> pts(n_points);
  std::vector<MapPoint*> vpMapPoints(n_points);
  for (int i = 0; i < n_points; ++i) {
    MapPoint& P = pts[i];
    int32_t bad, ref, no; float pos[3], nrm[3], mn, mx;
    P.mDescriptor = MatU8(1, 32);
    if (!rd(f, &bad) || !rd(f, pos, 3) || !rd(f, &ref) || !rd(f, P.mDescriptor.ptr<uint32_t>(), 8) || !rd(f, nrm, 3) || !rd(f, &mn) ||
        !rd(f, &mx) || !rd(f, &no))
      return 2;
    P.mnId = i; P.mbBad = bad != 0; P.mWorldPos = Mat(3, 1, pos); P.mpRefKF = &kfs[ref];
    P.mNormalVector = Mat(3, 1, nrm); P.mfMinDistance = mn; P.mfMaxDistance = mx;
    for (int o = 0; o < no; ++o) {
      int32_t kf, idx;
      if (!rd(f, &kf) || !rd(f, &idx)) return 2;
      P.mObservations[&kfs[kf]] = (size_t)idx;
    }
    vpMapPoints[i] = &P;
  }
  std::vector<MapLine> lines(n_lines);
  std::vector<MapLine*> vpMapLines(n_lines);
  for (int i = 0; i < n_lines; ++i) {
    MapLine& L = lines[i];
    int32_t bad, no;
    L.mDescriptor = Mat(1, dim);
    if (!rd(f, &bad) || !rd(f, L.mDescriptor.ptr<float>(), dim) || !rd(f, &no)) return 2;
    L.mnId = i; L.mbBad = bad != 0;
    for (int o = 0; o < no; ++o) {
      int32_t kf, idx;
      if (!rd(f, &kf) || !rd(f, &idx)) return 2;
      L.mObservations[&kfs[kf]] = (size_t)idx;
    }
    vpMapLines[i] = &L;
  }
  fclose(f);
  try {
    lld_amd::Context ctx(0);
    const int wp = lld_adapter::RefreshMapPoints(ctx, vpMapPoints, (unsigned)flags);
    const int wl = lld_adapter::ComputeDistinctiveDescriptors(ctx, vpMapLines);
    printf("R %d %d\n", wp, wl);
    for (int i = 0; i < n_points; ++i) {
      const MapPoint& P = pts[i];
      printf("P %d", i);
      hex(P.mDescriptor.ptr<uint32_t>(), 8); hex(P.mNormalVector.ptr<float>(), 3); hex(&P.mfMinDistance, 1); hex(&P.mfMaxDistance, 1);
      printf("\n");
    }
    for (int i = 0; i < n_lines; ++i) {
      printf("L %d", i);
      hex(lines[i].mDescriptor.ptr<float>(), dim);
      printf("\n");
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "landmark_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
