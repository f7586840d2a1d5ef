// map_refresh_harness — the landmark refresh on the resident map through include/lld_amd.hpp: a small map written out by formula (the
// same formulas as tests/test_gpu_map_refresh_cpp.py, which builds it through the Python wrapper), then lld_amd::DeviceMap's
// SetKeyFrameDescriptors / SetKeyFrameLineDescriptors / RefreshPoints / RefreshLines / DownloadPoints / DownloadLines.  Prints every output
// as integers (floats as their bit patterns), one array per line, for a comparison member by member.
//
//   keyframe s (0 .. 4)   order_key 100 - 7 s (stored rows run 4, 3, .., 0), bad: s == 3; point row (i + s) % 6, line row (0, 1) or (1, 0) for odd s;
//                         octave of keypoint i: (i + s) % 4; pose: identity rotation, centre (s + 1, s / 2, s / 4)
//   point p (0 .. 5)      (p / 2, 1 + p, 5 + p / 4), seen by the keyframes with (s + p) % 3 != 0, mpRefKF = p % 5
//   line l (0, 1)         seen by every keyframe
//   descriptor word w of keypoint i of keyframe s: a hash of (s, i, w); line descriptor float c of keyline j: ((31 s + 17 j + 7 c) % 23) * 1.5
//
//   map_refresh_harness formula                 the above
//   map_refresh_harness objects scene.bin       two identical object graphs (the file of examples/landmark_harness.cpp): one through
//                                               adapters/lld_map_adapter.cc's MapOnDevice::RefreshMapPoints / ComputeDistinctiveDescriptors, one
//                                               through adapters/lld_landmark_adapter.cc; both printed member by member, and the map's rows
//   map_refresh_harness time scene.bin reps     the host clock around both routes on objects, the second followed by MapOnDevice::UpdatePoints /
//                                               UpdateLines, alternating; prints one JSON line
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../adapters/lld_landmark_adapter.h"
#include "../adapters/lld_map_adapter.h"
#include "lld_amd.hpp"

static const int kKf = 5, kPts = 6, kLns = 2, kDim = 8;

static uint32_t word(int s, int i, int w) {
  uint32_t h = (uint32_t)s * 2654435761u + (uint32_t)i * 40503u + (uint32_t)w * 97u + 1u;
  h *= 2246822519u; h ^= h >> 15; h *= 3266489917u; h ^= h >> 13;
  return h;
}
static void put(const char* name, const std::vector<int64_t>& v) {
  std::printf("%s", name);
  for (size_t i = 0; i < v.size(); i++) std::printf(" %lld", (long long)v[i]);
  std::printf("\n");
}
template <class T> static std::vector<int64_t> ints(const std::vector<T>& v) { return std::vector<int64_t>(v.begin(), v.end()); }
static std::vector<int64_t> bits(const std::vector<float>& v) {
  std::vector<int64_t> r;
  for (size_t i = 0; i < v.size(); i++) { uint32_t b; std::memcpy(&b, &v[i], 4); r.push_back(b); }
  return r;
}

static int formula() {
  try {
    lld_amd::Context ctx(0);
    lld_map_limits L{};
    L.max_keyframes = kKf; L.max_points = kPts; L.max_lines = kLns; L.line_dim = kDim; L.max_observations = 64; L.max_kf_points = 64; L.max_kf_lines = 32;
    L.max_children = 4; L.max_local_points = 8; L.max_local_lines = 2;
    lld_amd::DeviceMap dm(ctx, L);
    lld_amd::DeviceMap::KeyFrameRows K;
    lld_amd::DeviceMap::KeyFrameFeatures F;
    std::vector<int32_t> kp_start(1, 0), kl_start(1, 0), octave; std::vector<float> depth, th(kKf, 0.f), ldesc; std::vector<uint32_t> desc;
    K.cov_start.assign(kKf + 1, 0); K.child_start.assign(kKf + 1, 0); K.point_start.push_back(0); K.line_start.push_back(0);
    for (int s = 0; s < kKf; s++) {
      K.slot.push_back(s); K.order_key.push_back(100 - 7 * s); K.bad.push_back(s == 3); K.parent.push_back(-1);
      for (int i = 0; i < kPts; i++) {
        K.point.push_back((i + s) % kPts); octave.push_back((i + s) % 4); depth.push_back(0.f);
        for (int w = 0; w < 8; w++) desc.push_back(word(s, i, w));
        F.kp_uvr.push_back(0.f); F.kp_uvr.push_back(0.f); F.kp_uvr.push_back(0.f);
      }
      for (int j = 0; j < kLns; j++) {
        K.line.push_back(s % 2 ? 1 - j : j);
        for (int c = 0; c < kDim; c++) ldesc.push_back((float)((31 * s + 17 * j + 7 * c) % 23) * 1.5f);
        for (int c = 0; c < 4; c++) { F.kl_left.push_back(0.f); F.kl_right.push_back(0.f); }
        F.kl_octave.push_back(0); F.kl_octave.push_back(0);
      }
      K.point_start.push_back((int32_t)K.point.size()); K.line_start.push_back((int32_t)K.line.size());
      kp_start.push_back((s + 1) * kPts); kl_start.push_back((s + 1) * kLns);
      F.slot.push_back(s); F.mn_id.push_back(s + 1);
      const float T[16] = {1, 0, 0, -(float)(s + 1), 0, 1, 0, -0.5f * s, 0, 0, 1, -0.25f * s, 0, 0, 0, 1};
      F.Tcw.insert(F.Tcw.end(), T, T + 16);
    }
    F.kp_start = kp_start; F.kl_start = kl_start;
    dm.SetKeyFrames(K);
    dm.SetKeyFrameKeypoints(K.slot, kp_start, octave, depth, th);
    dm.SetKeyFrameFeatures(F);
    std::vector<int32_t> pts, start(1, 0), okf, oidx, nobs, ref; std::vector<float> pos, zero3(3 * kPts, 0.f), zero(kPts, 0.f); std::vector<uint32_t> zdesc(8 * kPts, 0); std::vector<uint8_t> pbad(kPts, 0);
    for (int p = 0; p < kPts; p++) {
      pts.push_back(p); ref.push_back(p % kKf);
      pos.push_back(0.5f * p); pos.push_back(1.f + p); pos.push_back(5.f + 0.25f * p);
      for (int s = kKf - 1; s >= 0; s--) if ((s + p) % 3 != 0) { okf.push_back(s); oidx.push_back(((p - s) % kPts + kPts) % kPts); }
      start.push_back((int32_t)okf.size()); nobs.push_back(start[p + 1] - start[p]);
    }
    dm.SetPoints(pts, pos.data(), zero3.data(), zero.data(), zero.data(), zdesc.data(), pbad.data());
    dm.SetObservationsIndexed(pts, start, okf, oidx, nobs);
    dm.SetPointRefs(pts, ref);
    std::vector<int32_t> lns, lstart(1, 0), lkf, lidx, lnobs; std::vector<double> z3(3 * kLns, 0.0); std::vector<float> zl(kDim * kLns, 0.f); std::vector<uint8_t> lbad(kLns, 0);
    for (int l = 0; l < kLns; l++) {
      lns.push_back(l);
      for (int s = kKf - 1; s >= 0; s--) { lkf.push_back(s); lidx.push_back(s % 2 ? 1 - l : l); }
      lstart.push_back((int32_t)lkf.size()); lnobs.push_back(2 * kKf);
    }
    dm.SetLines(lns, z3.data(), z3.data(), z3.data(), z3.data(), zl.data(), lbad.data());
    dm.SetLineObservations(lns, lstart, lkf, lidx, lnobs);
    dm.SetKeyFrameDescriptors(K.slot, kp_start, desc);
    dm.SetKeyFrameLineDescriptors(K.slot, kl_start, ldesc);
    const std::vector<float> scale{1.f, 1.2f, 1.44f, 1.728f};
    const std::vector<int32_t> query{4, 1, 5, 0, 3, 2};
    const lld_amd::DeviceMap::RefreshedPoints rp = dm.RefreshPoints(query, LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH, scale);
    const lld_amd::DeviceMap::RefreshedLines rl = dm.RefreshLines(std::vector<int32_t>{1, 0});
    const lld_amd::DeviceMap::PointRows held = dm.DownloadPoints(pts);
    const lld_amd::DeviceMap::LineRows lheld = dm.DownloadLines(lns);
    put("p_updated", ints(rp.updated)); put("p_best_obs", ints(rp.best_obs)); put("p_best_median", ints(rp.best_median)); put("p_desc", ints(rp.desc));
    put("p_normal", bits(rp.normal)); put("p_min", bits(rp.min_distance)); put("p_max", bits(rp.max_distance));
    put("l_updated", ints(rl.updated)); put("l_best_obs", ints(rl.best_obs)); put("l_best_median", ints(rl.best_median)); put("l_desc", bits(rl.desc));
    put("t_pos", bits(held.pos)); put("t_normal", bits(held.normal)); put("t_min", bits(held.min_distance)); put("t_max", bits(held.max_distance));
    put("t_desc", ints(held.desc)); put("t_state", ints(held.state)); put("t_ldesc", bits(lheld.desc)); put("t_lbad", ints(lheld.bad));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "map_refresh_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ the object graph (landmark_harness's scene.bin)
using namespace lld_slam;

struct Graph {
  int32_t n_kf = 0, n_levels = 0, n_points = 0, n_lines = 0, dim = 0, flags = 0;
  std::vector<KeyFrame> kfs; std::vector<MapPoint> pts; std::vector<MapLine> lines;
  std::vector<KeyFrame*> vpKFs; std::vector<MapPoint*> vpMapPoints; std::vector<MapLine*> vpMapLines;
};
template <class T> static bool rd(FILE* f, T* x, size_t n = 1) { return n == 0 || fread(x, sizeof(T), n, f) == n; }

// The graph of examples/landmark_harness.cpp's file, with what MapOnDevice reads on top: the match rows of every keyframe (the point or line
// at the observed index) and a pose whose camera centre is the file's Ow (identity rotation, translation -Ow).
static bool load(const char* path, Graph& G) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  if (!rd(f, &G.n_kf) || !rd(f, &G.n_levels) || !rd(f, &G.n_points) || !rd(f, &G.n_lines) || !rd(f, &G.dim) || !rd(f, &G.flags)) return false;
  std::vector<float> scale(G.n_levels);
  if (!rd(f, scale.data(), scale.size())) return false;
  G.kfs.resize(G.n_kf); G.pts.resize(G.n_points); G.lines.resize(G.n_lines);
  for (int k = 0; k < G.n_kf; ++k) {
    KeyFrame& K = G.kfs[k];
    int32_t bad, nk, nl; float ow[3];
    if (!rd(f, &bad) || !rd(f, ow, 3) || !rd(f, &nk)) return false;
    K.mnId = k; K.mbBad = bad != 0; K.Ow = Mat(3, 1, ow);
    K.Tcw = Mat(4, 4);
    for (int r = 0; r < 4; ++r) K.Tcw.at<float>(r, r) = 1.f;
    for (int r = 0; r < 3; ++r) K.Tcw.at<float>(r, 3) = -ow[r];
    K.mnScaleLevels = G.n_levels; K.mvScaleFactors = scale;
    K.mvKeysUn.resize(nk); K.mDescriptors = MatU8(nk, 32); K.mvpMapPoints.assign(nk, nullptr);
    for (int i = 0; i < nk; ++i) {
      int32_t oct;
      if (!rd(f, &oct) || !rd(f, K.mDescriptors.ptr<uint32_t>(i), 8)) return false;
      K.mvKeysUn[i].octave = oct;
    }
    if (!rd(f, &nl)) return false;
    K.mDescriptorsLines = Mat(nl, G.dim); K.mvpMapLines.assign(nl, nullptr);
    if (!rd(f, K.mDescriptorsLines.ptr<float>(), (size_t)nl * G.dim)) return false;
    G.vpKFs.push_back(&K);
  }
  for (int i = 0; i < G.n_points; ++i) {
    MapPoint& P = G.pts[i];
    int32_t bad, ref, no; float pos[3], nrm[3], mn, mx;
    P.mDescriptor = MatU8(1, 32);
    if (!rd(f, &bad) || !rd(f, pos, 3) || !rd(f, &ref) || !rd(f, P.mDescriptor.ptr<uint32_t>(), 8) || !rd(f, nrm, 3) || !rd(f, &mn) || !rd(f, &mx) || !rd(f, &no)) return false;
    P.mnId = i; P.mbBad = bad != 0; P.mWorldPos = Mat(3, 1, pos); P.mpRefKF = &G.kfs[ref];
    P.mNormalVector = Mat(3, 1, nrm); P.mfMinDistance = mn; P.mfMaxDistance = mx;
    for (int o = 0; o < no; ++o) {
      int32_t kf, idx;
      if (!rd(f, &kf) || !rd(f, &idx)) return false;
      P.mObservations[&G.kfs[kf]] = (size_t)idx; P.nObs++;
      G.kfs[kf].mvpMapPoints[idx] = &P;
    }
    G.vpMapPoints.push_back(&P);
  }
  for (int i = 0; i < G.n_lines; ++i) {
    MapLine& L = G.lines[i];
    int32_t bad, no;
    L.mDescriptor = Mat(1, G.dim);
    if (!rd(f, &bad) || !rd(f, L.mDescriptor.ptr<float>(), G.dim) || !rd(f, &no)) return false;
    L.mnId = i; L.mbBad = bad != 0;
    for (int o = 0; o < no; ++o) {
      int32_t kf, idx;
      if (!rd(f, &kf) || !rd(f, &idx)) return false;
      L.mObservations[&G.kfs[kf]] = (size_t)idx;
      G.kfs[kf].mvpMapLines[idx] = &L;
    }
    G.vpMapLines.push_back(&L);
  }
  fclose(f);
  return true;
}

static lld_map_limits limits_of(const Graph& G) {
  size_t kp = 0, kl = 0, ob = 0;
  for (const KeyFrame& K : G.kfs) { kp += K.mvpMapPoints.size(); kl += K.mvpMapLines.size(); }
  for (const MapPoint& P : G.pts) ob += P.mObservations.size();
  lld_map_limits L{};
  L.max_keyframes = G.n_kf; L.max_points = G.n_points > 0 ? G.n_points : 1; L.max_lines = G.n_lines; L.line_dim = G.dim; L.max_observations = (int32_t)ob + 8;
  L.max_kf_points = (int32_t)kp + 8; L.max_kf_lines = (int32_t)kl + 8; L.max_children = 8; L.max_local_points = 64; L.max_local_lines = 16;
  return L;
}

static void hex(const void* v, int n) {
  unsigned u;
  for (int q = 0; q < n; ++q) { std::memcpy(&u, (const char*)v + 4 * q, 4); std::printf(" %08x", u); }
}
static void print(const char* tag, const Graph& G, int wp, int wl) {
  std::printf("%s R %d %d\n", tag, wp, wl);
  for (int i = 0; i < G.n_points; ++i) {
    const MapPoint& P = G.pts[i];
    std::printf("%s P %d", tag, i);
    hex(P.mDescriptor.ptr<uint32_t>(), 8); hex(P.mNormalVector.ptr<float>(), 3); hex(&P.mfMinDistance, 1); hex(&P.mfMaxDistance, 1);
    std::printf("\n");
  }
  for (int i = 0; i < G.n_lines; ++i) { std::printf("%s L %d", tag, i); hex(G.lines[i].mDescriptor.ptr<float>(), G.dim); std::printf("\n"); }
}
static void upload(lld_adapter::MapOnDevice& M, Graph& G) {
  M.EnableRefresh();
  M.UpdateKeyFrames(G.vpKFs); M.UpdatePoints(G.vpMapPoints); M.UpdateLines(G.vpMapLines);
}

// objects: graph A through MapOnDevice::RefreshMapPoints / ComputeDistinctiveDescriptors, an identical graph B through the gathering adapter
// (adapters/lld_landmark_adapter.cc); both printed member by member ("A ..." and "B ..." lines), then graph A's map as the device holds it
// ("T ..." lines: what a second upload of graph A's objects would send).
static int objects(const char* path) {
  Graph A, B;
  if (!load(path, A) || !load(path, B)) return 2;
  try {
    lld_amd::Context ctx(0);
    lld_adapter::MapOnDevice M(ctx.get(), limits_of(A));
    upload(M, A);
    const int wa = M.RefreshMapPoints(A.vpMapPoints, (unsigned)A.flags), la = M.ComputeDistinctiveDescriptors(A.vpMapLines);
    const int wb = lld_adapter::RefreshMapPoints(ctx, B.vpMapPoints, (unsigned)B.flags), lb = lld_adapter::ComputeDistinctiveDescriptors(ctx, B.vpMapLines);
    print("A", A, wa, la); print("B", B, wb, lb);
    std::vector<int32_t> ps(A.n_points), ls(A.n_lines);
    for (int i = 0; i < A.n_points; ++i) ps[i] = i;
    for (int i = 0; i < A.n_lines; ++i) ls[i] = i;
    std::vector<float> nrm(3 * ps.size() + 1), mn(ps.size() + 1), mx(ps.size() + 1), ld((size_t)A.dim * ls.size() + 1); std::vector<uint32_t> d(8 * ps.size() + 1);
    if (lld_map_download_points(M.get(), A.n_points, ps.data(), nullptr, nrm.data(), mn.data(), mx.data(), d.data(), nullptr) != LLD_OK) return 1;
    if (lld_map_download_lines(M.get(), A.n_lines, ls.data(), ld.data(), nullptr) != LLD_OK) return 1;
    for (int i = 0; i < A.n_points; ++i) { std::printf("T P %d", i); hex(&d[8 * i], 8); hex(&nrm[3 * i], 3); hex(&mn[i], 1); hex(&mx[i], 1); std::printf("\n"); }
    for (int i = 0; i < A.n_lines; ++i) { std::printf("T L %d", i); hex(&ld[(size_t)A.dim * i], A.dim); std::printf("\n"); }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "map_refresh_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}

// time: the host clock around (a) MapOnDevice::RefreshMapPoints + ComputeDistinctiveDescriptors and (b) the gathering adapter followed by
// MapOnDevice::UpdatePoints / UpdateLines (the results sent back into the map), alternating, on two identical graphs with a map each.
static int time_routes(const char* path, int reps) {
  Graph A, B;
  if (!load(path, A) || !load(path, B)) return 2;
  try {
    lld_amd::Context ctx(0);
    lld_adapter::MapOnDevice MA(ctx.get(), limits_of(A)), MB(ctx.get(), limits_of(B));
    upload(MA, A); upload(MB, B);
    std::vector<double> ta, tb;
    int wa = 0, wb = 0;
    for (int r = -5; r < reps; ++r) {
      const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
      wa = MA.RefreshMapPoints(A.vpMapPoints, (unsigned)A.flags) + MA.ComputeDistinctiveDescriptors(A.vpMapLines);
      const std::chrono::steady_clock::time_point t1 = std::chrono::steady_clock::now();
      wb = lld_adapter::RefreshMapPoints(ctx, B.vpMapPoints, (unsigned)B.flags) + lld_adapter::ComputeDistinctiveDescriptors(ctx, B.vpMapLines);
      MB.UpdatePoints(B.vpMapPoints); MB.UpdateLines(B.vpMapLines);
      lld_ctx_synchronize(ctx.get());
      const std::chrono::steady_clock::time_point t2 = std::chrono::steady_clock::now();
      if (r >= 0) { ta.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count()); tb.push_back(std::chrono::duration<double, std::milli>(t2 - t1).count()); }
    }
    std::printf("{\"points\": %d, \"lines\": %d, \"written_map\": %d, \"written_adapter\": %d, \"map_route_ms\": [", A.n_points, A.n_lines, wa, wb);
    for (size_t i = 0; i < ta.size(); i++) std::printf("%s%.4f", i ? ", " : "", ta[i]);
    std::printf("], \"adapter_and_update_ms\": [");
    for (size_t i = 0; i < tb.size(); i++) std::printf("%s%.4f", i ? ", " : "", tb[i]);
    std::printf("]}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "map_refresh_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "formula")) return formula();
  if (argc == 3 && !std::strcmp(argv[1], "objects")) return objects(argv[2]);
  if (argc == 4 && !std::strcmp(argv[1], "time")) return time_routes(argv[2], std::atoi(argv[3]));
  std::fprintf(stderr, "usage: map_refresh_harness formula | objects scene.bin | time scene.bin reps\n");
  return 2;
}
