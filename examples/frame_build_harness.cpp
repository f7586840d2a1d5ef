// C++ caller of the device-built stereo Frame (include/lld_amd.hpp): lld_amd::ORBextractor on an image pair, lld_amd::StereoFrame
// (lld_frame_build_stereo: ComputeStereoMatches and the resident frame without the keypoints leaving HBM), then the Tracking chain
// TrackWithMotionModel + TrackLocalMap on that frame - the sequence of Tracking::GrabImageStereo + Tracking::Track for one frame.
//   frame_build_harness <scene.bin>
//   scene.bin (written by tests/test_gpu_frame_build_cpp.py):
//     int32 [12]  cols, rows, nfeatures, n_levels, iniThFAST, minThFAST, n_last, n_mp, repeats, 0, 0, 0
//     float [3]   scaleFactor, mb, mbf;   int32 [1024] ORBextractor::pattern;   u8 left [rows][cols], right [rows][cols]
//     double [6]  fx, fy, cx, cy, bf, gamma;   lld_frame_view of the predicted pose;   float [16] Tcw
//     last frame: float pos [n][3], u8 valid [n], int32 octave [n], float angle [n], u32 desc [n][8], u8 has_obs [n], int32 id [n]
//     local map:  float pos [n][3], normal [n][3], max_distance [n], min_distance [n], u32 desc [n][8], u8 has_obs [n], skip [n], int32 id [n]
//   stdout: "N n_left n_matches", one "S k mvuRight mvDepth" per keypoint (float bits, hex), "P stage pose_qt[7] (double bits, hex) n_inliers
//   n_search n_points" per stage, and with repeats > 0 "T median q1 q3" in milliseconds of image pair -> final pose (extract, build, chain, download).
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lld_amd.hpp"

template <class T>
static bool rd(FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s scene.bin\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<int32_t> hd, pattern, l_oct, l_id, m_id;
  std::vector<float> fl, Tcw, l_pos, l_ang, m_pos, m_nrm, m_max, m_min;
  std::vector<uint8_t> left, right, l_valid, l_obs, m_obs, m_skip, view_bytes;
  std::vector<double> cam;
  std::vector<uint32_t> l_desc, m_desc;
  bool ok = rd(in, &hd, 12) && rd(in, &fl, 3) && rd(in, &pattern, 1024);
  const int cols = ok ? hd[0] : 0, rows = ok ? hd[1] : 0, n_last = ok ? hd[6] : 0, n_mp = ok ? hd[7] : 0, repeats = ok ? hd[8] : 0;
  ok = ok && cols > 0 && rows > 0 && n_last >= 0 && n_mp >= 0;
  ok = ok && rd(in, &left, (size_t)cols * rows) && rd(in, &right, (size_t)cols * rows) && rd(in, &cam, 6) && rd(in, &view_bytes, sizeof(lld_frame_view)) && rd(in, &Tcw, 16);
  ok = ok && rd(in, &l_pos, (size_t)n_last * 3) && rd(in, &l_valid, n_last) && rd(in, &l_oct, n_last) && rd(in, &l_ang, n_last) && rd(in, &l_desc, (size_t)n_last * 8) &&
       rd(in, &l_obs, n_last) && rd(in, &l_id, n_last);
  ok = ok && rd(in, &m_pos, (size_t)n_mp * 3) && rd(in, &m_nrm, (size_t)n_mp * 3) && rd(in, &m_max, n_mp) && rd(in, &m_min, n_mp) && rd(in, &m_desc, (size_t)n_mp * 8) &&
       rd(in, &m_obs, n_mp) && rd(in, &m_skip, n_mp) && rd(in, &m_id, n_mp);
  std::fclose(in);
  if (!ok) { std::fprintf(stderr, "short or malformed scene file\n"); return 2; }
  lld_frame_view view;
  std::memcpy(&view, view_bytes.data(), sizeof(view));
  lld_last_frame_points last{};
  last.n = n_last; last.world_pos = l_pos.data(); last.valid = l_valid.data(); last.octave = l_oct.data(); last.angle = l_ang.data();
  last.desc = l_desc.data(); last.has_obs = l_obs.data();
  lld_map_points mp{};
  mp.n = n_mp; mp.world_pos = m_pos.data(); mp.normal = m_nrm.data(); mp.max_distance = m_max.data(); mp.min_distance = m_min.data();
  mp.desc = m_desc.data(); mp.has_obs = m_obs.data(); mp.skip = m_skip.data();
  try {
    lld_amd::Context ctx(0);
    lld_amd::ORBextractor ex(ctx, hd[2], fl[0], hd[3], hd[4], hd[5], pattern.data(), cols, rows, 2);
    std::vector<lld_orb_image> images(2);
    images[0] = lld_orb_image{left.data(), cols, rows, cols, 0};
    images[1] = lld_orb_image{right.data(), cols, rows, cols, 0};
    std::vector<float> ur, depth;
    lld_amd::TrackRecord s1, s2;
    int n_left = 0, n_matches = 0;
    std::vector<double> ms;
    for (int it = 0; it < std::max(repeats, 1); it++) {
      const auto t0 = std::chrono::steady_clock::now();
      const std::vector<lld_amd::ORBFeatures> feats = ex(images);                                   // ORBextractor::operator() on both images
      n_left = feats[0].n();
      std::unique_ptr<lld_amd::TrackedFrame> F = lld_amd::StereoFrame(ex, 0, 1, n_left, cols, rows, fl[1], fl[2], nullptr);
      F->params.cam = lld_camera{cam[0], cam[1], cam[2], cam[3], cam[4]};
      F->params.pose.gamma = cam[5];
      F->TrackWithMotionModel(view, Tcw.data(), last, l_id.data(), nullptr);
      F->TrackLocalMap(mp, m_id.data(), nullptr);
      F->Download(&s1, &s2);                                                                         // the one synchronisation
      ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
      n_matches = F->DownloadStereo(ur, depth);
    }
    std::printf("N %d %d\n", n_left, n_matches);
    for (int k = 0; k < n_left; k++) {
      uint32_t a, b;
      std::memcpy(&a, &ur[k], 4); std::memcpy(&b, &depth[k], 4);
      std::printf("S %d %08x %08x\n", k, a, b);
    }
    const lld_amd::TrackRecord* recs[2] = {&s1, &s2};
    for (int s = 0; s < 2; s++) {
      std::printf("P %d", s + 1);
      for (int i = 0; i < 7; i++) { uint64_t u; std::memcpy(&u, &recs[s]->r.pose_qt[i], 8); std::printf(" %016" PRIx64, u); }
      std::printf(" %d %d %d\n", recs[s]->r.n_inliers, recs[s]->r.n_search, recs[s]->r.n_points);
    }
    if (repeats > 0) {
      std::sort(ms.begin(), ms.end());
      std::printf("T %.6f %.6f %.6f\n", ms[ms.size() / 2], ms[ms.size() / 4], ms[(3 * ms.size()) / 4]);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "frame_build_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
