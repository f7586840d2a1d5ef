// C++ caller of the device-built RGB-D / monocular Frame (include/lld_amd.hpp): lld_amd::ORBextractor on one grey image, lld_amd::MonoFrame
// (lld_frame_build_mono: UndistortKeyPoints and ComputeStereoFromRGBD without the keypoints leaving HBM), then the Tracking chain
// TrackWithMotionModel + TrackLocalMap on that frame - the sequence of Tracking::GrabImageRGBD / GrabImageMonocular + Tracking::Track for one frame.
//   frame_mono_harness <scene.bin>
//   scene.bin (written by tests/test_gpu_frame_mono_cpp.py):
//     int32 [16]  cols, rows, nfeatures, n_levels, iniThFAST, minThFAST, n_last, n_mp, n_dist, depth type (-1: no depth image), depth cols,
//                 depth rows, monocular, 0, 0, 0
//     float [16]  scaleFactor, mbf, depth factor, fx, fy, cx, cy, dist[5], th_motion, th_local, 0, 0
//     int32 [1024] ORBextractor::pattern;   u8 grey [rows][cols];   depth pixels [depth rows][depth cols] (float or uint16), none when type = -1
//     double [6]  fx, fy, cx, cy, bf, gamma;   lld_frame_view of the predicted pose;   float [16] Tcw
//     last frame: float pos [n][3], u8 valid [n], int32 octave [n], float angle [n], u32 desc [n][8], u8 has_obs [n], int32 id [n]
//     local map:  float pos [n][3], normal [n][3], max_distance [n], min_distance [n], u32 desc [n][8], u8 has_obs [n], skip [n], int32 id [n]
//   stdout: "N n", "B mnMinX mnMaxX mnMinY mnMaxY" (float bits, hex), one "K k u_un v_un mvuRight mvDepth" per keypoint (float bits, hex) and
//   "P stage pose_qt[7] (double bits, hex) n_inliers n_search n_points" per stage.
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

static uint32_t fbits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s scene.bin\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  std::vector<int32_t> hd, pattern, l_oct, l_id, m_id;
  std::vector<float> fl, Tcw, l_pos, l_ang, m_pos, m_nrm, m_max, m_min;
  std::vector<uint8_t> grey, depth_bytes, l_valid, l_obs, m_obs, m_skip, view_bytes;
  std::vector<double> cam;
  std::vector<uint32_t> l_desc, m_desc;
  bool ok = rd(in, &hd, 16) && rd(in, &fl, 16) && rd(in, &pattern, 1024);
  const int cols = ok ? hd[0] : 0, rows = ok ? hd[1] : 0, n_last = ok ? hd[6] : 0, n_mp = ok ? hd[7] : 0, n_dist = ok ? hd[8] : 0, d_type = ok ? hd[9] : -1;
  const int d_cols = ok ? hd[10] : 0, d_rows = ok ? hd[11] : 0;
  ok = ok && cols > 0 && rows > 0 && n_last >= 0 && n_mp >= 0 && (d_type == -1 || ((d_type == LLD_DEPTH_F32 || d_type == LLD_DEPTH_U16) && d_cols > 0 && d_rows > 0));
  const size_t d_elem = d_type == LLD_DEPTH_U16 ? 2 : 4;
  ok = ok && rd(in, &grey, (size_t)cols * rows) && rd(in, &depth_bytes, d_type < 0 ? 0 : (size_t)d_cols * d_rows * d_elem);
  ok = ok && rd(in, &cam, 6) && rd(in, &view_bytes, sizeof(lld_frame_view)) && rd(in, &Tcw, 16);
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
    lld_amd::ORBextractor ex(ctx, hd[2], fl[0], hd[3], hd[4], hd[5], pattern.data(), cols, rows, 1);
    std::vector<lld_orb_image> images(1);
    images[0] = lld_orb_image{grey.data(), cols, rows, cols, 0};
    const std::vector<lld_amd::ORBFeatures> feats = ex(images);                                     // ORBextractor::operator()
    const int n = feats[0].n();
    const float K[4] = {fl[3], fl[4], fl[5], fl[6]};
    float bounds[4];
    lld_amd::ImageBounds(cols, rows, K, &fl[7], n_dist, bounds);
    lld_depth_image D{depth_bytes.data(), d_cols, d_rows, (int32_t)(d_cols * d_elem), d_type, fl[2], 0};
    std::unique_ptr<lld_amd::TrackedFrame> F = lld_amd::MonoFrame(ex, 0, n, cols, rows, K, &fl[7], n_dist, fl[1], d_type < 0 ? nullptr : &D, nullptr);
    F->params.cam = lld_camera{cam[0], cam[1], cam[2], cam[3], cam[4]};
    F->params.pose.gamma = cam[5];
    F->params.th_motion = fl[12]; F->params.th_local = fl[13]; F->params.monocular = hd[12];
    F->TrackWithMotionModel(view, Tcw.data(), last, l_id.data(), nullptr);
    F->TrackLocalMap(mp, m_id.data(), nullptr);
    lld_amd::TrackRecord s1, s2;
    F->Download(&s1, &s2);                                                                           // the one synchronisation
    std::vector<float> xy, ur, depth;
    F->DownloadKeypoints(xy, ur, depth);
    std::printf("N %d\n", n);
    std::printf("B %08x %08x %08x %08x\n", fbits(bounds[0]), fbits(bounds[1]), fbits(bounds[2]), fbits(bounds[3]));
    for (int k = 0; k < n; k++) std::printf("K %d %08x %08x %08x %08x\n", k, fbits(xy[2 * k]), fbits(xy[2 * k + 1]), fbits(ur[k]), fbits(depth[k]));
    const lld_amd::TrackRecord* recs[2] = {&s1, &s2};
    for (int s = 0; s < 2; s++) {
      std::printf("P %d", s + 1);
      for (int i = 0; i < 7; i++) { uint64_t u; std::memcpy(&u, &recs[s]->r.pose_qt[i], 8); std::printf(" %016" PRIx64, u); }
      std::printf(" %d %d %d\n", recs[s]->r.n_inliers, recs[s]->r.n_search, recs[s]->r.n_points);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "frame_mono_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
