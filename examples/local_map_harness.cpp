// local_map_harness.cpp — one frame of the Tracking chain with Tracking::UpdateLocalMap between its stages, from compiled C++ over
// include/lld_amd.hpp, two ways:
//   resident  lld_amd::DeviceMap filled from the map file; TrackWithMotionModel -> TrackedFrame::UpdateLocalMap -> TrackLocalMapResident ->
//             DownloadLocalMap (the frame's one download);
//   host      TrackWithMotionModel -> Download -> the two loops of UpdateLocalMap on flat tables (local_map_host.cpp) -> the local points and
//             lines gathered into arrays -> TrackLocalMap -> Download.
// Input: a track scene as examples/harness.cpp's `track` mode reads it (lld_slam_amd.tracking.write_harness_scene; its local map is not
// read: the map file names it) and a map file (tests/local_map_scenes.py write_map_file).  Output: UpdateLocalMap's record, the three
// lists and mp_in_view of the resident route, then both stage records of the resident and of the host route, and the host route's lists.
// tests/test_gpu_local_map_cpp.py compares them with the Python wrapper's.  Exit code 3 when the two routes of this program differ.
// With `objects` in front: the same comparison on live object doubles through the adapters (local_map_objects.cpp).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "local_map_harness.h"
#include "local_map_host.h"
#include "lld_amd.hpp"

namespace {

struct Reader {
  std::FILE* f;
  explicit Reader(const char* p) : f(std::fopen(p, "rb")) { if (!f) throw std::runtime_error(std::string("cannot open ") + p); }
  ~Reader() { std::fclose(f); }
  template <class T> void get(T* p, size_t n) { if (n && std::fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short read"); }
  template <class T> void get(std::vector<T>& v, size_t n) { v.resize(n); get(v.data(), n); }
};
struct Writer {
  std::FILE* f;
  explicit Writer(const char* p) : f(std::fopen(p, "wb")) { if (!f) throw std::runtime_error(std::string("cannot open ") + p); }
  ~Writer() { std::fclose(f); }
  template <class T> void put(const T* p, size_t n) { if (n && std::fwrite(p, sizeof(T), n, f) != n) throw std::runtime_error("short write"); }
  template <class T> void put(const std::vector<T>& v) { put(v.data(), v.size()); }
};

void put_record(Writer& w, const lld_amd::TrackRecord& rec) {
  w.put(rec.r.pose_qt, 7); w.put(&rec.r.chi2, 1);
  const int32_t c[14] = {rec.r.n_inliers, rec.r.lm_iterations, rec.r.lm_trials, rec.r.n_edges, rec.r.n_search_first, rec.r.n_search, rec.r.used_wide, rec.r.n_points,
                         rec.r.n_points_map, rec.r.n_lines_matched, rec.r.n_lines, rec.r.n_discarded, rec.r.n_point_edges, rec.r.n_in_view};
  w.put(c, 14);
  w.put(rec.kp_point_id); w.put(rec.kp_outlier); w.put(rec.ln_line_id); w.put(rec.ln_outlier);
}
bool same_record(const lld_amd::TrackRecord& a, const lld_amd::TrackRecord& b) {
  return !std::memcmp(a.r.pose_qt, b.r.pose_qt, sizeof a.r.pose_qt) && !std::memcmp(&a.r.chi2, &b.r.chi2, 8) && a.r.n_inliers == b.r.n_inliers && a.r.n_points == b.r.n_points &&
         a.r.n_search == b.r.n_search && a.r.n_lines == b.r.n_lines && a.r.n_in_view == b.r.n_in_view && a.kp_point_id == b.kp_point_id && a.kp_outlier == b.kp_outlier &&
         a.ln_line_id == b.ln_line_id && a.ln_outlier == b.ln_outlier;
}

int run(const char* scene_path, const char* map_path, const char* out_path, bool objects) {
  // ---- the frame and stage 1's inputs (the layout of harness.cpp's run_track)
  Reader r(scene_path);
  int32_t h[16]; r.get(h, 16);
  const int nt = h[0], n_levels = h[1], n_last = h[2], n_mp = h[3], nl = h[4], nr = h[5], dim = h[6], n_ll = h[7], n_ml = h[8];
  float fc[6]; r.get(fc, 6);
  std::vector<float> scale, inv_sigma2; r.get(scale, n_levels); r.get(inv_sigma2, n_levels);
  double dc[8]; r.get(dc, 8);
  std::vector<uint32_t> t_desc; std::vector<float> t_xy, t_ur, t_ang; std::vector<int32_t> t_oct;
  r.get(t_desc, 8 * (size_t)nt); r.get(t_xy, 2 * (size_t)nt); r.get(t_oct, nt); r.get(t_ur, nt); r.get(t_ang, nt);
  lld_frame_view view; r.get(&view, 1);
  float Tcw[16]; r.get(Tcw, 16);
  std::vector<float> l_pos, l_ang; std::vector<uint8_t> l_valid, l_obs; std::vector<int32_t> l_oct, l_id; std::vector<uint32_t> l_desc;
  r.get(l_pos, 3 * (size_t)n_last); r.get(l_valid, n_last); r.get(l_oct, n_last); r.get(l_ang, n_last); r.get(l_desc, 8 * (size_t)n_last); r.get(l_obs, n_last); r.get(l_id, n_last);
  { std::vector<char> skip; r.get(skip, (size_t)n_mp * (12 + 12 + 4 + 4 + 32 + 1 + 1 + 4)); }      // the scene's own local MapPoints: not used here
  std::vector<float> ln_left, ln_right, ln_desc; std::vector<int32_t> ln_lo, ln_ro, ln_lm;
  r.get(ln_left, 4 * (size_t)nl); r.get(ln_lo, nl); r.get(ln_right, 4 * (size_t)nr); r.get(ln_ro, nr); r.get(ln_lm, nl); r.get(ln_desc, (size_t)nl * dim);
  struct LineSet { std::vector<double> x0, dir, x1, x2; std::vector<uint8_t> skip; std::vector<float> desc; std::vector<int32_t> id; lld_map_lines c; };
  auto read_lines = [&](LineSet& L, int n) {
    r.get(L.x0, 3 * (size_t)n); r.get(L.dir, 3 * (size_t)n); r.get(L.x1, 3 * (size_t)n); r.get(L.x2, 3 * (size_t)n); r.get(L.skip, n); r.get(L.desc, (size_t)n * dim); r.get(L.id, n);
    L.c = lld_map_lines{n, L.x0.data(), L.dir.data(), L.x1.data(), L.x2.data(), L.skip.data(), L.desc.data(), L.id.data()};
  };
  LineSet last_lines, unused_local; read_lines(last_lines, n_ll); read_lines(unused_local, n_ml);
  lld_orb_search kp{};
  kp.nt = nt; kp.t_desc = t_desc.data(); kp.t_xy = t_xy.data(); kp.t_octave = t_oct.data(); kp.t_uright = t_ur.data(); kp.t_angle = t_ang.data();
  kp.grid_min_x = fc[0]; kp.grid_min_y = fc[1]; kp.grid_width_inv = fc[4]; kp.grid_height_inv = fc[5]; kp.grid_cols = 64; kp.grid_rows = 48;
  kp.n_levels = n_levels; kp.level_scale = scale.data(); kp.level_inv_sigma2 = inv_sigma2.data();
  lld_frame_lines fl{};
  fl.n_left = nl; fl.left = ln_left.data(); fl.left_octave = ln_lo.data(); fl.n_right = nr; fl.right = ln_right.data(); fl.right_octave = ln_ro.data();
  fl.line_matches = ln_lm.data(); fl.desc = ln_desc.data(); fl.dim = dim; fl.sx = 1.0 / fc[2]; fl.sy = 1.0 / fc[3];
  lld_last_frame_points last{n_last, l_pos.data(), l_valid.data(), l_oct.data(), l_ang.data(), l_desc.data(), l_obs.data()};

  // ---- the map: limits, flat tables, payload by dense slot
  Reader mr(map_path);
  int32_t lim[10]; mr.get(lim, 10);
  lld_map_limits L{lim[0], lim[1], lim[2], lim[3], lim[4], lim[5], lim[6], lim[7], lim[8], lim[9]};
  const int nk = L.max_keyframes, np = L.max_points, nln = L.max_lines;
  lld_amd::DeviceMap::KeyFrameRows K;
  std::vector<uint8_t> pt_state, ln_bad; std::vector<int32_t> obs_start, obs;
  mr.get(K.order_key, nk); mr.get(K.bad, nk); mr.get(K.parent, nk);
  mr.get(K.cov_start, (size_t)nk + 1); mr.get(K.cov, K.cov_start[nk]); mr.get(K.child_start, (size_t)nk + 1); mr.get(K.child, K.child_start[nk]);
  mr.get(K.point_start, (size_t)nk + 1); mr.get(K.point, K.point_start[nk]); mr.get(K.line_start, (size_t)nk + 1); mr.get(K.line, K.line_start[nk]);
  mr.get(pt_state, np); mr.get(obs_start, (size_t)np + 1); mr.get(obs, obs_start[np]); mr.get(ln_bad, nln);
  std::vector<float> p_pos, p_nrm, p_mind, p_maxd, l_desc_map; std::vector<uint32_t> p_desc; std::vector<double> l_x0, l_dir, l_x1, l_x2;
  mr.get(p_pos, 3 * (size_t)np); mr.get(p_nrm, 3 * (size_t)np); mr.get(p_mind, np); mr.get(p_maxd, np); mr.get(p_desc, 8 * (size_t)np);
  mr.get(l_x0, 3 * (size_t)nln); mr.get(l_dir, 3 * (size_t)nln); mr.get(l_x1, 3 * (size_t)nln); mr.get(l_x2, 3 * (size_t)nln); mr.get(l_desc_map, (size_t)nln * L.line_dim);
  for (int s = 0; s < nk; s++) K.slot.push_back(s);

  lld_amd::Context ctx(0);
  auto new_frame = [&](lld_amd::TrackedFrame& f) {
    f.params.cam = lld_camera{dc[0], dc[1], dc[2], dc[3], dc[4]};
    f.params.pose.gamma = dc[5]; f.params.line_thr_reproj_base = dc[6]; f.params.line_md_thr = dc[7];
  };
  if (objects) {
    // stage 1 on a TrackedFrame; what it left enters the object graphs' frames through SetFrameState (local_map_objects.cpp)
    HarnessInput in;
    in.nt = nt; in.nl = nl; in.nr = nr; in.dim = dim; in.n_levels = n_levels; in.fc = fc; in.dc = dc; in.scale = &scale; in.inv_sigma2 = &inv_sigma2; in.t_xy = &t_xy; in.t_ur = &t_ur;
    in.t_ang = &t_ang; in.ln_left = &ln_left; in.ln_right = &ln_right; in.ln_desc = &ln_desc; in.t_desc = &t_desc; in.t_oct = &t_oct; in.ln_lo = &ln_lo; in.ln_ro = &ln_ro; in.ln_lm = &ln_lm;
    in.log_scale_factor = view.log_scale_factor; in.L = L; in.K = &K; in.pt_state = &pt_state; in.ln_bad = &ln_bad; in.obs_start = &obs_start; in.obs = &obs;
    in.p_pos = &p_pos; in.p_nrm = &p_nrm; in.p_mind = &p_mind; in.p_maxd = &p_maxd; in.l_desc = &l_desc_map; in.p_desc = &p_desc; in.l_x0 = &l_x0; in.l_dir = &l_dir; in.l_x1 = &l_x1; in.l_x2 = &l_x2;
    lld_amd::TrackedFrame frame(ctx, kp, nl > 0 ? &fl : nullptr);
    new_frame(frame);
    frame.TrackWithMotionModel(view, Tcw, last, l_id.data(), n_ll > 0 ? &last_lines.c : nullptr);
    lld_amd::TrackRecord s1; frame.Download(&s1, nullptr);
    in.kp_id.assign(nt, -1); in.ln_id.assign(nl, -1);
    for (int k = 0; k < nt; k++) if (!s1.kp_outlier[k]) in.kp_id[k] = s1.kp_point_id[k];
    for (int i = 0; i < nl; i++) if (!s1.ln_outlier[i]) in.ln_id[i] = s1.ln_line_id[i];
    if (s1.r.n_point_edges >= 3) lld_se3_to_tcw_f32(s1.r.pose_qt, in.Tcw); else std::memcpy(in.Tcw, Tcw, sizeof in.Tcw);
    return run_objects(ctx, in, out_path);
  }
  lld_amd::DeviceMap map(ctx, L);
  map.SetKeyFrames(K);
  {
    // the points the map holds, packed; a slot with state 0 is never set (a temporal point)
    std::vector<int32_t> slot, start(1, 0), flat; std::vector<float> pos, nrm, mind, maxd; std::vector<uint32_t> desc; std::vector<uint8_t> bad;
    for (int s = 0; s < np; s++) {
      if (!pt_state[s]) continue;
      slot.push_back(s); bad.push_back(pt_state[s] == 2); mind.push_back(p_mind[s]); maxd.push_back(p_maxd[s]);
      pos.insert(pos.end(), &p_pos[3 * s], &p_pos[3 * s] + 3); nrm.insert(nrm.end(), &p_nrm[3 * s], &p_nrm[3 * s] + 3); desc.insert(desc.end(), &p_desc[8 * s], &p_desc[8 * s] + 8);
      flat.insert(flat.end(), obs.begin() + obs_start[s], obs.begin() + obs_start[s + 1]); start.push_back((int32_t)flat.size());
    }
    map.SetPoints(slot, pos.data(), nrm.data(), mind.data(), maxd.data(), desc.data(), bad.data());
    map.SetObservations(slot, start, flat);
    std::vector<int32_t> lslot;
    for (int s = 0; s < nln; s++) lslot.push_back(s);
    map.SetLines(lslot, l_x0.data(), l_dir.data(), l_x1.data(), l_x2.data(), l_desc_map.data(), ln_bad.data());
  }

  // ---- resident route
  lld_amd::LocalMapRecord rec; lld_amd::TrackRecord b1, b2;
  {
    lld_amd::TrackedFrame frame(ctx, kp, nl > 0 ? &fl : nullptr);
    new_frame(frame);
    frame.TrackWithMotionModel(view, Tcw, last, l_id.data(), n_ll > 0 ? &last_lines.c : nullptr);
    frame.UpdateLocalMap(map);
    frame.TrackLocalMapResident(map);
    frame.DownloadLocalMap(map, rec, &b1, &b2);
  }
  // ---- host route
  lld_amd::TrackRecord a1, a2; local_map_host::Result R; local_map_host::State S;
  std::vector<uint8_t> in_view_host;
  {
    lld_amd::TrackedFrame frame(ctx, kp, nl > 0 ? &fl : nullptr);
    new_frame(frame);
    frame.TrackWithMotionModel(view, Tcw, last, l_id.data(), n_ll > 0 ? &last_lines.c : nullptr);
    lld_amd::TrackRecord s1; frame.Download(&s1, nullptr);
    std::vector<int32_t> ids(nt);
    for (int k = 0; k < nt; k++) ids[k] = s1.kp_outlier[k] ? -1 : s1.kp_point_id[k];
    local_map_host::Tables T;
    T.n_keyframes = nk; T.n_points = np; T.n_lines = nln; T.kf_key = K.order_key.data(); T.kf_bad = K.bad.data(); T.kf_parent = K.parent.data();
    T.cov_start = K.cov_start.data(); T.cov = K.cov.data(); T.child_start = K.child_start.data(); T.child = K.child.data(); T.point_start = K.point_start.data();
    T.point = K.point.data(); T.line_start = K.line_start.data(); T.line = K.line.data(); T.pt_state = pt_state.data(); T.obs_start = obs_start.data(); T.obs = obs.data();
    T.ln_bad = ln_bad.data();
    local_map_host::update_local_map(T, S, ids.data(), nt, L.max_local_points, L.max_local_lines, R);
    if (R.status) throw std::runtime_error("the host route overflowed: the scene is not meant to");
    const size_t n = R.local_points.size(), m = R.local_lines.size();
    std::vector<float> pos(3 * n), nrm(3 * n), mind(n), maxd(n); std::vector<uint32_t> desc(8 * n); std::vector<uint8_t> has_obs(n);
    for (size_t q = 0; q < n; q++) {
      const int s = R.local_points[q];
      std::memcpy(&pos[3 * q], &p_pos[3 * s], 12); std::memcpy(&nrm[3 * q], &p_nrm[3 * s], 12); std::memcpy(&desc[8 * q], &p_desc[8 * s], 32);
      mind[q] = p_mind[s]; maxd[q] = p_maxd[s]; has_obs[q] = obs_start[s + 1] > obs_start[s];
    }
    std::vector<double> x0(3 * m), dir(3 * m), x1(3 * m), x2(3 * m); std::vector<float> ld(m * (size_t)L.line_dim);
    for (size_t q = 0; q < m; q++) {
      const int s = R.local_lines[q];
      std::memcpy(&x0[3 * q], &l_x0[3 * s], 24); std::memcpy(&dir[3 * q], &l_dir[3 * s], 24); std::memcpy(&x1[3 * q], &l_x1[3 * s], 24); std::memcpy(&x2[3 * q], &l_x2[3 * s], 24);
      std::memcpy(&ld[q * L.line_dim], &l_desc_map[(size_t)s * L.line_dim], (size_t)L.line_dim * 4);
    }
    lld_map_points mp{(int32_t)n, pos.data(), nrm.data(), maxd.data(), mind.data(), desc.data(), has_obs.data(), nullptr};
    lld_map_lines ml{(int32_t)m, x0.data(), dir.data(), x1.data(), x2.data(), nullptr, ld.data(), R.local_lines.data()};
    frame.TrackLocalMap(mp, R.local_points.data(), (m > 0 && nl > 0) ? &ml : nullptr);
    in_view_host.assign(n, 0);
    a2.r.mp_in_view = in_view_host.data();        // (TrackRecord::bind leaves it alone)
    frame.Download(&a1, &a2);
  }
  Writer w(out_path);
  const int32_t head[12] = {rec.r.status, rec.r.n_voted, rec.r.n_local_keyframes, rec.r.n_local_points, rec.r.n_local_lines, rec.r.n_bad_cleared, rec.r.ref_keyframe,
                            rec.r.vote_empty, rec.r.stage2_ran, (int32_t)S.local_keyframes.size(), (int32_t)R.local_points.size(), (int32_t)R.local_lines.size()};
  w.put(head, 12);
  w.put(rec.local_keyframes.data(), rec.r.n_local_keyframes); w.put(rec.local_points.data(), rec.r.n_local_points); w.put(rec.local_lines.data(), rec.r.n_local_lines);
  w.put(rec.mp_in_view);
  put_record(w, b1); put_record(w, b2); put_record(w, a1); put_record(w, a2);
  w.put(S.local_keyframes); w.put(R.local_points); w.put(R.local_lines); w.put(in_view_host);
  bool same = rec.r.status == 0 && rec.r.stage2_ran == 1 && same_record(a1, b1) && same_record(a2, b2) && R.ref_keyframe == rec.r.ref_keyframe &&
              std::vector<int32_t>(rec.local_keyframes.begin(), rec.local_keyframes.begin() + rec.r.n_local_keyframes) == S.local_keyframes &&
              std::vector<int32_t>(rec.local_points.begin(), rec.local_points.begin() + rec.r.n_local_points) == R.local_points &&
              std::vector<int32_t>(rec.local_lines.begin(), rec.local_lines.begin() + rec.r.n_local_lines) == R.local_lines &&
              std::equal(in_view_host.begin(), in_view_host.end(), rec.mp_in_view.begin());
  std::printf("local map: %d keyframes, %d points, %d lines; stage 2 holds %d points; routes %s\n", rec.r.n_local_keyframes, rec.r.n_local_points, rec.r.n_local_lines,
              b2.r.n_points, same ? "equal" : "DIFFER");
  return same ? 0 : 3;
}

}  // namespace

int main(int argc, char** argv) {
  const bool objects = argc == 5 && !std::strcmp(argv[1], "objects");
  if (argc != 4 && !objects) { std::fprintf(stderr, "usage: local_map_harness [objects] <track scene> <map file> <out>\n"); return 2; }
  try {
    return run(argv[1 + objects], argv[2 + objects], argv[3 + objects], objects);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "local_map_harness: %s\n", e.what());
    return 1;
  }
}
