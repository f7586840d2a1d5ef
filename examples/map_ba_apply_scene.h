// map_ba_apply_scene.h — the scene file of map_ba_apply_host_check and of map_ba_harness's `apply` mode: one map as flat tables, the window
// assembled on it and a result to apply (tests/map_ba_apply_scenes.py write_scene writes it), and the answer file both programs write
// (read_answer there reads it).  Little endian, arrays one after the other in the order of read_scene below.
#ifndef LLD_MAP_BA_APPLY_SCENE_H
#define LLD_MAP_BA_APPLY_SCENE_H

#include <cstdio>
#include <stdexcept>
#include <string>

#include "map_ba_apply_host.h"

namespace map_ba_apply_scene {

struct File {
  FILE* f;
  File(const char* path, const char* mode) : f(std::fopen(path, mode)) { if (!f) throw std::runtime_error(std::string("cannot open ") + path); }
  ~File() { std::fclose(f); }
  template <class T> void get(std::vector<T>& v, size_t n) { v.resize(n); if (n && std::fread(v.data(), sizeof(T), n, f) != n) throw std::runtime_error("short read"); }
  template <class T> void put(const std::vector<T>& v) { if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("short write"); }
  template <class T> void put(const T* p, size_t n) { if (n && std::fwrite(p, sizeof(T), n, f) != n) throw std::runtime_error("short write"); }
};

struct Scene {
  std::vector<int32_t> hdr, limits, query;                 // hdr: n_kf n_pt n_ln n_levels n_cams n_local n_points n_pt_obs n_lines n_ln_obs has_refs n_query
  std::vector<double> cam, cam_qt;
  std::vector<float> sigma2;
  std::vector<uint8_t> kf_set, kf_bad, kf_has_keypoints, ln_set, ln_has_row;
  std::vector<uint64_t> kf_key, kf_mn_id;
  std::vector<int32_t> kp_start, kp_point, kl_start, kl_line, kp_octave, kl_octave, pt_obs_start, pt_obs_kf, pt_obs_idx, ln_obs_start, ln_obs_kf, ln_obs_idx;
  std::vector<float> kp_uvr, kl_left, kl_right;
  map_ba_apply_host::Map M;
  map_ba_apply_host::Window W;
  map_ba_apply_host::Result R;
};

inline void rows_of(const std::vector<int32_t>& start, const std::vector<int32_t>& data, map_ba_apply_host::Rows& rows) {
  rows.assign(start.size() - 1, std::vector<int32_t>());
  for (size_t i = 0; i + 1 < start.size(); i++) rows[i].assign(data.begin() + start[i], data.begin() + start[i + 1]);
}

inline void read_scene(const char* path, Scene& S) {
  File r(path, "rb");
  r.get(S.hdr, 12); r.get(S.limits, 10);
  const std::vector<int32_t>& h = S.hdr;
  const size_t nk = h[0], np = h[1], nl = h[2], nlev = h[3], nc = h[4], nloc = h[5], wp = h[6], wpo = h[7], wl = h[8], wlo = h[9];
  map_ba_apply_host::Map& M = S.M;
  M.n_kf = (int)nk; M.n_pt = (int)np; M.n_ln = (int)nl; M.has_refs = h[10] != 0;
  r.get(S.cam, 5); r.get(S.sigma2, nlev); r.get(S.R.level_scale, nlev); r.get(S.query, h[11]);
  r.get(S.kf_set, nk); r.get(S.kf_bad, nk); r.get(M.kf_feat, nk); r.get(S.kf_has_keypoints, nk); r.get(S.kf_key, nk); r.get(S.kf_mn_id, nk); r.get(M.kf_tcw, 16 * nk);
  r.get(S.kp_start, nk + 1); r.get(S.kp_point, S.kp_start[nk]); r.get(S.kl_start, nk + 1); r.get(S.kl_line, S.kl_start[nk]);
  r.get(S.kp_octave, S.kp_start[nk]); r.get(S.kp_uvr, 3 * (size_t)S.kp_start[nk]);
  r.get(S.kl_left, 4 * (size_t)S.kl_start[nk]); r.get(S.kl_right, 4 * (size_t)S.kl_start[nk]); r.get(S.kl_octave, 2 * (size_t)S.kl_start[nk]);
  r.get(M.pt_state, np); r.get(M.pt_pos, 3 * np); r.get(M.pt_nrm, 3 * np); r.get(M.pt_mind, np); r.get(M.pt_maxd, np); r.get(M.pt_nobs, np); r.get(M.pt_ref, np);
  r.get(S.pt_obs_start, np + 1); r.get(S.pt_obs_kf, S.pt_obs_start[np]); r.get(S.pt_obs_idx, S.pt_obs_start[np]);
  r.get(S.ln_set, nl); r.get(M.ln_bad, nl); r.get(S.ln_has_row, nl); r.get(M.ln_x0, 3 * nl); r.get(M.ln_dir, 3 * nl); r.get(M.ln_nobs, nl);
  r.get(S.ln_obs_start, nl + 1); r.get(S.ln_obs_kf, S.ln_obs_start[nl]); r.get(S.ln_obs_idx, S.ln_obs_start[nl]);
  map_ba_apply_host::Window& W = S.W;
  W.n_local = (int)nloc;
  r.get(W.cam_slot, nc); r.get(W.point_slot, wp); r.get(W.pt_obs_start, wp + 1); r.get(W.pt_obs_cam, wpo); r.get(W.line_slot, wl); r.get(W.ln_obs_start, wl + 1);
  r.get(W.ln_obs_cam, wlo);
  r.get(S.cam_qt, 7 * nc); r.get(S.R.tcw, 16 * nloc); r.get(S.R.pt_xyz, 3 * wp); r.get(S.R.line_x0, 3 * wl); r.get(S.R.line_dir, 3 * wl);
  r.get(S.R.pt_obs_outlier, wpo); r.get(S.R.ln_edge_outlier, 2 * wlo); r.get(S.R.line_removed, wl);
  // the map as the host tail holds it
  rows_of(S.kp_start, S.kp_point, M.kf_points); rows_of(S.kl_start, S.kl_line, M.kf_lines);
  rows_of(S.pt_obs_start, S.pt_obs_kf, M.pt_obs_kf); rows_of(S.pt_obs_start, S.pt_obs_idx, M.pt_obs_idx);
  rows_of(S.ln_obs_start, S.ln_obs_kf, M.ln_obs_kf); rows_of(S.ln_obs_start, S.ln_obs_idx, M.ln_obs_idx);
  M.kf_octave.assign(nk, std::vector<int32_t>()); M.kf_uvr.assign(nk, std::vector<float>()); M.kf_kl_right.assign(nk, std::vector<float>()); M.kf_ow.assign(3 * nk, 0.f);
  for (size_t s = 0; s < nk; s++) {
    if (S.kf_has_keypoints[s]) M.kf_octave[s].assign(S.kp_octave.begin() + S.kp_start[s], S.kp_octave.begin() + S.kp_start[s + 1]);
    if (!M.kf_feat[s]) continue;
    M.kf_uvr[s].assign(S.kp_uvr.begin() + 3 * (size_t)S.kp_start[s], S.kp_uvr.begin() + 3 * (size_t)S.kp_start[s + 1]);
    M.kf_kl_right[s].assign(S.kl_right.begin() + 4 * (size_t)S.kl_start[s], S.kl_right.begin() + 4 * (size_t)S.kl_start[s + 1]);
    map_ba_apply_host::centre(&M.kf_tcw[16 * s], &M.kf_ow[3 * s]);
  }
}

inline void put_rows(File& w, const std::vector<int32_t>& start, const std::vector<int32_t>& data) { w.put(start); w.put(data); }
inline void put_rows(File& w, const map_ba_apply_host::Rows& rows) {
  std::vector<int32_t> start(1, 0), data;
  for (size_t i = 0; i < rows.size(); i++) { data.insert(data.end(), rows[i].begin(), rows[i].end()); start.push_back((int32_t)data.size()); }
  put_rows(w, start, data);
}

}  // namespace map_ba_apply_scene

#endif
