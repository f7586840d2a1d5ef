// map_ba_apply_host.cpp — see map_ba_apply_host.h.  The loops follow src/Optimizer.cc:1334-1386 with MapPoint.cc:111-168, MapLine.cc:77-123
// and MapPoint::UpdateNormalAndDepth (:330-371) behind them; the numerics of the last are those include/lld_amd.h states for
// lld_mappoint_refresh (float cv::Mat arithmetic, cv::norm in double).  Compile without -ffast-math and without FMA contraction.
#include "map_ba_apply_host.h"

#include <algorithm>
#include <cmath>

namespace map_ba_apply_host {

namespace {

double norm3(float x, float y, float z) {
  double s = (double)x * (double)x;
  s += (double)y * (double)y;
  s += (double)z * (double)z;
  return std::sqrt(s);
}

int find(const std::vector<int32_t>& row, int32_t v) {
  for (size_t j = 0; j < row.size(); j++) if (row[j] == v) return (int)j;
  return -1;
}

// mvpMapPoints[idx] = NULL / mvpMapLines[idx] = NULL by index; 1 when the index is outside the row
int erase_match(Rows& rows, std::vector<int32_t>& changed, int kf, int idx) {
  if (kf < 0 || kf >= (int)rows.size() || idx < 0 || idx >= (int)rows[kf].size()) return 1;
  rows[kf][idx] = -1; changed.push_back(kf);
  return 0;
}

void drop(std::vector<int32_t>& a, std::vector<int32_t>& b, int at) { a.erase(a.begin() + at); b.erase(b.begin() + at); }

bool stereo(const Map& M, int kf, int idx) {
  const std::vector<float>& u = M.kf_uvr[kf];
  return 3 * (size_t)idx + 2 < u.size() && u[3 * (size_t)idx + 2] >= 0.f;
}

// false: nothing was refreshed
bool update_normal_and_depth(Map& M, int s, const std::vector<float>& level_scale) {
  const std::vector<int32_t>& kfs = M.pt_obs_kf[s]; const std::vector<int32_t>& ids = M.pt_obs_idx[s];
  const int ref = M.has_refs ? M.pt_ref[s] : -1;
  if (ref < 0 || !M.kf_feat[ref]) return false;
  for (size_t j = 0; j < kfs.size(); j++) if (!M.kf_feat[kfs[j]]) return false;
  const int at = find(kfs, ref);
  const int idx = at >= 0 ? ids[at] : 0;                               // observations[pRefKF] inserts 0 for a keyframe that is no observer
  if (idx >= (int)M.kf_octave[ref].size()) return false;
  const int level = M.kf_octave[ref][idx];
  if (level < 0 || level >= (int)level_scale.size()) return false;
  const float px = M.pt_pos[3 * (size_t)s], py = M.pt_pos[3 * (size_t)s + 1], pz = M.pt_pos[3 * (size_t)s + 2];
  float nx = 0.f, ny = 0.f, nz = 0.f;
  for (size_t j = 0; j < kfs.size(); j++) {
    const float* ow = &M.kf_ow[3 * (size_t)kfs[j]];
    const float dx = px - ow[0], dy = py - ow[1], dz = pz - ow[2];
    const float inv = (float)(1.0 / norm3(dx, dy, dz));
    nx = nx + dx * inv; ny = ny + dy * inv; nz = nz + dz * inv;
  }
  const float invn = (float)(1.0 / (double)kfs.size());
  M.pt_nrm[3 * (size_t)s] = nx * invn; M.pt_nrm[3 * (size_t)s + 1] = ny * invn; M.pt_nrm[3 * (size_t)s + 2] = nz * invn;
  const float* owr = &M.kf_ow[3 * (size_t)ref];
  const float dist = (float)norm3(px - owr[0], py - owr[1], pz - owr[2]);
  M.pt_maxd[s] = dist * level_scale[level];
  M.pt_mind[s] = M.pt_maxd[s] / level_scale[level_scale.size() - 1];
  return true;
}

void unique(std::vector<int32_t>& v) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }

}  // namespace

void centre(const float* T, float* ow) {
  for (int i = 0; i < 3; i++) {
    double s = (double)T[i] * (double)T[3];
    s += (double)T[4 + i] * (double)T[7];
    s += (double)T[8 + i] * (double)T[11];
    ow[i] = -(float)s;
  }
}

void apply(Map& M, const Window& W, const Result& R, Out& O) {
  O = Out();
  const size_t np = W.point_slot.size(), nl = W.line_slot.size();
  O.pt_flags.assign(np, 0);
  // ---- vToErase: the mono edges' observations, then the stereo edges' (:1282-1310), erased in that order (:1336-1345)
  for (size_t q = 0; q < np; q++) {
    const int s = W.point_slot[q];
    std::vector<int32_t>& kfs = M.pt_obs_kf[s]; std::vector<int32_t>& ids = M.pt_obs_idx[s];
    std::vector<int32_t> order;
    for (int pass = 0; pass < 2; pass++)
      for (int e = W.pt_obs_start[q]; e < W.pt_obs_start[q + 1]; e++) {
        if (!R.pt_obs_outlier[e]) continue;
        const int kf = W.cam_slot[W.pt_obs_cam[e]], at = find(kfs, kf);
        if (at >= 0 && stereo(M, kf, ids[at]) == (pass == 1)) order.push_back(kf);
      }
    int skipped = 0;
    for (size_t k = 0; k < order.size() && M.pt_state[s] != 2; k++) {
      const int kf = order[k], at = find(kfs, kf), idx = ids[at];
      skipped += erase_match(M.kf_points, O.changed_kf_rows, kf, idx);                 // KeyFrame::EraseMapPointMatch(pMP)
      M.pt_nobs[s] -= stereo(M, kf, idx) ? 2 : 1;                                       // MapPoint::EraseObservation
      drop(kfs, ids, at);
      O.changed_pt_rows.push_back(s); O.n_pt_obs_erased++;
      if (M.has_refs && M.pt_ref[s] == kf && !kfs.empty()) M.pt_ref[s] = kfs[0];
      if (M.pt_nobs[s] <= 2) {                                                          // SetBadFlag
        M.pt_state[s] = 2;
        for (size_t j = 0; j < kfs.size(); j++) skipped += erase_match(M.kf_points, O.changed_kf_rows, kfs[j], ids[j]);
        kfs.clear(); ids.clear();
        if (M.has_refs) M.pt_ref[s] = -1;
        O.n_points_bad++; O.pt_flags[q] |= WENT_BAD;
      }
    }
    if (skipped) { O.pt_flags[q] |= INDEX_SKIPPED; O.n_index_skipped += skipped; }
  }
  for (size_t l = 0; l < nl; l++) {
    if (R.line_removed[l]) continue;
    const int s = W.line_slot[l];
    std::vector<int32_t>& kfs = M.ln_obs_kf[s]; std::vector<int32_t>& ids = M.ln_obs_idx[s];
    for (int e = W.ln_obs_start[l]; e < W.ln_obs_start[l + 1] && !M.ln_bad[s]; e++) {
      if (!R.ln_edge_outlier[2 * (size_t)e] && !R.ln_edge_outlier[2 * (size_t)e + 1]) continue;
      const int kf = W.cam_slot[W.ln_obs_cam[e]], at = find(kfs, kf);
      if (at < 0) continue;
      const int idx = ids[at];
      O.n_index_skipped += erase_match(M.kf_lines, O.changed_kf_rows, kf, idx);
      const std::vector<float>& right = M.kf_kl_right[kf];
      bool partner = false;
      if (4 * (size_t)idx + 3 < right.size()) partner = !(right[4 * idx] == -1.f && right[4 * idx + 1] == -1.f && right[4 * idx + 2] == -1.f && right[4 * idx + 3] == -1.f);
      M.ln_nobs[s] -= partner ? 2 : 1;
      drop(kfs, ids, at);
      O.changed_ln_rows.push_back(s); O.n_ln_obs_erased++;
      if (M.ln_nobs[s] <= 4) { M.ln_bad[s] = 1; kfs.clear(); ids.clear(); O.n_lines_bad++; }      // SetBadFlag clears first: no observer's entry is found
    }
  }
  // ---- SetPose (:1364-1370)
  O.ow.assign(3 * (size_t)W.n_local, 0.f);
  for (int c = 0; c < W.n_local; c++) {
    const int s = W.cam_slot[c];
    std::copy(R.tcw.begin() + 16 * (size_t)c, R.tcw.begin() + 16 * (size_t)c + 16, M.kf_tcw.begin() + 16 * (size_t)s);
    centre(&M.kf_tcw[16 * (size_t)s], &M.kf_ow[3 * (size_t)s]);
    std::copy(M.kf_ow.begin() + 3 * (size_t)s, M.kf_ow.begin() + 3 * (size_t)s + 3, O.ow.begin() + 3 * (size_t)c);
  }
  // ---- SetWorldPos, UpdateNormalAndDepth (:1373-1379)
  for (size_t q = 0; q < np; q++) {
    const int s = W.point_slot[q];
    for (int k = 0; k < 3; k++) M.pt_pos[3 * (size_t)s + k] = (float)R.pt_xyz[3 * q + k];
    if (M.pt_state[s] == 2 || M.pt_obs_kf[s].empty()) continue;
    O.pt_flags[q] |= update_normal_and_depth(M, s, R.level_scale) ? REFRESHED : NO_REFERENCE;
  }
  // ---- SetMinimalPos (:1382-1386)
  for (size_t l = 0; l < nl; l++) {
    if (R.line_removed[l]) continue;
    const int s = W.line_slot[l];
    for (int k = 0; k < 3; k++) { M.ln_x0[3 * (size_t)s + k] = R.line_x0[3 * l + k]; M.ln_dir[3 * (size_t)s + k] = R.line_dir[3 * l + k]; }
  }
  unique(O.changed_kf_rows); unique(O.changed_pt_rows); unique(O.changed_ln_rows);
}

}  // namespace map_ba_apply_host
