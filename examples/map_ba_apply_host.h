// map_ba_apply_host.h — the tail of Optimizer::LocalBundleAdjustment under mMutexMapUpdate (src/Optimizer.cc:1334-1386 of the reference) as a
// host runs it today, in compiled C++ on flat tables: erase the outlier observations, SetPose, SetWorldPos + UpdateNormalAndDepth,
// SetMinimalPos.  It is the route a caller of lld_map_local_ba has without lld_map_ba_apply (the changed rows then go back through the
// lld_map_set_* calls: `changed_*` lists them), the other side of tools' timing, and a second restatement next to
// tests/map_ba_apply_ref.py.  Restated from the reference, not copied: objects are slots, members are arrays.  No liblld_amd.so.
#ifndef LLD_MAP_BA_APPLY_HOST_H
#define LLD_MAP_BA_APPLY_HOST_H

#include <cstdint>
#include <vector>

namespace map_ba_apply_host {

typedef std::vector<std::vector<int32_t> > Rows;

struct Map {
  int n_kf = 0, n_pt = 0, n_ln = 0;
  // keyframe slot s: has a pose and features; Tcw [16]; Ow [3] (SetPose keeps it); mvpMapPoints / mvpMapLines as slots or -1; per keypoint
  // the octave and (u, v, uR); per keyline the right end points (four times -1.0f: no partner)
  std::vector<uint8_t> kf_feat; std::vector<float> kf_tcw, kf_ow;
  Rows kf_points, kf_lines, kf_octave; std::vector<std::vector<float> > kf_uvr, kf_kl_right;
  // point slot s: 0 never set, 1 live, 2 isBad; mWorldPos, mNormalVector, min / max distance, nObs, mpRefKF (-1 unknown), mObservations
  std::vector<uint8_t> pt_state; std::vector<float> pt_pos, pt_nrm, pt_mind, pt_maxd; std::vector<int32_t> pt_nobs, pt_ref; bool has_refs = false;
  Rows pt_obs_kf, pt_obs_idx;
  std::vector<uint8_t> ln_bad; std::vector<double> ln_x0, ln_dir; std::vector<int32_t> ln_nobs; Rows ln_obs_kf, ln_obs_idx;
};

struct Window {                                // the index arrays of lld_map_ba_window / lld_map_ba_ids
  int n_local = 0;
  std::vector<int32_t> cam_slot, point_slot, pt_obs_start, pt_obs_cam, line_slot, ln_obs_start, ln_obs_cam;
};

struct Result {                                // lld_ba_result, with the local cameras' poses already as float matrices (lld_se3_to_tcw_f32)
  std::vector<float> tcw;                      // [n_local][16]
  std::vector<double> pt_xyz, line_x0, line_dir;
  std::vector<uint8_t> pt_obs_outlier, ln_edge_outlier, line_removed;
  std::vector<float> level_scale;
};

enum { WENT_BAD = 1, REFRESHED = 2, NO_REFERENCE = 4, INDEX_SKIPPED = 8 };

struct Out {                                   // lld_map_ba_apply_out, and the rows a caller has to send back through the setters
  int n_pt_obs_erased = 0, n_ln_obs_erased = 0, n_points_bad = 0, n_lines_bad = 0, n_index_skipped = 0;
  std::vector<float> ow;
  std::vector<uint8_t> pt_flags;
  std::vector<int32_t> changed_kf_rows, changed_pt_rows, changed_ln_rows;      // slots whose point / line rows, observation rows changed (each once, ascending)
};

// KeyFrame::SetPose's centre of a float pose: -Rcw^T tcw, each entry one three-term double sum rounded once
void centre(const float* T, float* ow);
void apply(Map& M, const Window& W, const Result& R, Out& O);

}  // namespace map_ba_apply_host

#endif
