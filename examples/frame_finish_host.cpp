// frame_finish_host.cpp — the tail of Tracking::Track (src/Tracking.cc:446-476, :1223-1310, :1386-1430) as the HOST loops a caller runs when the
// frame's state has been downloaded: the route the library offered before lld_frame_track_finish.  Plain C++ on flat arrays, no library call:
// examples/frame_finish_harness.cpp compares it with the device call, tools/time_frame_finish.py times it (built as a shared object).
#include "frame_finish_host.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace {

// Tracking::NeedNewKeyFrame after its counting loop (:1227-1309)
bool need_new_keyframe(const lld_frame_finish_params& p, int nTrackedClose, int nNonTrackedClose, int mnMatchesInliers, int* interrupt) {
  *interrupt = 0;
  if (p.only_tracking) return false;
  if (p.mapper_stopped) return false;
  const int nKFs = p.n_keyframes;
  if (p.frame_id < p.last_reloc_frame_id + p.max_frames && nKFs > p.max_frames) return false;
  const int nRefMatches = p.n_ref_matches;
  const bool bLocalMappingIdle = p.mapper_idle != 0;
  const bool bNeedToInsertClose = (nTrackedClose < 100) && (nNonTrackedClose > 70);
  float thRefRatio = 0.75f;
  if (nKFs < 2) thRefRatio = 0.4f;
  if (p.monocular) thRefRatio = 0.9f;
  const bool c1a = p.frame_id >= p.last_keyframe_id + p.max_frames;
  const bool c1b = (p.frame_id >= p.last_keyframe_id + p.min_frames && bLocalMappingIdle);
  const bool c1c = !p.monocular && (mnMatchesInliers < nRefMatches * 0.25 || bNeedToInsertClose);
  const bool c2 = ((mnMatchesInliers < nRefMatches * thRefRatio || bNeedToInsertClose) && mnMatchesInliers > 15);
  if ((c1a || c1b || c1c) && c2) {
    if (bLocalMappingIdle) return true;
    *interrupt = 1;
    if (!p.monocular) return p.keyframes_in_queue < 3;
    return false;
  }
  return false;
}

}  // namespace

// mCurrentFrame.mvpMapPoints / mvbOutlier as TrackLocalMap leaves them for a STEREO system (src/Tracking.cc:1155-1175), from the stage-2 record of
// lld_frame_track_download and the host's own MapPoints (world_of / obs_of: GetWorldPos() and Observations() > 0 by id): the flagged points leave, the flags stay.
extern "C" void frame_finish_host_state(int nt, const int32_t* rec_kp_point_id, const uint8_t* rec_kp_outlier, const float* world_of, const uint8_t* obs_of,
                                        int32_t* kp_id, uint8_t* kp_obs, uint8_t* kp_outlier, float* kp_world) {
  for (int i = 0; i < nt; i++) {
    const int32_t id = (rec_kp_point_id[i] >= 0 && !rec_kp_outlier[i]) ? rec_kp_point_id[i] : -1;
    kp_id[i] = id; kp_outlier[i] = rec_kp_outlier[i]; kp_obs[i] = id >= 0 ? obs_of[id] : 0;
    for (int c = 0; c < 3; c++) kp_world[3 * i + c] = id >= 0 ? world_of[3 * (size_t)id + c] : 0.f;
  }
}

extern "C" void frame_finish_host_tail(int nt, const float* mvDepth, const float* mvKeysUn_xy, const lld_frame_view* view, const lld_frame_finish_params* p,
                                       int32_t* kp_id, uint8_t* kp_obs, uint8_t* kp_outlier, float* kp_world, lld_frame_finish_result* out) {
  for (int i = 0; i < nt; i++) {                                              // Clean VO matches (:446-453)
    if (kp_id[i] >= 0 && !kp_obs[i]) { kp_outlier[i] = 0; kp_id[i] = -1; }
    out->created[i] = 0; out->new_id[i] = -1; out->order[i] = -1; out->x3d[3 * i] = out->x3d[3 * i + 1] = out->x3d[3 * i + 2] = 0.f;
  }
  int nNonTrackedClose = 0, nTrackedClose = 0;                                // :1250-1264
  if (!p->monocular) {
    for (int i = 0; i < nt; i++) {
      if (mvDepth[i] > 0 && mvDepth[i] < p->th_depth) {
        if (kp_id[i] >= 0 && !kp_outlier[i]) nTrackedClose++; else nNonTrackedClose++;
      }
    }
  }
  int interrupt = 0;
  const bool need = need_new_keyframe(*p, nTrackedClose, nNonTrackedClose, p->n_matches_inliers, &interrupt);
  const bool made = p->force >= 0 ? p->force != 0 : (need && p->set_not_stop_ok);
  int n_visited = 0, n_created = 0;
  if (made) {                                                                 // CreateNewKeyFrame (:1386-1430)
    std::vector<std::pair<float, int> > vDepthIdx;
    vDepthIdx.reserve(nt);
    for (int i = 0; i < nt; i++) {
      const float z = mvDepth[i];
      if (z > 0) vDepthIdx.push_back(std::make_pair(z, i));
    }
    if (!vDepthIdx.empty()) {
      std::sort(vDepthIdx.begin(), vDepthIdx.end());
      const float invfx = 1.0f / view->fx, invfy = 1.0f / view->fy;
      int nPoints = 0;
      for (size_t j = 0; j < vDepthIdx.size(); j++) {
        const int i = vDepthIdx[j].second;
        out->order[i] = (int32_t)j; n_visited++;
        bool bCreateNew = false;
        if (kp_id[i] < 0) bCreateNew = true;
        else if (!kp_obs[i]) { bCreateNew = true; kp_id[i] = -1; }
        if (bCreateNew) {
          const float z = mvDepth[i], u = mvKeysUn_xy[2 * i], v = mvKeysUn_xy[2 * i + 1];   // Frame::UnprojectStereo (Frame.cc:730-744)
          const float x = (u - view->cx) * z * invfx, y = (v - view->cy) * z * invfy;
          const float c[3] = {x, y, z};
          for (int r = 0; r < 3; r++) {                                       // mRwc*x3Dc+mOw: double accumulation, one rounding, then the float sum
            double acc = (double)view->Rcw[r] * (double)c[0];
            acc += (double)view->Rcw[3 + r] * (double)c[1];
            acc += (double)view->Rcw[6 + r] * (double)c[2];
            const float w = (float)acc + view->Ow[r];
            out->x3d[3 * i + r] = w; kp_world[3 * i + r] = w;
          }
          const int32_t id = p->first_new_id + n_created;
          kp_id[i] = id; kp_obs[i] = 1;
          out->created[i] = 1; out->new_id[i] = id;
          n_created++; nPoints++;
        } else {
          nPoints++;
        }
        if (vDepthIdx[j].first > p->th_depth && nPoints > 100) break;
      }
    }
  }
  for (int i = 0; i < nt; i++) {                                              // :472-476
    if (kp_id[i] >= 0 && kp_outlier[i]) kp_id[i] = -1;
    out->kp_point_id[i] = kp_id[i];
  }
  out->n_tracked_close = nTrackedClose; out->n_non_tracked_close = nNonTrackedClose; out->need = need; out->interrupt_ba = interrupt; out->made = made;
  out->n_visited = n_visited; out->n_created = n_created; out->reserved = 0;
}
