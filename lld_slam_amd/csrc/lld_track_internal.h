// lld_track_internal.h — what the translation units of liblld_amd.so share for the device-resident Tracking-thread chain (lld_frame_track_*,
// lld_frame_track.hip): the resident frame, and launchers that run the searches, the line association and the pose optimisation of the
// single-call entry points on DEVICE arrays, on a stream, without touching the host.  Nothing here is exported (-fvisibility=hidden).
#ifndef LLD_TRACK_INTERNAL_H
#define LLD_TRACK_INTERNAL_H

#include "lld_common.h"

struct lld_frame_track_state;

// A frame whose keypoint side lives on the device for as long as the Tracking thread works on it (round 5, lld_frame_*): descriptors,
// undistorted positions, octaves, right coordinates and angles are uploaded ONCE; the per-frame routines that search this frame
// (lld_frame_search_last_frame: Tracking.cc:904, lld_frame_search_local_points: :1133) then move only their queries and the occupancy bytes.
// Round 6: `track` holds what the reference keeps IN the Frame between those calls (mvpMapPoints, mvbOutlier, mvpMapLines, mvbOutlierLines, mTcw)
// as device arrays, so that the whole sequence runs without a trip through the host (lld_frame_track.hip).
struct lld_frame {
  lld_ctx* ctx = nullptr;
  int nt = 0; bool has_uright = false, has_angle = false, has_inv_sigma2 = false;
  char* d = nullptr;                       // one device allocation: desc | xy | octave | uright | angle
  size_t o_td = 0, o_txy = 0, o_toct = 0, o_tur = 0, o_tang = 0;
  lld_orb_search consts;                   // grid constants, n_levels; the level tables are copied below
  float scale[LLD_ORB_MAX_LEVELS], sigma2[LLD_ORB_MAX_LEVELS], inv_sigma2[LLD_ORB_MAX_LEVELS];
  std::vector<int32_t> octave;             // host copy (validation of queries needs none of the rest)
  lld_frame_track_state* track = nullptr;  // owned by lld_frame_track.hip (lld_track::state_free)
  // A frame built by lld_frame_build_stereo* (lld_frame_build.hip): mvuRight / mvDepth were computed into `d` by kernels.  o_res is the start of
  // the contiguous block u_right | depth | best_r | sad | summary that lld_frame_stereo_download fetches in one copy (u_right at o_tur); h_stage is
  // the pinned staging of the build's one upload, owned by the frame because the build returns before that copy has run.
  bool stereo_built = false;
  size_t o_res = 0, o_depth = 0, o_bestr = 0, o_sad = 0, o_sum = 0, res_bytes = 0;
  void* h_stage = nullptr;
  // lld_frame_build_lines (lld_frame_lines.hip): the pinned staging of its one upload, grow-only and the frame's own for the same reason.
  void* h_lines = nullptr; size_t h_lines_bytes = 0;
  // A frame built by lld_frame_build_mono* (lld_frame_mono.hip): the kernel wrote mvKeysUn, mvuRight and mvDepth into `d`; o_res is the start of
  // the contiguous block u_right | depth | xy that lld_frame_keypoints_download fetches in one copy.  h_stage as above.
  bool mono_built = false;
  // Frame::ComputeBoW (lld_frame_compute_bow, lld_bow.hip): the frame's copy of the vocabulary's output block for its nt descriptors -
  // value[nt] f64 | int32 {n_words, n_nodes} | word[nt] | node[nt] | node_start[nt + 1] | feature[nt] | ... - so mFeatVec stays in HBM.
  char* d_bow = nullptr; bool has_bow = false;
  const int32_t* bow_ints() const { return reinterpret_cast<const int32_t*>(d_bow + (size_t)8 * nt); }
  const int32_t* bow_n_nodes() const { return bow_ints() + 1; }
  const int32_t* bow_node() const { return bow_ints() + 2 + nt; }
  const int32_t* bow_node_start() const { return bow_ints() + 2 + 2 * (size_t)nt; }
  const int32_t* bow_feature() const { return bow_ints() + 3 + 3 * (size_t)nt; }
};

namespace lld_track {

void state_free(lld_frame* f);             // lld_frame_destroy calls it before the keypoints go
// The keypoint side of a search or a pose problem as DEVICE pointers; of a resident frame (lld_orb_search.hip): uright / angle null when it has none.
struct KeypointsDev { int nt; const uint32_t* desc; const float* xy; const int32_t* octave; const float* uright; const float* angle; };
KeypointsDev resident_keypoints(const lld_frame* f, bool want_angle);

// ---------------------------------------------------------------- guided ORB search on device arrays (lld_orb_search.hip)
// One search = a projection kernel that writes the query records + orb_search_kernel on one workgroup, which also hands the frame what it
// matched (mvpMapPoints[bestIdx] = pMP as an epilogue).  Everything the kernels read or write is a device pointer; the problem is filled on the
// host into pinned memory the caller uploads before the launch.  run_if: when non-null the kernels return at once unless
// (*flag < below) == (want != 0) - the reference's "if(nmatches<20) search again with 2*th" (src/Tracking.cc:907-911) without a host decision.
// sizeof the search kernel's problem record.  It is also the stride of the arrays of problems the kernel indexes (orbs_launch_n), so it
// is not rounded up: a caller that places a lone problem in a work buffer aligns the offset like every other region of that buffer.
size_t orbs_problem_bytes();
size_t orbs_qrec_bytes(int nq);
size_t orbs_cache_bytes(int nq);
struct SearchOut { int32_t* match; int32_t* best_dist; int32_t* second_dist; uint8_t* removed; int32_t* owner; int32_t* summary; };
struct RunIf { const int32_t* flag = nullptr; int below = 0; int want = 1; };
// the frame's mvpMapPoints and where the queries' MapPoints are described; counts: [0] n of the first search, [1] n of the search taken, [2] retry used
struct ApplyDev { uint8_t* kp_has; float* kp_world; int32_t* kp_id; uint8_t* kp_obs; const float* q_pos; const int32_t* q_id; const uint8_t* q_obs;
                  int32_t* counts; int min_matches; int is_retry; };
struct LastFrameDev { int n; const float* pos; const uint8_t* valid; const int32_t* octave; const float* angle; const uint8_t* has_obs; };
struct MapPointsDev { int n; const float* pos; const float* normal; const float* maxd; const float* mind; const uint8_t* has_obs; const uint8_t* skip; };
// mode 0: SearchByProjection(Current, Last) rules (TH_HIGH, no ratio, rotation histogram optional); mode 1: SearchByProjection(F, MapPoints) rules
void orbs_fill_problem(const lld_frame* f, int mode, int nq, const uint8_t* d_occupied, const void* d_qrec, const uint32_t* d_qdesc, const SearchOut& out,
                       void* d_cache, float nnratio, int check_orientation, RunIf run_if, const ApplyDev& ap, void* problem_h);
// The projection loops, shared with the single-call entry points.  c: the searched frame's level_scale / n_levels; the view is read from
// view_d (device memory) when that is non-null, else passed by value from view_h.  d_uvr and every member of FrustumOut are optional
// device outputs: in_view[n] u8, uvr[n][3], level[n], view_cos[n]; *n_in_view += the number of points inside the frustum.
struct FrustumOut { uint8_t* in_view; float* uvr; int32_t* level; float* view_cos; int32_t* n_in_view; };
int orbs_project_last_frame(hipStream_t st, const lld_orb_search& c, const lld_frame_view* view_h, const lld_frame_view* view_d, const LastFrameDev& last, int direction, float th,
                            void* d_qrec, float* d_uvr, RunIf run_if);
int orbs_project_local_points(hipStream_t st, const lld_orb_search& c, const lld_frame_view* view_h, const lld_frame_view* view_d, const MapPointsDev& mp, float cos_limit, float th,
                              void* d_qrec, const FrustumOut& out);
// ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1472-1599, LLD_ORB_PROJ_RELOC) on n_slots copies
// of the frame's mvpMapPoints at once, each against its own keyframe: slot s projects its candidate's MapPoints through ITS view (device
// memory) and searches with ITS occupancy.  A slot runs iff *run != 0 (projection) / its Problem's run_if holds (search).
struct RelocProjSlot { int32_t n; int32_t pad; const float* pos; const float* maxd; const float* mind; const uint8_t* skip; const float* angle; void* qrec;
                       const lld_frame_view* view; const int32_t* run; };
int orbs_project_reloc_slots(hipStream_t st, const lld_frame* f, int n_slots, int n_max, const RelocProjSlot* slots_d, float th);
// orbs_fill_problem for that search: occupancy = any MapPoint on the keypoint (:1528), bestDist <= accept_max, the rotation histogram, no ratio test
void orbs_fill_problem_reloc(const lld_frame* f, int nq, const uint8_t* d_occupied, const void* d_qrec, const uint32_t* d_qdesc, const SearchOut& out, void* d_cache,
                             int accept_max, RunIf run_if, const ApplyDev& ap, void* problem_h);
int orbs_launch_n(lld_ctx* ctx, hipStream_t st, const lld_frame* f, const void* problems_d, int n);   // problems_d[n], one workgroup per problem

// ---------------------------------------------------------------- ORBmatcher::SearchByBoW(KeyFrame*, Frame&) on device arrays (lld_frame_track_bow.hip)
// The frame's FeatureVector is the one in lld_frame::d_bow (its node count is read on the device), the keyframe's an uploaded CSR.  One
// wavefront per keyframe node; `taken` [nt] is scratch (the keyframe feature that took frame feature k, or -1).  The accepted matches that
// survive the rotation histogram go into the frame's tables through `ap` (q_* index keyframe features); ap.counts[0..2] = n, n, 0.
struct BowSearchDev {
  int nt, n_kf_nodes;
  const uint32_t* f_desc; const float* f_angle;
  const int32_t* f_n_nodes; const int32_t* f_node; const int32_t* f_node_start; const int32_t* f_feature;
  const uint32_t* kf_desc; const float* kf_angle; const int32_t* kf_point_id;
  const int32_t* kf_node; const int32_t* kf_node_start; const int32_t* kf_feature;
  float nnratio; int check_orientation;
  int32_t* taken;
};
int bow_search_launch(hipStream_t st, const BowSearchDev& in, const ApplyDev& ap);

// ---------------------------------------------------------------- the line matchers on device arrays (lld_line_match.hip)
// The limits every line matcher with a resolve shares (include/lld_amd.h, lld_line_match_greedy): LLD_ERR_UNSUPPORTED for dim > LLD_LINE_DIM_MAX,
// for a row of `cols` distances + the descriptor or the resolve's rows + cols words above LLD_LINE_LDS_CEILING; LLD_OK when either side is empty.
// Decided from the counts alone, so every route asks before it allocates or queues anything.
int line_limits_check(int rows, int cols, int dim);
size_t line_work_bytes(int rows, int cols);          // the d_work of the launchers below: gate [rows][cols] | distances [rows][cols] | candidate lists [rows]

// Tracking::AddLinesFrom.  The camera the gate kernel takes (by value, or from device memory where a pose kernel wrote it):
struct LineTrackDevParams { double K[9]; double R[9]; double t[3]; double tr[3]; double thr_base, sx, sy; int monocular, use_grid; };
struct LineMapDev { int n; const double* x0; const double* dir; const double* x1; const double* x2; const uint8_t* skip; const float* desc; };
struct LineFrameDev { int n_cur; const float* left; const int32_t* loct; const float* right; const int32_t* lmatch; const uint8_t* occupied; const int32_t* cell;
                      const float* desc; int dim; };
// mCurrentFrame.mvpMapLines[mi] = pML; pML->tracked_last_id = mnId (src/Tracking.cc:1116-1117), done by the assignment kernel itself
struct LineApplyDev { uint8_t* ln_has; double* ln_x0; double* ln_dir; int32_t* ln_id; int32_t* tracked; int32_t* n_tracked; int tracked_cap; const int32_t* map_id; };
int line_cells_dev(hipStream_t st, const float* d_left, int n, double sx, double sy, int32_t* d_cell);
// params_d: LineTrackDevParams in device memory (written by the tracker's pose kernel); matches_d [n_map]
int line_track_launch_dev(hipStream_t st, const LineTrackDevParams* params_d, const LineMapDev& map, const LineFrameDev& cur, double md_thr,
                          void* d_work, int32_t* matches_d, const LineApplyDev& apply);

// TwoFrameLineMatcher::MatchLines of the frame's stereo pair (the kernels of lld_line_match_stereo) on device arrays: matches_d [nl] is the
// frame's line_matches, match_dist_d [nl] the accepted distances (DBL_MAX where none).  Nothing is launched when either side is empty.
struct LineStereoDev { int nl, nr, dim; const float* left; const int32_t* loct; const float* right; const int32_t* roct; const float* dl; const float* dr; };
int line_stereo_launch_dev(hipStream_t st, const lld_line_stereo_params& prm, const LineStereoDev& in, void* d_work, int32_t* matches_d, double* match_dist_d);
// Tracking::MatchLinesLastKF (the kernel of lld_line_match_last_frame) between two resident frames: `last` is a LineFrameDev whose n_cur counts
// the last frame's lines; the cameras are the frames' own LineTrackDevParams in device memory (K, sx, sy from cur_cam).
struct LastKfDev { LineFrameDev cur, last; const uint8_t* last_skip; const LineTrackDevParams* cur_cam; const LineTrackDevParams* last_cam; };
int line_lastkf_launch_dev(hipStream_t st, const LastKfDev& in, double thr_base, double md_thr, int use_grid, int32_t* match_last, uint8_t* created, double* x0, double* dir);

// ---------------------------------------------------------------- Optimizer::PoseOptimization on the frame's device state (lld_pose.hip)
struct PoseTrackDev {
  int nt, nl;                                          // keypoints / left lines of the frame (upper bounds of the edge counts)
  const float* t_xy; const float* t_uright; const int32_t* t_octave;
  const uint8_t* kp_has; const float* kp_world;
  const float* ln_left; const int32_t* ln_loct; const float* ln_right; const int32_t* ln_roct; const int32_t* ln_match;
  const uint8_t* ln_has; const double* ln_x0; const double* ln_dir;
  const double* pose_qt;                               // [7] device: the estimate the optimisation starts from (Converter::toSE3Quat(pFrame->mTcw))
  lld_camera cam; double gamma; float inv_sigma2[LLD_ORB_MAX_LEVELS];
  // outputs (device): per keypoint / per line outlier flags as PoseOptimization leaves mvbOutlier / mvbOutlierLines for the entries it touched
  uint8_t* kp_outlier; uint8_t* ln_outlier;
  double* pose_out;                                    // [7] + chi2 + (n_inliers, lm_iterations, lm_trials, n_edges, n_points, n_line_edges) as int32: 11 doubles
};
size_t pose_track_work_bytes(int nt, int nl);
int pose_track_launch(lld_ctx* ctx, hipStream_t st, const PoseTrackDev& in, const lld_pose_params& prm, void* d_work);
// The same PoseOptimization on n_slots COPIES of one frame's mvpMapPoints / mvbOutlier / mTcw at once (Tracking::Relocalization evaluates its
// candidates side by side, lld_frame_reloc.hip): points only, one workgroup of pose_opt_kernel per slot.  Slot s runs iff run[s] != 0 - a
// slot that does not run keeps its flags and its pose_out.
struct PoseSlotsDev {
  int n_slots, nt;
  const float* t_xy; const float* t_uright; const int32_t* t_octave;       // the frame's keypoints (shared by the slots)
  const uint8_t* kp_has; const float* kp_world;                            // [n_slots][nt], [n_slots][nt][3]
  const double* pose_qt;                                                   // [n_slots][7]
  const int32_t* run;                                                      // [n_slots]
  lld_camera cam; float inv_sigma2[LLD_ORB_MAX_LEVELS];
  uint8_t* kp_outlier;                                                     // [n_slots][nt]
  double* pose_out;                                                        // [n_slots][12], each as PoseTrackDev::pose_out
};
size_t pose_slots_work_bytes(int n_slots, int nt);
int pose_slots_launch(lld_ctx* ctx, hipStream_t st, const PoseSlotsDev& in, const lld_pose_params& prm, void* d_work);

}  // namespace lld_track

#endif
