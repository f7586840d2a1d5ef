// lld_frame_track_state.h — the device-resident tracking state of one lld_frame (what the reference keeps IN the Frame between the calls of
// the Tracking thread) as the translation units that run stages on it see it: lld_frame_track.hip (TrackWithMotionModel, TrackReferenceKeyFrame,
// TrackLocalMap, set_state, download) and lld_frame_reloc.hip (Relocalization), the device functions their kernels share, and the host half of a
// stage that both use: begin / submit and the region structs of the arrays both upload.  Nothing here is exported.
#ifndef LLD_FRAME_TRACK_STATE_H
#define LLD_FRAME_TRACK_STATE_H

#include "lld_common.h"
#include "lld_device_math.h"
#include "lld_track_internal.h"
#include "lld_upload_block.h"

namespace lld_track {

constexpr int kRecInts = 16;
struct RecHeader { double pose_qt[7]; double chi2; int32_t i[kRecInts]; };
// i[]: 0 n_inliers, 1 lm_iterations, 2 lm_trials, 3 n_edges, 4 n_search_first, 5 n_search, 6 used_wide, 7 n_points, 8 n_points_map,
//      9 n_lines_matched, 10 n_lines, 11 n_discarded, 12 n_point_edges, 13 n_in_view
enum { RI_INL = 0, RI_ITS, RI_TRIALS, RI_EDGES, RI_SEARCH1, RI_SEARCH, RI_WIDE, RI_POINTS, RI_POINTS_MAP, RI_LINES_MATCHED, RI_LINES, RI_DISCARDED, RI_POINT_EDGES, RI_IN_VIEW };

struct TrackDev {                 // device pointers of the frame's tracking state (all inside lld_frame_track_state::d_state)
  int nt, nl, nr, dim;
  uint8_t* kp_has; float* kp_world; int32_t* kp_id; uint8_t* kp_obs; uint8_t* kp_outlier;
  int32_t* discard; int32_t* n_discard;
  uint8_t* ln_has; double* ln_x0; double* ln_dir; int32_t* ln_id; uint8_t* ln_outlier;
  int32_t* tracked; int32_t* n_tracked; int tracked_cap;
  double* pose_qt; double* pose_out; lld_frame_view* view; LineTrackDevParams* line_params;
  // per-stage records
  RecHeader* rec_h[2]; int32_t* rec_kp_id[2]; uint8_t* rec_kp_out[2]; int32_t* rec_ln_id[2]; uint8_t* rec_ln_out[2];
};

// Both record headers to zero, one word per thread, when a frame enters stage 1.
__device__ inline void rec_headers_zero(const TrackDev& D, int i) {
  if (i < 2 * (int)(sizeof(RecHeader) / 4)) {
    int32_t* h = reinterpret_cast<int32_t*>(i < (int)(sizeof(RecHeader) / 4) ? D.rec_h[0] : D.rec_h[1]);
    h[i % (int)(sizeof(RecHeader) / 4)] = 0;
  }
}
// What PoseOptimization left in pose_out (PoseTrackDev::pose_out) as the head of a stage's record.
__device__ inline void rec_header_from_pose(RecHeader& H, const double* pose_out) {
  const int* pi = reinterpret_cast<const int*>(pose_out + 8);
  for (int c = 0; c < 7; c++) H.pose_qt[c] = pose_out[c];
  H.chi2 = pose_out[7];
  H.i[RI_INL] = pi[0]; H.i[RI_ITS] = pi[1]; H.i[RI_TRIALS] = pi[2]; H.i[RI_EDGES] = pi[3]; H.i[RI_POINT_EDGES] = pi[4];
}

struct ViewConsts { float fx, fy, cx, cy, bf, min_x, max_x, min_y, max_y, log_scale_factor; int n_levels; double b, thr_base, sx, sy; int monocular, use_grid; };

// Frame::UpdatePoseMatrices (src/Frame.cc:325-331) of a FLOAT mTcw, and Converter::toSE3Quat of it: mOw = -mRcw.t()*mtcw is one cv::gemm
// (double accumulation, one rounding).  The Frame keeps the FLOAT matrix only: the next PoseOptimization starts from
// Converter::toSE3Quat(pFrame->mTcw) (Optimizer.cc:823), i.e. from lld_se3_from_tcw_f32 of these floats.  No contraction: the same
// operations, one rounding each, as the host's conversions perform.
__device__ inline void view_from_matrix(const float* Rf, const float* tf, const ViewConsts& C, lld_frame_view* V, double* qt_of_float_matrix) {
#pragma clang fp contract(off)
  {
    lld::Mat3 Rd;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rd.m[i][j] = (double)Rf[3 * i + j];
    lld::Pose pf; pf.q = lld::quat_from_rotation(Rd); pf.t = lld::vec3((double)tf[0], (double)tf[1], (double)tf[2]);
    lld::pose_normalize(pf);
    lld::pose_store(pf, qt_of_float_matrix);
  }
  for (int i = 0; i < 9; i++) V->Rcw[i] = Rf[i];
  for (int i = 0; i < 3; i++) {
    V->tcw[i] = tf[i];
    const double acc = ((double)Rf[0 + i] * (double)tf[0] + (double)Rf[3 + i] * (double)tf[1]) + (double)Rf[6 + i] * (double)tf[2];
    V->Ow[i] = (float)(-acc);
  }
  V->fx = C.fx; V->fy = C.fy; V->cx = C.cx; V->cy = C.cy; V->bf = C.bf;
  V->min_x = C.min_x; V->max_x = C.max_x; V->min_y = C.min_y; V->max_y = C.max_y; V->log_scale_factor = C.log_scale_factor; V->n_levels = C.n_levels;
}

// AddLinesFrom's camera (src/Tracking.cc:920-923, :1136-1139): T_curr = mTcw.inv() widened to double.  The build takes the frame's own
// Rwc = Rcw^T and Ow for it (equal to OpenCV's float LU inverse up to float rounding: include/lld_amd.h); the right camera is GetTForRight.
// On the host for stage 1, where the view is the caller's (mVelocity * mLastFrame.mTcw is a float product).
__host__ __device__ inline void line_camera_from_view(const ViewConsts& C, const lld_frame_view& V, LineTrackDevParams* L) {
#pragma clang fp contract(off)
  for (int i = 0; i < 9; i++) L->K[i] = 0.0;
  L->K[0] = (double)C.fx; L->K[2] = (double)C.cx; L->K[4] = (double)C.fy; L->K[5] = (double)C.cy; L->K[8] = 1.0;
  for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) L->R[3 * r + c] = (double)V.Rcw[3 * c + r]; L->t[r] = (double)V.Ow[r]; }
  for (int r = 0; r < 3; r++) L->tr[r] = L->t[r] + L->R[3 * r] * C.b;
  L->thr_base = C.thr_base; L->sx = C.sx; L->sy = C.sy; L->monocular = C.monocular; L->use_grid = C.use_grid;
}

// Frame::SetPose + UpdatePoseMatrices (src/Frame.cc:318-331) from the optimised SE3Quat: Converter::toCvMat narrows to_homogeneous_matrix
// to float (src/Converter.cc:49-70), as lld_se3_to_tcw_f32 does on the host.  L (may be null): AddLinesFrom's camera.
__device__ inline void view_from_pose(const double* qt, const ViewConsts& C, lld_frame_view* V, LineTrackDevParams* L, double* qt_of_float_matrix) {
#pragma clang fp contract(off)
  const lld::Pose p = lld::pose_load(qt);
  const lld::Mat3 R = lld::quat_rotation(p.q);
  float Rf[9], tf[3];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Rf[3 * i + j] = (float)R.m[i][j];
  tf[0] = (float)p.t.x; tf[1] = (float)p.t.y; tf[2] = (float)p.t.z;
  view_from_matrix(Rf, tf, C, V, qt_of_float_matrix);
  if (L) line_camera_from_view(C, *V, L);
}

// Open-addressing sets of MapPoint / MapLine ids (>= 0; -1 = empty) in LDS, at most half full: "is this id among those the frame holds".
__device__ __forceinline__ unsigned seen_hash(int32_t id, unsigned mask) { return ((unsigned)id * 2654435761u >> 7) & mask; }
__device__ __forceinline__ void seen_insert(int32_t* tab, unsigned mask, int32_t id) {
  unsigned h = seen_hash(id, mask);
  for (;;) {
    const int32_t old = atomicCAS(&tab[h], -1, id);
    if (old == -1 || old == id) return;
    h = (h + 1) & mask;
  }
}
__device__ __forceinline__ bool seen_lookup(const int32_t* tab, unsigned mask, int32_t id) {
  unsigned h = seen_hash(id, mask);
  for (;;) {
    const int32_t v = tab[h];
    if (v == id) return true;
    if (v == -1) return false;
    h = (h + 1) & mask;
  }
}

}  // namespace lld_track

struct lld_frame_track_state {
  lld_track::TrackDev D{};
  char* d_state = nullptr;                 // per-frame state + records (sized at lld_frame_set_lines / first track call)
  size_t rec_off = 0, rec_bytes = 0;       // the two records, contiguous (one download)
  // frame lines
  int nl = 0, nr = 0, dim = 0; double sx = 0, sy = 0;
  const float* ln_left = nullptr; const int32_t* ln_loct = nullptr; const float* ln_right = nullptr; const int32_t* ln_roct = nullptr;
  const int32_t* ln_match = nullptr; const float* ln_desc = nullptr; int32_t* ln_cell = nullptr;
  // lld_frame_build_lines: the accepted stereo distances behind ln_match (null on a frame of lld_frame_set_lines); bytes of the span
  // ln_match [| ln_mdist] that lld_frame_lines_download fetches
  const double* ln_mdist = nullptr; size_t match_bytes = 0;
  // per-call work: uploaded inputs + search / line / pose scratch (grow-only), one pinned staging region per stage
  char* d_work = nullptr; size_t work_bytes = 0;
  char* h_stage[2] = {nullptr, nullptr}; size_t h_stage_bytes[2] = {0, 0};
  hipEvent_t uploaded[2] = {nullptr, nullptr}; bool upload_pending[2] = {false, false};
  char* h_rec = nullptr; size_t h_rec_bytes = 0;
  lld_track::ViewConsts consts{};
  bool stage1_queued = false;
  unsigned long long local_map_serial = 0;     // ... and that call's number on the map: another frame's update since replaces the lists
  const lld_map* local_map_of = nullptr;       // the map lld_frame_track_update_local_map ran on after the last stage 1 (every stage 1 clears it)
  bool stage2_queued = false;                  // lld_frame_track_local_map ran after the last stage 1: the stage-2 record is this frame's
  bool finish_ready = false;                   // the last chain call was lld_frame_track_local_map or lld_frame_track_set_state (lld_frame_track_finish)
  size_t in_view_off = 0; int n_in_view = 0;   // Frame::isInFrustum flags of stage 2's local MapPoints, inside d_work
  unsigned seen_psize = 0, seen_lsize = 0; size_t seen_lds = 0;   // track_mark_seen_kernel's tables (state_build)
};

namespace lld_track {
// host plumbing of a stage (lld_frame_track.hip)
int ensure_state(lld_frame* f);                                            // the state exists (a frame without lines unless lld_frame_set_lines ran)
int frame_max_lines(int nt);                                               // the most lines the chain tracks next to nt keypoints (lld_frame_set_lines' limit)
// (re)builds the state with the lines of lld_frame_build_lines (null or n_left = 0: without lines); queues the upload, the cells and the
// stereo match on the context's stream and does not wait.  The caller has validated `Bd` and waited if a state existed.
int frame_state_build_lines(lld_frame* f, const lld_frame_lines_build* Bd);
int ensure_stage(lld_frame_track_state* S, int s, size_t bytes);           // grow-only pinned staging of stage s, free of its previous upload
// begin: the grow-only d_work holds everything B declared (the stream is synchronised before it is reallocated), the pinned staging of stage s the uploaded prefix,
// and B is bound to the two; submit: the one copy of that prefix is queued
int stage_begin(lld_frame_track_state* S, lld_ctx* ctx, int s, UploadBlock& B);
int stage_submit(lld_frame_track_state* S, hipStream_t st, int s, const UploadBlock& B);
// what lld_frame_track_reference_keyframe refuses about a keyframe (LLD_ERR_INVALID); n_features: entries of its feature list
int ref_keyframe_check(const lld_ref_keyframe* kf, int* n_features);
void fill_consts(lld_frame_track_state* S, const lld_track_params* P, const lld_frame_view* view);

// ---- The groups of arrays a stage moves, each laid out (reserve), packed (stage) and bound to the kernels' structs (dev / out) in one place.
// pose | line camera | view: what a frame enters a stage-1 routine with
struct StageHeader {
  Span<double> pose; Span<LineTrackDevParams> lp; Span<lld_frame_view> view;
  void reserve(UploadBlock& B) { pose = B.take<double>(7); lp = B.take<LineTrackDevParams>(1); view = B.take<lld_frame_view>(1); }
  void stage(const UploadBlock& B, const ViewConsts& C, const lld_frame_view* v, const double* pose_qt) const {
    B.stage(pose, pose_qt); line_camera_from_view(C, *v, B.host(lp)); B.stage(view, v);
  }
};
// a new frame enters stage 1: no MapPoints, no flags, nothing discarded or tracked, both record headers zero, the uploaded header taken over
int track_reset_launch(hipStream_t st, lld_frame_track_state* S, const UploadBlock& B, const StageHeader& H);

// A reference keyframe: descriptors, angles, MapPoints, the FeatureVector as CSR; of a relocalisation candidate (x) also the MapPoints' distances and own descriptors.
struct RefKeyframeUp {
  Span<uint32_t> desc, pdesc; Span<float> ang, pos, maxd, mind; Span<int32_t> id, node, start, feat; Span<uint8_t> obs;
  struct Query { const float* pos; const int32_t* id; const uint8_t* obs; };                 // the q_* of an ApplyDev
  void reserve(UploadBlock& B, const lld_ref_keyframe& kf, int nv, const lld_reloc_candidate* x = nullptr) {
    const size_t n = kf.n, nn = kf.n_nodes;
    desc = B.take<uint32_t>(n, 8); ang = B.take<float>(n); id = B.take<int32_t>(n); pos = B.take<float>(n, 3); obs = B.take<uint8_t>(n);
    node = B.take<int32_t>(nn); start = B.take<int32_t>(nn + 1); feat = B.take<int32_t>(nv);
    maxd = B.take<float>(x ? n : 0); mind = B.take<float>(x ? n : 0); pdesc = (x && x->point_desc) ? B.take<uint32_t>(n, 8) : desc;   // no own descriptors: the keyframe's
  }
  void stage(const UploadBlock& B, const lld_ref_keyframe& kf, const lld_reloc_candidate* x = nullptr) const {
    B.stage(desc, kf.desc); B.stage(ang, kf.angle); B.stage(id, kf.point_id); B.stage(pos, kf.world_pos); B.stage(obs, kf.has_obs, 1);
    B.stage(node, kf.node); B.stage(start, kf.n_nodes ? kf.node_start : nullptr, 0); B.stage(feat, kf.feature);   // no nodes: node_start = {0}
    if (x) { B.stage(maxd, x->max_distance); B.stage(mind, x->min_distance); if (x->point_desc) B.stage(pdesc, x->point_desc); }
  }
  Query dev(const UploadBlock& B, BowSearchDev& S) const {
    S.kf_desc = B.dev(desc); S.kf_angle = B.dev(ang); S.kf_point_id = B.dev(id); S.kf_node = B.dev(node); S.kf_node_start = B.dev(start); S.kf_feature = B.dev(feat);
    return {B.dev(pos), B.dev(id), B.dev(obs)};
  }
};
// the searched side of a SearchByBoW: the resident frame's descriptors, angles and FeatureVector
inline void bow_frame_side(const lld_frame* f, BowSearchDev& S) {
  const KeypointsDev K = resident_keypoints(f, true);
  S.nt = K.nt; S.f_desc = K.desc; S.f_angle = K.angle;
  S.f_n_nodes = f->bow_n_nodes(); S.f_node = f->bow_node(); S.f_node_start = f->bow_node_start(); S.f_feature = f->bow_feature();
}

// Device-only scratch of one (nq, nt) guided search: SearchOut, query records, candidate cache (a retry of the same queries shares the last two).
// (ResultRegion of lld_orb_search.hip holds the same six arrays, but 64-byte aligned in the order its download fetches: it stays where it is.)
struct SearchScratch {
  Span<int32_t> match, bd, sd, owner, sum; Span<uint8_t> rem; Span<char> qrec, cache;
  void reserve(UploadBlock& B, int nq, int nt, const SearchScratch* query_of = nullptr) {
    match = B.take<int32_t>(nq); bd = B.take<int32_t>(nq); sd = B.take<int32_t>(nq); rem = B.take<uint8_t>(nq); owner = B.take<int32_t>(nt); sum = B.take<int32_t>(4);
    qrec = query_of ? query_of->qrec : B.take<char>(orbs_qrec_bytes(nq)); cache = query_of ? query_of->cache : B.take<char>(orbs_cache_bytes(nq));
  }
  SearchOut out(const UploadBlock& B) const { return {B.dev(match), B.dev(bd), B.dev(sd), B.dev(rem), B.dev(owner), B.dev(sum)}; }
};
}  // namespace lld_track

#endif
