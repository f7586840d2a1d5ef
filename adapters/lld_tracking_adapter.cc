// lld_tracking_adapter.cc — see lld_tracking_adapter.h
#include "lld_tracking_adapter.h"

#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>

namespace lld_adapter {

namespace {

void check(int status, const char* what) {
  if (status != LLD_OK) throw std::runtime_error(std::string(what) + ": " + lld_status_string(status));
}

void key_lines(const std::vector<lld_slam::KeyLine>& kl, std::vector<float>& seg, std::vector<int32_t>& octave) {
  seg.resize(4 * kl.size()); octave.resize(kl.size());
  for (size_t i = 0; i < kl.size(); i++) {
    seg[4 * i] = kl[i].startPointX; seg[4 * i + 1] = kl[i].startPointY; seg[4 * i + 2] = kl[i].endPointX; seg[4 * i + 3] = kl[i].endPointY;
    octave[i] = kl[i].octave;
  }
}

// Frame::UpdatePoseMatrices as the frame holds it
lld_frame_view view_of(const Frame& F) {
  lld_frame_view v; std::memset(&v, 0, sizeof v);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) v.Rcw[3 * r + c] = F.mRcw.at<float>(r, c);
    v.tcw[r] = F.mtcw.at<float>(r); v.Ow[r] = F.mOw.at<float>(r);
  }
  v.fx = F.fx; v.fy = F.fy; v.cx = F.cx; v.cy = F.cy; v.bf = F.mbf;
  v.min_x = F.mnMinX; v.max_x = F.mnMaxX; v.min_y = F.mnMinY; v.max_y = F.mnMaxY;
  v.log_scale_factor = F.mfLogScaleFactor; v.n_levels = F.mnScaleLevels;
  return v;
}

// MapLine list -> lld_map_lines (GetMinimalPos, GetMainPoints3D, descriptor row, skip = NULL || tracked_last_id == mnId || isBad:
// src/Tracking.cc:1013-1025; the device applies the "already tracked" rule by id as well)
struct LineSide {
  std::vector<double> x0, dir, x1, x2; std::vector<uint8_t> skip; std::vector<float> desc; std::vector<int32_t> id;
  lld_map_lines m;
  LineSide(const std::vector<MapLine*>& lines, const std::vector<lld_slam::Mat>* descs, const lld_slam::Mat* rows, int dim, unsigned long frame_id) {
    const int n = (int)lines.size();
    x0.assign(3 * (size_t)n + 3, 0.0); dir = x0; x1 = x0; x2 = x0; skip.assign(n + 1, 1); desc.assign((size_t)n * dim + 1, 0.f); id.assign(n + 1, 0);
    for (int i = 0; i < n; i++) {
      MapLine* pML = lines[i];
      if (!pML) continue;
      id[i] = (int32_t)pML->mnId;
      if ((unsigned int)pML->tracked_last_id == frame_id || pML->isBad()) continue;                       // :1018-1025
      skip[i] = 0;
      lld_slam::Vector3d a, d, p1, p2;
      pML->GetMinimalPos(&a, &d); pML->GetMainPoints3D(&p1, &p2);
      for (int k = 0; k < 3; k++) { x0[3 * i + k] = a(k); dir[3 * i + k] = d(k); x1[3 * i + k] = p1(k); x2[3 * i + k] = p2(k); }
      const float* row = (descs && !descs->empty()) ? (*descs)[i].ptr<float>() : rows->ptr<float>(i);       // :1043-1048
      for (int k = 0; k < dim; k++) desc[(size_t)i * dim + k] = row[k];
    }
    m.n = n; m.x0 = x0.data(); m.dir = dir.data(); m.x1 = x1.data(); m.x2 = x2.data(); m.skip = skip.data(); m.desc = desc.data(); m.id = id.data();
  }
};

struct Outputs {
  std::vector<int32_t> kp_id, ln_id; std::vector<uint8_t> kp_out, ln_out, in_view;
  lld_track_result r;
  Outputs(int nt, int nl, int n_mp) : kp_id(nt + 1, -1), ln_id(nl + 1, -1), kp_out(nt + 1, 0), ln_out(nl + 1, 0), in_view(n_mp + 1, 0) {
    std::memset(&r, 0, sizeof r);
    r.kp_point_id = kp_id.data(); r.kp_outlier = kp_out.data(); r.ln_line_id = ln_id.data(); r.ln_outlier = ln_out.data(); r.mp_in_view = n_mp > 0 ? in_view.data() : nullptr;
  }
  void to(TrackTrace* t, int nt, int nl, int n_mp) const {
    if (!t) return;
    t->r = r; t->r.kp_point_id = nullptr; t->r.kp_outlier = nullptr; t->r.ln_line_id = nullptr; t->r.ln_outlier = nullptr; t->r.mp_in_view = nullptr;
    t->kp_point_id.assign(kp_id.begin(), kp_id.begin() + nt); t->kp_outlier.assign(kp_out.begin(), kp_out.begin() + nt);
    t->ln_line_id.assign(ln_id.begin(), ln_id.begin() + nl); t->ln_outlier.assign(ln_out.begin(), ln_out.begin() + nl);
    t->mp_in_view.assign(in_view.begin(), in_view.begin() + n_mp);
  }
};

// pFrame->SetPose(Converter::toCvMat(SE3quat_recov)) (src/Optimizer.cc:915-918) - when PoseOptimization got past its early return
void set_pose(Frame& F, const lld_track_result& r) {
  if (r.n_point_edges < 3) return;
  float T[16];
  lld_se3_to_tcw_f32(r.pose_qt, T);
  F.SetPose(lld_slam::Mat(4, 4, T));
}

// KeyFrame -> lld_ref_keyframe (src/ORBmatcher.cc:161-199, :234): mDescriptors, mvKeysUn[k].angle, GetMapPointMatches() with NULL / isBad as -1, mFeatVec
struct KeyFrameSide {
  std::vector<float> angle, pos, maxd, mind; std::vector<int32_t> ids, knode, kstart, kfeat; std::vector<uint8_t> has_obs; std::vector<uint32_t> pdesc;
  std::unordered_map<int32_t, MapPoint*> point_of;
  lld_ref_keyframe kf;
  explicit KeyFrameSide(const KeyFrame* pKF, bool for_projection = false) : kstart(1, 0) {
    const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
    const int n = (int)vpMapPointsKF.size();
    angle.assign(n + 1, 0.f); pos.assign(3 * (size_t)n + 3, 0.f); ids.assign(n + 1, -1); has_obs.assign(n + 1, 0);
    if (for_projection) { maxd.assign(n + 1, 0.f); mind.assign(n + 1, 0.f); pdesc.assign(8 * (size_t)n + 8, 0u); }
    for (int i = 0; i < n; i++) {
      angle[i] = pKF->mvKeysUn[i].angle;
      MapPoint* pMP = vpMapPointsKF[i];
      if (!pMP || pMP->isBad()) continue;                                      // :193-197
      ids[i] = (int32_t)pMP->mnId; point_of[ids[i]] = pMP;
      const lld_slam::Mat P = pMP->GetWorldPos();
      for (int k = 0; k < 3; k++) pos[3 * i + k] = P.at<float>(k);
      has_obs[i] = pMP->Observations() > 0;
      if (for_projection) {                                                    // SearchByProjection(F, pKF, ..) reads these of the MapPoint (:1507-1530)
        maxd[i] = pMP->GetMaxDistance(); mind[i] = pMP->GetMinDistance();
        const lld_slam::MatU8 d = pMP->GetDescriptor();
        std::memcpy(&pdesc[8 * (size_t)i], d.ptr<uint32_t>(), 32);
      }
    }
    for (DBoW2::FeatureVector::const_iterator it = pKF->mFeatVec.begin(); it != pKF->mFeatVec.end(); ++it) {   // a std::map: ascending node ids
      knode.push_back((int32_t)it->first);
      for (size_t j = 0; j < it->second.size(); j++) kfeat.push_back((int32_t)it->second[j]);
      kstart.push_back((int32_t)kfeat.size());
    }
    knode.push_back(0); kfeat.push_back(0);                                    // (never read: non-null pointers for empty lists)
    std::memset(&kf, 0, sizeof kf);
    kf.n = n; kf.desc = pKF->mDescriptors.ptr<uint32_t>(); kf.angle = angle.data(); kf.point_id = ids.data(); kf.world_pos = pos.data(); kf.has_obs = has_obs.data();
    kf.n_nodes = (int)kstart.size() - 1; kf.node = knode.data(); kf.node_start = kstart.data(); kf.feature = kfeat.data();
    static const uint32_t no_desc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (n == 0) kf.desc = no_desc;
  }
  KeyFrameSide(const KeyFrameSide&) = delete;
};

// Frame::UpdatePoseMatrices of a float matrix with the frame's constants
lld_frame_view view_of_matrix(const Frame& Cur, const float* T) {
  lld_frame_view view; std::memset(&view, 0, sizeof view);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) view.Rcw[3 * r + c] = T[4 * r + c];
    view.tcw[r] = T[4 * r + 3];
  }
  for (int r = 0; r < 3; r++) {
    double acc = 0.0;                                                         // mOw = -mRcw.t()*mtcw: one gemm, double accumulation
    for (int k = 0; k < 3; k++) acc += (double)view.Rcw[3 * k + r] * (double)view.tcw[k];
    view.Ow[r] = (float)(-acc);
  }
  view.fx = Cur.fx; view.fy = Cur.fy; view.cx = Cur.cx; view.cy = Cur.cy; view.bf = Cur.mbf;
  view.min_x = Cur.mnMinX; view.max_x = Cur.mnMaxX; view.min_y = Cur.mnMinY; view.max_y = Cur.mnMaxY;
  view.log_scale_factor = Cur.mfLogScaleFactor; view.n_levels = Cur.mnScaleLevels;
  return view;
}

// Matches, PoseOptimization's flags, the statistics loop (src/Tracking.cc:1155-1187) and SetPose from a stage-2 record
void stage2_to_frame(const TrackingMembers& tr, Frame& Cur, const Outputs& out, std::unordered_map<int32_t, MapPoint*>& point_of, std::unordered_map<int32_t, MapLine*>& line_of,
                     int nt, int nl, int* mnMatchesInliers) {
  int inliers = 0;
  for (int k = 0; k < nt; k++) {
    Cur.mvpMapPoints[k] = static_cast<MapPoint*>(NULL);
    if (out.kp_id[k] < 0) { continue; }
    MapPoint* pMP = point_of[out.kp_id[k]];
    Cur.mvbOutlier[k] = out.kp_out[k] != 0;
    if (!out.kp_out[k]) {
      Cur.mvpMapPoints[k] = pMP;
      pMP->IncreaseFound();
      if (!tr.mbOnlyTracking) { if (pMP->Observations() > 0) inliers++; } else inliers++;
    }                                                                          // else: STEREO -> mvpMapPoints[k] = NULL, the flag stays (:1170-1171)
  }
  for (int i = 0; i < nl; i++) {
    if (out.ln_id[i] < 0) { Cur.mvpMapLines[i] = static_cast<MapLine*>(NULL); continue; }
    MapLine* pML = line_of[out.ln_id[i]];
    pML->tracked_last_id = (long)Cur.mnId;
    Cur.mvbOutlierLines[i] = out.ln_out[i] != 0;
    Cur.mvpMapLines[i] = out.ln_out[i] ? static_cast<MapLine*>(NULL) : pML;
  }
  set_pose(Cur, out.r);
  if (mnMatchesInliers) *mnMatchesInliers = inliers;
}

}  // namespace

void FrameOnDevice::create(const Frame& F) {
  lld_ctx* ctx = ctx_;
  std::vector<float> xy(2 * (size_t)F.N + 2), angle(F.N + 1); std::vector<int32_t> octave(F.N + 1);
  for (int k = 0; k < F.N; k++) { xy[2 * k] = F.mvKeysUn[k].pt.x; xy[2 * k + 1] = F.mvKeysUn[k].pt.y; octave[k] = F.mvKeysUn[k].octave; angle[k] = F.mvKeysUn[k].angle; }
  lld_orb_search kp; std::memset(&kp, 0, sizeof kp);
  kp.nt = F.N; kp.t_desc = F.mDescriptors.ptr<uint32_t>(); kp.t_xy = xy.data(); kp.t_octave = octave.data(); kp.t_uright = F.mvuRight.data(); kp.t_angle = angle.data();
  kp.grid_min_x = F.mnMinX; kp.grid_min_y = F.mnMinY; kp.grid_width_inv = F.mfGridElementWidthInv; kp.grid_height_inv = F.mfGridElementHeightInv;
  kp.grid_cols = 64; kp.grid_rows = 48;
  kp.n_levels = F.mnScaleLevels; kp.level_scale = F.mvScaleFactors.data(); kp.level_sigma2 = F.mvLevelSigma2.data(); kp.level_inv_sigma2 = F.mvInvLevelSigma2.data();
  check(lld_frame_create(ctx, &kp, &f_), "lld_frame_create");
  lld_track_params_default(&params_);
  params_.cam = lld_camera{F.fx, F.fy, F.cx, F.cy, F.mbf};
}

FrameOnDevice::FrameOnDevice(lld_ctx* ctx, const Frame& F) : ctx_(ctx), nt_(F.N), nl_((int)F.mvLinesLeft.size()) {
  create(F);
  std::vector<float> left, right; std::vector<int32_t> lo, ro, lm(F.line_matches.begin(), F.line_matches.end());
  key_lines(F.mvLinesLeft, left, lo); key_lines(F.mvLinesRight, right, ro);
  dim_ = nl_ > 0 ? F.mDescriptorsLines.cols : 1;
  lld_frame_lines fl; std::memset(&fl, 0, sizeof fl);
  fl.n_left = nl_; fl.left = left.data(); fl.left_octave = lo.data(); fl.n_right = (int)F.mvLinesRight.size(); fl.right = right.data(); fl.right_octave = ro.data();
  fl.line_matches = lm.data(); fl.desc = nl_ > 0 ? F.mDescriptorsLines.ptr<float>() : nullptr; fl.dim = dim_;
  fl.sx = 1.0 / F.mnMaxX; fl.sy = 1.0 / F.mnMaxY;
  const int st = lld_frame_set_lines(f_, nl_ > 0 ? &fl : nullptr);
  if (st != LLD_OK) { lld_frame_destroy(f_); f_ = nullptr; check(st, "lld_frame_set_lines"); }
}

// The Frame constructor's line half on the device (src/Frame.cc:118-122): lineMatcher.MatchLines(mvLinesLeft, mvLinesRight, mDescriptorsLines,
// mDescriptorsLinesRight, &line_matches) and the upload in one queued call; line_matches comes back for the host's readers (KeyFrame::line_matches,
// the counts of src/Tracking.cc:978).
FrameOnDevice::FrameOnDevice(lld_ctx* ctx, Frame& F, const StereoLineParams& matcher) : ctx_(ctx), nt_(F.N), nl_((int)F.mvLinesLeft.size()) {
  create(F);
  std::vector<float> left, right; std::vector<int32_t> lo, ro;
  key_lines(F.mvLinesLeft, left, lo); key_lines(F.mvLinesRight, right, ro);
  dim_ = nl_ > 0 ? F.mDescriptorsLines.cols : 1;
  const int nr = (int)F.mvLinesRight.size();
  lld_frame_lines_build fl; std::memset(&fl, 0, sizeof fl);
  fl.n_left = nl_; fl.left = left.data(); fl.left_octave = lo.data(); fl.desc_left = nl_ > 0 ? F.mDescriptorsLines.ptr<float>() : nullptr;
  fl.n_right = nr; fl.right = right.data(); fl.right_octave = ro.data(); fl.desc_right = nr > 0 ? F.mDescriptorsLinesRight.ptr<float>() : nullptr;
  fl.dim = dim_; fl.sx = 1.0 / F.mnMaxX; fl.sy = 1.0 / F.mnMaxY;
  for (int i = 0; i < 9; i++) fl.stereo.K[i] = matcher.K[i];
  fl.stereo.b = matcher.b; fl.stereo.tau = matcher.tau; fl.stereo.min_line_length = matcher.minLineLength; fl.stereo.is_stereo = 1;
  int st = lld_frame_build_lines(f_, nl_ > 0 ? &fl : nullptr);
  std::vector<int32_t> lm(nl_ + 1, -1);
  if (st == LLD_OK) st = lld_frame_lines_download(f_, lm.data(), nullptr);
  if (st != LLD_OK) { lld_frame_destroy(f_); f_ = nullptr; check(st, "lld_frame_build_lines"); }
  F.line_matches.assign(lm.begin(), lm.begin() + nl_);
}

// Tracking::MatchLinesLastKF between two frames that are on the device: the call's result drives the object bookkeeping of :1597-1604; nothing is
// gathered.  The device numbers the new lines from MapLine::nNextId in creation order, which is the order the constructors below run in.
int FrameOnDevice::MatchLinesLastKF(const TrackingMembers& tr, Frame& Cur, FrameOnDevice& lastOnDevice, KeyFrame* pKF, lld_slam::Map* mpMap,
                                    std::vector<MapLine*>* created, std::vector<int>* match_trace) {
  const int n = nl_;
  std::vector<int32_t> match_last(n + 1, -1), new_id(n + 1, -1); std::vector<uint8_t> made(n + 1, 0); std::vector<double> X0(3 * (size_t)n + 3, 0.0), dir(3 * (size_t)n + 3, 0.0);
  lld_frame_new_lines_params p; std::memset(&p, 0, sizeof p);
  p.thr_reproj_base = 6; p.md_thr = tr.mdThr; p.use_grid = 1;                // thrReprojLineBase = 6 pixels (:1451)
  p.first_new_id = (int32_t)MapLine::nNextId();
  lld_frame_new_lines_result r; std::memset(&r, 0, sizeof r);
  r.match_last = match_last.data(); r.new_id = new_id.data(); r.created = made.data(); r.x0 = X0.data(); r.dir = dir.data();
  check(lld_frame_new_map_lines(f_, lastOnDevice.f_, &p, &r), "lld_frame_new_map_lines");
  if (created) created->assign(n, static_cast<MapLine*>(NULL));
  for (int i = 0; i < n; i++) {
    if (!made[i]) continue;
    const lld_slam::Vector3d x0(X0[3 * i], X0[3 * i + 1], X0[3 * i + 2]), line_dir(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
    MapLine* ml = new MapLine(x0, line_dir, pKF, mpMap, i);                   // :1597-1604
    if ((int32_t)ml->mnId != new_id[i]) throw std::runtime_error("lld_frame_new_map_lines: MapLine ids left the device's numbering");
    ml->AddObservation(pKF, i);
    pKF->AddMapLine(ml, i);
    ml->ComputeDistinctiveDescriptors();
    Cur.mvpMapLines[i] = ml;
    ml->tracked_last_id = Cur.mnId;
    mpMap->AddMapLine(ml);
    if (created) (*created)[i] = ml;
  }
  if (match_trace) match_trace->assign(match_last.begin(), match_last.begin() + n);
  return r.n_created + r.n_held;                                              // :1610
}

namespace {
void bind(FinishTrace& T, int n) {
  T.created.assign(n + 1, 0); T.new_id.assign(n + 1, -1); T.kp_point_id.assign(n + 1, -1); T.order.assign(n + 1, -1); T.x3d.assign(3 * (size_t)n + 3, 0.f);
  std::memset(&T.r, 0, sizeof T.r);
  T.r.created = T.created.data(); T.r.new_id = T.new_id.data(); T.r.kp_point_id = T.kp_point_id.data(); T.r.order = T.order.data(); T.r.x3d = T.x3d.data();
}
// the created keypoints in visiting order: the order the reference's loop runs its constructors in
std::vector<int> creation_order(const FinishTrace& T, int n) {
  std::vector<int> at(n + 1, -1);                                             // at[rank] = keypoint
  for (int i = 0; i < n; i++) if (T.order[i] >= 0) at[T.order[i]] = i;
  std::vector<int> made;
  for (int j = 0; j < n; j++) if (at[j] >= 0 && T.created[at[j]]) made.push_back(at[j]);
  return made;
}
lld_slam::Mat point_of_result(const FinishTrace& T, int i) { return lld_slam::Mat(3, 1, &T.x3d[3 * (size_t)i]); }
}  // namespace

// The frame was made by lld_frame_create, which keeps no depth: mvDepth travels with the call.
bool FrameOnDevice::NeedNewKeyFrame(const TrackingMembers& tr, const KeyFrameDecision& d, Frame& Cur, bool* interruptBA, FinishTrace* trace) {
  for (int i = 0; i < nt_; i++) {                                             // Clean VO matches (:446-453)
    MapPoint* pMP = Cur.mvpMapPoints[i];
    if (pMP && pMP->Observations() < 1) { Cur.mvbOutlier[i] = false; Cur.mvpMapPoints[i] = static_cast<MapPoint*>(NULL); }
  }
  lld_frame_finish_params p; std::memset(&p, 0, sizeof p);
  p.th_depth = d.mThDepth; p.first_new_id = (int32_t)MapPoint::nNextId(); p.force = -1;
  p.only_tracking = tr.mbOnlyTracking; p.mapper_stopped = d.mapperStopped; p.mapper_idle = d.bLocalMappingIdle; p.keyframes_in_queue = d.KeyframesInQueue;
  p.set_not_stop_ok = d.setNotStopOk; p.monocular = d.monocular; p.sensor_rgbd = d.rgbd; p.max_frames = d.mMaxFrames; p.min_frames = d.mMinFrames;
  p.n_keyframes = d.nKFs; p.n_ref_matches = d.nRefMatches; p.n_matches_inliers = d.mnMatchesInliers;
  p.frame_id = (int64_t)Cur.mnId; p.last_reloc_frame_id = (int64_t)d.mnLastRelocFrameId; p.last_keyframe_id = (int64_t)d.mnLastKeyFrameId;
  p.depth = Cur.mvDepth.data();
  bind(finish_, nt_);
  check(lld_frame_track_finish(f_, &p, &finish_.r), "lld_frame_track_finish");
  finish_made_ = finish_.r.made != 0;
  if (interruptBA) *interruptBA = finish_.r.interrupt_ba != 0;
  if (trace) {                                                                // a copy whose pointers name its own arrays
    *trace = finish_;
    trace->r.created = trace->created.data(); trace->r.new_id = trace->new_id.data(); trace->r.kp_point_id = trace->kp_point_id.data();
    trace->r.order = trace->order.data(); trace->r.x3d = trace->x3d.data();
  }
  return finish_.r.need != 0;
}

void FrameOnDevice::CreateNewKeyFrame(const TrackingMembers& tr, Frame& Cur, KeyFrame* pKF, lld_slam::Map* mpMap, FrameOnDevice* lastOnDevice, std::vector<MapPoint*>* created) {
  if (created) created->assign(nt_, static_cast<MapPoint*>(NULL));
  if (!finish_made_) return;                                                  // :1369
  const std::vector<int> made = creation_order(finish_, nt_);
  for (size_t k = 0; k < made.size(); k++) {                                  // :1399-1429, the entries with bCreateNew
    const int i = made[k];
    MapPoint* pNewMP = new MapPoint(point_of_result(finish_, i), pKF, mpMap);
    if ((int32_t)pNewMP->mnId != finish_.new_id[i]) throw std::runtime_error("lld_frame_track_finish: MapPoint ids left the device's numbering");
    pNewMP->AddObservation(pKF, i);
    pKF->AddMapPoint(pNewMP, i);
    mpMap->AddMapPoint(pNewMP);
    Cur.mvpMapPoints[i] = pNewMP;
    if (created) (*created)[i] = pNewMP;
  }
  if (lastOnDevice && nl_ > 0) MatchLinesLastKF(tr, Cur, *lastOnDevice, pKF, mpMap);   // :1432-1434
}

void FrameOnDevice::DropOutliers(Frame& Cur) const {
  for (int i = 0; i < nt_; i++)                                               // :472-476
    if (Cur.mvpMapPoints[i] && Cur.mvbOutlier[i]) Cur.mvpMapPoints[i] = static_cast<MapPoint*>(NULL);
}

void FrameOnDevice::UpdateLastFrame(const TrackingMembers& tr, float mThDepth, Frame& Last, lld_slam::Map* mpMap, std::vector<MapPoint*>* mlpTemporalPoints) {
  params_.pose.gamma = tr.gamma; params_.line_md_thr = tr.mdThr;
  const lld_frame_view view = view_of(Last);                                  // mLastFrame.SetPose(Tlr*pRef->GetPose()) ran (:825)
  double qt[7];
  lld_se3_from_tcw_f32(Last.mTcw.ptr<float>(), qt);
  lld_frame_points_params p; std::memset(&p, 0, sizeof p);
  p.mode = LLD_POINTS_LAST_FRAME; p.th_depth = mThDepth; p.first_new_id = (int32_t)MapPoint::nNextId(); p.params = &params_; p.view = &view; p.pose_qt = qt;
  p.depth = Last.mvDepth.data();
  FinishTrace T; bind(T, nt_);
  check(lld_frame_create_stereo_points(f_, &p, &T.r), "lld_frame_create_stereo_points");
  const std::vector<int> made = creation_order(T, nt_);
  for (size_t k = 0; k < made.size(); k++) {                                  // :865-874
    const int i = made[k];
    MapPoint* pNewMP = new MapPoint(point_of_result(T, i), static_cast<KeyFrame*>(NULL), mpMap);
    if ((int32_t)pNewMP->mnId != T.new_id[i]) throw std::runtime_error("lld_frame_create_stereo_points: MapPoint ids left the device's numbering");
    Last.mvpMapPoints[i] = pNewMP;
    if (mlpTemporalPoints) mlpTemporalPoints->push_back(pNewMP);
  }
}

FrameOnDevice::~FrameOnDevice() { if (f_) lld_frame_destroy(f_); }

bool FrameOnDevice::TrackWithMotionModel(const TrackingMembers& tr, Frame& Cur, const Frame& Last, bool* mbVO, TrackTrace* trace) {
  params_.pose.gamma = tr.gamma; params_.line_md_thr = tr.mdThr;
  // ---- gather LastFrame.mvpMapPoints (src/ORBmatcher.cc:1352-1358, :1381, :1435) and the direction test (:1338-1350)
  const int n = Last.N;
  std::vector<float> pos(3 * (size_t)n + 3, 0.f), angle(n + 1, 0.f); std::vector<uint8_t> valid(n + 1, 0), has_obs(n + 1, 0);
  std::vector<int32_t> octave(n + 1, 0), ids(n + 1, 0); std::vector<uint32_t> desc(8 * (size_t)n + 8, 0u);
  std::unordered_map<int32_t, MapPoint*> point_of;
  for (int i = 0; i < n; i++) {
    MapPoint* pMP = Last.mvpMapPoints[i];
    if (!pMP || Last.mvbOutlier[i]) continue;
    valid[i] = 1; ids[i] = (int32_t)pMP->mnId; point_of[ids[i]] = pMP;
    const lld_slam::Mat x3Dw = pMP->GetWorldPos();
    for (int k = 0; k < 3; k++) pos[3 * i + k] = x3Dw.at<float>(k);
    octave[i] = Last.mvKeys[i].octave; angle[i] = Last.mvKeysUn[i].angle;
    const lld_slam::MatU8 d = pMP->GetDescriptor();
    std::memcpy(&desc[8 * (size_t)i], d.ptr<unsigned char>(), 32);
    has_obs[i] = pMP->Observations() > 0;
  }
  lld_last_frame_points last; std::memset(&last, 0, sizeof last);
  last.n = n; last.world_pos = pos.data(); last.valid = valid.data(); last.octave = octave.data(); last.angle = angle.data(); last.desc = desc.data(); last.has_obs = has_obs.data();
  {
    double accz = 0.0;                                                        // tlc = Rlw*twc+tlw, twc = mOw of the current frame
    for (int k = 0; k < 3; k++) accz += (double)Last.mTcw.at<float>(2, k) * (double)Cur.mOw.at<float>(k);
    const float tlc2 = (float)(accz + (double)Last.mTcw.at<float>(2, 3));
    params_.direction = (tlc2 > Cur.mb) ? 1 : ((-tlc2 > Cur.mb) ? -1 : 0);
  }
  LineSide lines(Last.mvpMapLines, nullptr, &Last.mDescriptorsLines, dim_, Cur.mnId);
  std::unordered_map<int32_t, MapLine*> line_of;
  for (size_t i = 0; i < Last.mvpMapLines.size(); i++) if (Last.mvpMapLines[i]) line_of[(int32_t)Last.mvpMapLines[i]->mnId] = Last.mvpMapLines[i];
  // ---- the stage
  const lld_frame_view view = view_of(Cur);
  double qt[7];
  lld_se3_from_tcw_f32(Cur.mTcw.ptr<float>(), qt);                            // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw))
  check(lld_frame_track_motion_model(f_, &params_, &view, qt, &last, ids.data(), nl_ > 0 ? &lines.m : nullptr), "lld_frame_track_motion_model");
  Outputs out(nt_, nl_, 0);
  check(lld_frame_track_download(f_, &out.r, nullptr), "lld_frame_track_download");
  out.to(trace, nt_, nl_, 0);
  if (out.r.n_search < 10) {
    // :913-917: the reference returns before AddLinesFrom and PoseOptimization.  The frame holds the raw matches of the search used (the
    // stage-1 record's ids), mvbOutlier stays false, no MapLine, the predicted pose; no MapPoint / MapLine is marked.  The chain has run
    // on, so the device frame is handed this state back: it never holds what the object graph lacks.
    for (int k = 0; k < nt_; k++) {
      Cur.mvpMapPoints[k] = out.kp_id[k] >= 0 ? point_of[out.kp_id[k]] : static_cast<MapPoint*>(NULL);
      Cur.mvbOutlier[k] = false;
    }
    SetFrameState(tr, Cur);
    return false;
  }
  // ---- write-back: matches, PoseOptimization's flags, the outlier discard (:940-975)
  for (int k = 0; k < nt_; k++) {
    Cur.mvpMapPoints[k] = static_cast<MapPoint*>(NULL); Cur.mvbOutlier[k] = false;
    if (out.kp_id[k] < 0) continue;
    MapPoint* pMP = point_of[out.kp_id[k]];
    if (out.kp_out[k]) { pMP->mbTrackInView = false; pMP->mnLastFrameSeen = Cur.mnId; }
    else Cur.mvpMapPoints[k] = pMP;
  }
  for (int i = 0; i < nl_; i++) {
    if (out.ln_id[i] < 0) continue;
    MapLine* pML = line_of[out.ln_id[i]];
    pML->tracked_last_id = (long)Cur.mnId;                                    // AddLinesFrom (:1117); stays when the line is thrown out below
    Cur.mvbOutlierLines[i] = out.ln_out[i] != 0;
    Cur.mvpMapLines[i] = out.ln_out[i] ? static_cast<MapLine*>(NULL) : pML;
  }
  set_pose(Cur, out.r);
  if (tr.mbOnlyTracking) { if (mbVO) *mbVO = out.r.n_points_map < 10; return out.r.n_points > 20; }
  return out.r.n_points_map >= 7;
}

// mCurrentFrame.ComputeBoW(): the FeatureVector stays on the device; the host copy goes into the Frame
void FrameOnDevice::ComputeBoW(Frame& Cur, lld_bow_vocab* voc, int levelsup) {
  const int m = nt_ + 1;
  std::vector<int32_t> word(m), node(m), start(m + 1), feat(m); std::vector<double> value(m);
  lld_bow_result R; std::memset(&R, 0, sizeof R);
  R.word = word.data(); R.value = value.data(); R.node = node.data(); R.node_start = start.data(); R.feature = feat.data();
  check(lld_frame_compute_bow(f_, voc, levelsup, &R), "lld_frame_compute_bow");
  Cur.mFeatVec.clear();
  for (int i = 0; i < R.n_nodes; i++) Cur.mFeatVec[(unsigned int)node[i]].assign(feat.begin() + start[i], feat.begin() + start[i + 1]);
}

bool FrameOnDevice::Relocalization(const TrackingMembers& tr, Frame& Cur, const std::vector<KeyFrame*>& vpCandidateKFs, lld_bow_vocab* voc, int levelsup,
                                   const std::vector<uint32_t>* seeds, RelocTrace* trace) {
  params_.pose.gamma = tr.gamma; params_.line_md_thr = tr.mdThr;
  if (voc) ComputeBoW(Cur, voc, levelsup);                                     // :1840 (NULL: the caller ran ComputeBoW on this object to query the database)
  const int K = (int)vpCandidateKFs.size();
  if (K == 0) return false;                                                    // :1846-1847
  if (seeds && (int)seeds->size() != K) check(LLD_ERR_INVALID, "FrameOnDevice::Relocalization: one seed per candidate");
  std::vector<std::unique_ptr<KeyFrameSide>> sides;
  std::vector<lld_ref_keyframe> kfs(K); std::vector<lld_reloc_candidate> ex(K);
  for (int i = 0; i < K; i++) {
    sides.emplace_back(new KeyFrameSide(vpCandidateKFs[i], true));
    KeyFrameSide& s = *sides.back();
    kfs[i] = s.kf;
    std::memset(&ex[i], 0, sizeof ex[i]);
    ex[i].max_distance = s.maxd.data(); ex[i].min_distance = s.mind.data(); ex[i].point_desc = s.pdesc.data();
    ex[i].is_bad = vpCandidateKFs[i]->isBad(); ex[i].seed = seeds ? (*seeds)[i] : (uint32_t)i;
  }
  // the pose the frame keeps when nothing matches: what it holds now (a lost frame may hold none: identity)
  float T0[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (!Cur.mTcw.empty()) std::memcpy(T0, Cur.mTcw.ptr<float>(), sizeof T0);
  const lld_frame_view view = view_of_matrix(Cur, T0);
  double qt[7];
  lld_se3_from_tcw_f32(T0, qt);
  lld_pnp_params prm; lld_pnp_params_default(&prm);                            // SetRansacParameters(0.99,10,300,4,0.5,5.991) (:1882)
  RelocTrace local; RelocTrace& R = trace ? *trace : local;
  R.n_bow.assign(K, 0); R.rounds.assign(K, 0); R.n_good_last.assign(K, -1); R.rungs.assign(K, 0); R.n_additional1.assign(K, 0); R.n_additional2.assign(K, 0);
  R.discarded.assign(K, 0);
  std::memset(&R.r, 0, sizeof R.r);
  R.r.n_bow = R.n_bow.data(); R.r.rounds = R.rounds.data(); R.r.n_good_last = R.n_good_last.data(); R.r.rungs = R.rungs.data();
  R.r.n_additional1 = R.n_additional1.data(); R.r.n_additional2 = R.n_additional2.data(); R.r.discarded = R.discarded.data();
  check(lld_frame_relocalize(f_, &params_, &view, qt, K, kfs.data(), ex.data(), &prm, &R.r), "lld_frame_relocalize");
  if (!R.r.matched) return false;                                              // the objects stay untouched (:1988-1991)
  // ---- write-back: what the winning attempt left in the frame (:1919-1971): mTcw, mvpMapPoints, mvbOutlier of the held points
  Outputs out(nt_, nl_, 0);
  check(lld_frame_track_download(f_, &out.r, nullptr), "lld_frame_track_download");
  KeyFrameSide& w = *sides[R.r.winner];
  for (int k = 0; k < nt_; k++) {
    Cur.mvpMapPoints[k] = out.kp_id[k] >= 0 ? w.point_of[out.kp_id[k]] : static_cast<MapPoint*>(NULL);
    Cur.mvbOutlier[k] = out.kp_id[k] >= 0 && out.kp_out[k] != 0;
  }
  Cur.SetPose(lld_slam::Mat(4, 4, R.r.Tcw));
  return true;                                                                 // the caller sets mnLastRelocFrameId (:1994)
}

bool FrameOnDevice::TrackReferenceKeyFrame(const TrackingMembers& tr, Frame& Cur, const Frame& Last, const KeyFrame* pKF, lld_bow_vocab* voc, int levelsup, TrackTrace* trace) {
  params_.pose.gamma = tr.gamma; params_.line_md_thr = tr.mdThr;
  if (voc) ComputeBoW(Cur, voc, levelsup);                                     // mCurrentFrame.ComputeBoW() (:776); NULL: done on this object already
  // ---- gather mpReferenceKF; the stage starts from mLastFrame.mTcw (:789): Frame::UpdatePoseMatrices of that matrix with this frame's constants
  KeyFrameSide side(pKF);
  const lld_ref_keyframe& kf = side.kf;
  std::unordered_map<int32_t, MapPoint*>& point_of = side.point_of;
  const lld_frame_view view = view_of_matrix(Cur, Last.mTcw.ptr<float>());
  double qt[7];
  lld_se3_from_tcw_f32(Last.mTcw.ptr<float>(), qt);
  check(lld_frame_track_reference_keyframe(f_, &params_, &view, qt, &kf), "lld_frame_track_reference_keyframe");
  Outputs out(nt_, nl_, 0);
  check(lld_frame_track_download(f_, &out.r, nullptr), "lld_frame_track_download");
  out.to(trace, nt_, nl_, 0);
  if (out.r.n_search < 15) {
    // :785-786: the reference returns before it assigns the matches or sets the pose.  The chain has run on, so the device frame is handed
    // back what the objects hold (possible only once the frame has a pose).
    if (!Cur.mTcw.empty()) SetFrameState(tr, Cur);
    return false;
  }
  // ---- write-back: mvpMapPoints = vpMapPointMatches (:788), SetPose (:789), PoseOptimization, the discard (:796-814)
  Cur.SetPose(Last.mTcw);
  for (int k = 0; k < nt_; k++) {
    Cur.mvpMapPoints[k] = static_cast<MapPoint*>(NULL);
    if (out.kp_id[k] < 0) continue;
    MapPoint* pMP = point_of[out.kp_id[k]];
    Cur.mvbOutlier[k] = false;                                                 // cleared by PoseOptimization for an inlier, by the discard for an outlier (:806)
    if (out.kp_out[k]) { pMP->mbTrackInView = false; pMP->mnLastFrameSeen = Cur.mnId; }
    else Cur.mvpMapPoints[k] = pMP;
  }
  set_pose(Cur, out.r);
  return out.r.n_points_map >= 10;
}

void FrameOnDevice::SetFrameState(const TrackingMembers& tr, const Frame& Cur) {
  params_.pose.gamma = tr.gamma; params_.line_md_thr = tr.mdThr;
  std::vector<int32_t> kp_id(nt_ + 1, -1), ln_id(nl_ + 1, -1); std::vector<float> world(3 * (size_t)nt_ + 3, 0.f); std::vector<uint8_t> obs(nt_ + 1, 0), out(nt_ + 1, 0), lout(nl_ + 1, 0);
  std::vector<double> x0(3 * (size_t)nl_ + 3, 0.0), dir(3 * (size_t)nl_ + 3, 0.0);
  for (int k = 0; k < nt_; k++) {
    MapPoint* pMP = Cur.mvpMapPoints[k];
    out[k] = Cur.mvbOutlier[k];
    if (!pMP) continue;
    kp_id[k] = (int32_t)pMP->mnId; obs[k] = pMP->Observations() > 0;
    const lld_slam::Mat P = pMP->GetWorldPos();
    for (int c = 0; c < 3; c++) world[3 * k + c] = P.at<float>(c);
  }
  for (int i = 0; i < nl_; i++) {
    MapLine* pML = i < (int)Cur.mvpMapLines.size() ? Cur.mvpMapLines[i] : static_cast<MapLine*>(NULL);
    lout[i] = i < (int)Cur.mvbOutlierLines.size() && Cur.mvbOutlierLines[i];
    if (!pML) continue;
    ln_id[i] = (int32_t)pML->mnId;
    lld_slam::Vector3d a, d;
    pML->GetMinimalPos(&a, &d);
    for (int c = 0; c < 3; c++) { x0[3 * i + c] = a(c); dir[3 * i + c] = d(c); }
  }
  lld_frame_held held; std::memset(&held, 0, sizeof held);
  held.kp_point_id = kp_id.data(); held.kp_world_pos = world.data(); held.kp_has_obs = obs.data(); held.kp_outlier = out.data();
  held.ln_line_id = ln_id.data(); held.ln_x0 = x0.data(); held.ln_dir = dir.data(); held.ln_outlier = lout.data();
  // (MapPoints / MapLines this frame marked without holding them - mnLastFrameSeen, tracked_last_id - are skipped by TrackLocalMap's own gather)
  const lld_frame_view view = view_of(Cur);
  double qt[7];
  lld_se3_from_tcw_f32(Cur.mTcw.ptr<float>(), qt);
  check(lld_frame_track_set_state(f_, &params_, &view, qt, &held), "lld_frame_track_set_state");
}

void FrameOnDevice::TrackLocalMap(const TrackingMembers& tr, Frame& Cur, const std::vector<MapPoint*>& mvpLocalMapPoints, const std::vector<MapLine*>& local_lines,
                                  const std::vector<lld_slam::Mat>& local_line_descs, int* mnMatchesInliers, TrackTrace* trace) {
  params_.pose.gamma = tr.gamma; params_.line_md_thr = tr.mdThr;
  params_.th_local = tr.just_relocalised ? 5.f : 1.f;
  // ---- SearchLocalPoints, first loop (:1616-1633): host bookkeeping on the MapPoints the frame holds
  std::unordered_map<int32_t, MapPoint*> point_of;
  for (int k = 0; k < nt_; k++) {
    MapPoint* pMP = Cur.mvpMapPoints[k];
    if (!pMP) continue;
    pMP->IncreaseVisible(); pMP->mnLastFrameSeen = Cur.mnId; pMP->mbTrackInView = false;
    point_of[(int32_t)pMP->mnId] = pMP;
  }
  // ---- gather the local map (as lld_orb_search_local_points)
  const int n = (int)mvpLocalMapPoints.size();
  std::vector<float> pos(3 * (size_t)n + 3), nrm(3 * (size_t)n + 3), maxd(n + 1), mind(n + 1); std::vector<uint32_t> desc(8 * (size_t)n + 8);
  std::vector<uint8_t> has_obs(n + 1, 0), skip(n + 1, 1); std::vector<int32_t> ids(n + 1, 0);
  for (int i = 0; i < n; i++) {
    MapPoint* pMP = mvpLocalMapPoints[i];
    ids[i] = (int32_t)pMP->mnId; point_of[ids[i]] = pMP;
    if (pMP->isBad() || pMP->mnLastFrameSeen == Cur.mnId) continue;          // :1639-1642 (the device skips the same ones by id; the objects are the authority)
    skip[i] = 0;
    const lld_slam::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal();
    for (int k = 0; k < 3; k++) { pos[3 * i + k] = P.at<float>(k); nrm[3 * i + k] = Pn.at<float>(k); }
    maxd[i] = pMP->GetMaxDistance(); mind[i] = pMP->GetMinDistance();
    const lld_slam::MatU8 d = pMP->GetDescriptor();
    std::memcpy(&desc[8 * (size_t)i], d.ptr<unsigned char>(), 32);
    has_obs[i] = pMP->Observations() > 0;
  }
  lld_map_points mp; std::memset(&mp, 0, sizeof mp);
  mp.n = n; mp.world_pos = pos.data(); mp.normal = nrm.data(); mp.max_distance = maxd.data(); mp.min_distance = mind.data(); mp.desc = desc.data(); mp.has_obs = has_obs.data();
  mp.skip = skip.data();
  LineSide lines(local_lines, &local_line_descs, nullptr, dim_, Cur.mnId);
  std::unordered_map<int32_t, MapLine*> line_of;
  for (int i = 0; i < nl_; i++) if (Cur.mvpMapLines[i]) line_of[(int32_t)Cur.mvpMapLines[i]->mnId] = Cur.mvpMapLines[i];
  for (size_t i = 0; i < local_lines.size(); i++) if (local_lines[i]) line_of[(int32_t)local_lines[i]->mnId] = local_lines[i];
  // ---- the stage
  check(lld_frame_track_local_map(f_, &params_, &mp, ids.data(), nl_ > 0 ? &lines.m : nullptr), "lld_frame_track_local_map");
  Outputs out(nt_, nl_, n);
  check(lld_frame_track_download(f_, nullptr, &out.r), "lld_frame_track_download");
  out.to(trace, nt_, nl_, n);
  // ---- what Frame::isInFrustum and the loop around it leave in the MapPoints (:1637-1650)
  for (int i = 0; i < n; i++) {
    if (skip[i]) continue;
    MapPoint* pMP = mvpLocalMapPoints[i];
    pMP->mbTrackInView = out.in_view[i] != 0;
    if (out.in_view[i]) pMP->IncreaseVisible();
  }
  stage2_to_frame(tr, Cur, out, point_of, line_of, nt_, nl_, mnMatchesInliers);
}

void FrameOnDevice::TrackLocalMap(const TrackingMembers& tr, Frame& Cur, MapOnDevice& map, LocalMapMembers& lm, int* mnMatchesInliers, TrackTrace* trace,
                                  lld_local_map_result* rec) {
  params_.pose.gamma = tr.gamma; params_.line_md_thr = tr.mdThr;
  params_.th_local = tr.just_relocalised ? 5.f : 1.f;
  const lld_map_limits& L = map.limits();
  // ---- UpdateLocalKeyFrames' side effect on the frame (:1741-1744): the device takes the same MapPoints out of its copy
  for (int k = 0; k < nt_; k++) if (Cur.mvpMapPoints[k] && Cur.mvpMapPoints[k]->isBad()) Cur.mvpMapPoints[k] = static_cast<MapPoint*>(NULL);
  // ---- the three calls
  check(lld_frame_track_update_local_map(f_, map.get()), "lld_frame_track_update_local_map");
  check(lld_frame_track_local_map_resident(f_, &params_, map.get()), "lld_frame_track_local_map_resident");
  const int n_max = L.max_local_points;
  Outputs out(nt_, nl_, n_max);
  std::vector<int32_t> kfs(LLD_MAP_MAX_LOCAL_KEYFRAMES, -1), pts(n_max + 1, -1), lns(L.max_local_lines + 1, -1);
  lld_local_map_result R; std::memset(&R, 0, sizeof R);
  R.local_keyframes = kfs.data(); R.local_points = pts.data(); R.local_lines = lns.data(); R.mp_in_view = out.in_view.data(); R.stage2 = &out.r;
  check(lld_frame_local_map_download(f_, map.get(), &R), "lld_frame_local_map_download");
  if (rec) { *rec = R; rec->local_keyframes = nullptr; rec->local_points = nullptr; rec->local_lines = nullptr; rec->mp_in_view = nullptr; rec->stage1 = nullptr; rec->stage2 = nullptr; }
  if (R.status != 0) throw std::runtime_error("FrameOnDevice::TrackLocalMap: the local map exceeds the resident map's limits (lld_local_map_result.status " + std::to_string(R.status) + ")");
  // ---- what UpdateLocalMap leaves on Tracking and in the objects (:1684-1722, :1758-1834)
  lm.mvpLocalKeyFrames.clear(); lm.mvpLocalMapPoints.clear(); lm.local_lines.clear(); lm.local_line_descs.clear();
  for (int i = 0; i < R.n_local_keyframes; i++) {
    KeyFrame* pKF = map.KeyFrameOf(kfs[i]);
    lm.mvpLocalKeyFrames.push_back(pKF);
    if (!R.vote_empty) pKF->mnTrackReferenceForFrame = Cur.mnId;              // (after an empty vote the routine returned before it marked anything, :1748)
  }
  if (R.ref_keyframe >= 0) { lm.mpReferenceKF = map.KeyFrameOf(R.ref_keyframe); Cur.mpReferenceKF = lm.mpReferenceKF; }
  for (int i = 0; i < R.n_local_points; i++) { MapPoint* pMP = map.PointOf(pts[i]); lm.mvpLocalMapPoints.push_back(pMP); pMP->mnTrackReferenceForFrame = Cur.mnId; }
  for (int i = 0; i < R.n_local_lines; i++) {
    MapLine* pML = map.LineOf(lns[i]);
    lm.local_lines.push_back(pML); pML->mnTrackReferenceForFrame = (long)Cur.mnId;
    lld_slam::Mat ml_desc; pML->GetDescriptor(&ml_desc); lm.local_line_descs.push_back(ml_desc);
  }
  // ---- SearchLocalPoints' bookkeeping (:1616-1650), in the order of the TrackLocalMap above
  std::unordered_map<int32_t, MapPoint*> point_of;
  for (int k = 0; k < nt_; k++) {
    MapPoint* pMP = Cur.mvpMapPoints[k];
    if (!pMP) continue;
    pMP->IncreaseVisible(); pMP->mnLastFrameSeen = Cur.mnId; pMP->mbTrackInView = false;
    point_of[(int32_t)pMP->mnId] = pMP;
  }
  for (int i = 0; i < R.n_local_points; i++) {
    MapPoint* pMP = lm.mvpLocalMapPoints[i];
    point_of[pts[i]] = pMP;
    if (pMP->isBad() || pMP->mnLastFrameSeen == Cur.mnId) continue;
    pMP->mbTrackInView = out.in_view[i] != 0;
    if (out.in_view[i]) pMP->IncreaseVisible();
  }
  std::unordered_map<int32_t, MapLine*> line_of;
  for (int i = 0; i < nl_; i++) if (Cur.mvpMapLines[i]) line_of[(int32_t)Cur.mvpMapLines[i]->mnId] = Cur.mvpMapLines[i];
  for (int i = 0; i < R.n_local_lines; i++) line_of[lns[i]] = lm.local_lines[i];
  out.to(trace, nt_, nl_, R.n_local_points);
  stage2_to_frame(tr, Cur, out, point_of, line_of, nt_, nl_, mnMatchesInliers);
}

}  // namespace lld_adapter
