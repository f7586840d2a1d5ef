// lld_tracking_adapter.h — host adapter for the Tracking thread's per-frame chain on live SLAM objects (round 6):
//   bool Tracking::TrackWithMotionModel()   src/Tracking.cc:885-994   (from `mCurrentFrame.SetPose(mVelocity*mLastFrame.mTcw)` on)
//   bool Tracking::TrackLocalMap()          src/Tracking.cc:1126-1220 (after UpdateLocalMap())
//   bool Tracking::TrackReferenceKeyFrame() src/Tracking.cc:773-817   (the other common way into TrackLocalMap)
//   bool Tracking::Relocalization()         src/Tracking.cc:1837-1998 (the third)
// All run as ONE device-resident sequence (lld_frame_track_*, include/lld_amd.h): the frame's keypoints and lines go to the device once
// (FrameOnDevice's constructor - the last step of the reference's Frame constructor), each routine gathers its map-side inputs, queues
// its stage, fetches the stage's record and writes it back into the objects the way the reference's loops do (mvpMapPoints / mvbOutlier /
// mvpMapLines / mvbOutlierLines / mTcw of the frame; mnLastFrameSeen, mbTrackInView, IncreaseVisible / IncreaseFound of the MapPoints;
// tracked_last_id of the MapLines).  Same object model switch as lld_optimizer_adapter.h (LLD_ADAPTER_OBJECTS_HEADER).
// MapPoints and MapLines are named on the device by their mnId (ids below 2^31).
#ifndef LLD_TRACKING_ADAPTER_H
#define LLD_TRACKING_ADAPTER_H

#include <vector>

#include "../include/lld_amd.h"

#ifndef LLD_ADAPTER_OBJECTS_HEADER
#define LLD_ADAPTER_OBJECTS_HEADER "lld_slam_objects.h"
#endif
#include LLD_ADAPTER_OBJECTS_HEADER
#include "lld_map_adapter.h"

namespace lld_adapter {

using lld_slam::Frame;
using lld_slam::KeyFrame;
using lld_slam::MapLine;
using lld_slam::MapPoint;

struct TrackingMembers {          // what the two routines read off `this` (include/Tracking.h)
  double gamma = 0.5;             // yaml `gamma`
  double mdThr = 0.9;             // yaml mdThr
  bool mbOnlyTracking = false;
  bool just_relocalised = false;  // mCurrentFrame.mnId < mnLastRelocFrameId + 2: SearchLocalPoints uses th = 5 (:1656-1658)
};

// What Tracking::UpdateLocalMap writes on `this` (include/Tracking.h): the local map, and the reference keyframe
struct LocalMapMembers {
  std::vector<KeyFrame*> mvpLocalKeyFrames;
  std::vector<MapPoint*> mvpLocalMapPoints;
  std::vector<MapLine*> local_lines;
  std::vector<lld_slam::Mat> local_line_descs;
  KeyFrame* mpReferenceKF = nullptr;
};

// What one stage got back (optional; the tests read it, a live system passes nullptr).
struct TrackTrace { lld_track_result r; std::vector<int32_t> kp_point_id, ln_line_id; std::vector<uint8_t> kp_outlier, ln_outlier, mp_in_view; };

// What Relocalization got back (optional, as TrackTrace): lld_reloc_result with its per-candidate arrays owned here.
struct RelocTrace { lld_reloc_result r; std::vector<int32_t> n_bow, rounds, n_good_last, rungs, n_additional1, n_additional2; std::vector<uint8_t> discarded; };

// What Tracking::NeedNewKeyFrame and CreateNewKeyFrame read off `this`, mpLocalMapper and mpMap (src/Tracking.cc:1227-1309, :1369), gathered by the
// caller before the one device call that decides and creates.
struct KeyFrameDecision {
  float mThDepth = 0;
  bool mapperStopped = false;          // mpLocalMapper->isStopped() || mpLocalMapper->stopRequested() (:1231)
  bool bLocalMappingIdle = true;       // mpLocalMapper->AcceptKeyFrames() (:1247)
  int KeyframesInQueue = 0;            // mpLocalMapper->KeyframesInQueue() (:1299)
  bool setNotStopOk = true;            // mpLocalMapper->SetNotStop(true) (:1369): taken before the call; the caller undoes it (SetNotStop(false)) when no keyframe is made
  int nKFs = 0;                        // mpMap->KeyFramesInMap()
  int nRefMatches = 0;                 // mpReferenceKF->TrackedMapPoints(nKFs <= 2 ? 2 : 3)
  int mnMatchesInliers = 0;
  int mMaxFrames = 0, mMinFrames = 0;
  unsigned long mnLastRelocFrameId = 0, mnLastKeyFrameId = 0;
  bool monocular = false, rgbd = false;   // mSensor
};
// What the tail of Track() got back (optional, as TrackTrace): lld_frame_finish_result with its arrays owned here.
struct FinishTrace { lld_frame_finish_result r; std::vector<uint8_t> created; std::vector<int32_t> new_id, kp_point_id, order; std::vector<float> x3d; };

// TwoFrameLineMatcher's constructor arguments (include/TwoFrameLineMatcher.h:31-38) as the Frame constructor passes them (src/Frame.cc:118-121)
struct StereoLineParams { double K[9]; double b; double tau; int minLineLength; };

class FrameOnDevice {
 public:
  // the frame's own data: mDescriptors, mvKeysUn, mvuRight, the grid and level tables, mvLinesLeft / mvLinesRight / line_matches / mDescriptorsLines
  FrameOnDevice(lld_ctx* ctx, const Frame& mCurrentFrame);
  // the same, with the lines matched on the device (lld_frame_build_lines): mCurrentFrame brings mDescriptorsLinesRight instead of line_matches,
  // which this constructor fills from the call's download - lineMatcher.MatchLines(...) of src/Frame.cc:121-122 is not run on the host
  FrameOnDevice(lld_ctx* ctx, Frame& mCurrentFrame, const StereoLineParams& matcher);
  ~FrameOnDevice();
  FrameOnDevice(const FrameOnDevice&) = delete;
  FrameOnDevice& operator=(const FrameOnDevice&) = delete;

  // bool Tracking::TrackWithMotionModel(): the caller has run UpdateLastFrame() and mCurrentFrame.SetPose(mVelocity*mLastFrame.mTcw), and
  // cleared mCurrentFrame.mvpMapPoints (:897).  *mbVO as the reference sets it in localisation mode (:985).  Below 10 matches (:913-917) the
  // frame keeps only the raw matches of the search, with mvbOutlier false, no MapLines, the predicted pose and no marks on any MapPoint / MapLine;
  // the device frame is set to that state, so TrackLocalMap may follow it on this object as after SetFrameState.
  bool TrackWithMotionModel(const TrackingMembers& tr, Frame& mCurrentFrame, const Frame& mLastFrame, bool* mbVO = nullptr, TrackTrace* trace = nullptr);
  // mCurrentFrame.ComputeBoW() on the resident descriptors (lld_frame_compute_bow): the FeatureVector stays on the device with the frame, mFeatVec is
  // filled from the call's host result; `voc` belongs to this frame's context.  The two routines below run it themselves unless they are handed
  // voc = NULL, which says it has been run on this object - Relocalization's caller needs the frame's vectors for DetectRelocalizationCandidates
  // (:1844) before it has any candidate to hand over.
  void ComputeBoW(Frame& mCurrentFrame, lld_bow_vocab* voc, int levelsup = 4);
  // bool Tracking::TrackReferenceKeyFrame() (src/Tracking.cc:773-817) as one device sequence (lld_frame_compute_bow + lld_frame_track_reference_keyframe):
  // mCurrentFrame.ComputeBoW() on the resident descriptors (mFeatVec is filled from the call's host result; `voc` belongs to this frame's
  // context), the gather from mpReferenceKF (mDescriptors, mvKeysUn[k].angle, GetMapPointMatches() with NULL / isBad as -1, mFeatVec), the stage,
  // then the write-back: mvpMapPoints, mvbOutlier, mTcw, and mbTrackInView / mnLastFrameSeen of the discarded.  Returns as :816.  Below 15 matches
  // (:785-786) the objects stay untouched and false is returned; when mCurrentFrame has a pose the device frame is set back to what the objects
  // hold, otherwise the caller does that (SetFrameState) before TrackLocalMap follows.
  bool TrackReferenceKeyFrame(const TrackingMembers& tr, Frame& mCurrentFrame, const Frame& mLastFrame, const KeyFrame* mpReferenceKF, lld_bow_vocab* voc,
                              int levelsup = 4, TrackTrace* trace = nullptr);
  // bool Tracking::Relocalization() (src/Tracking.cc:1837-1998) in one call (lld_frame_compute_bow + lld_frame_relocalize), vpCandidateKFs being what
  // DetectRelocalizationCandidates returned (:1844): ComputeBoW as above, the gather of every candidate (as for TrackReferenceKeyFrame, plus each
  // MapPoint's distance band and descriptor and pKF->isBad()), the call, and on success the write-back of mTcw, mvpMapPoints and mvbOutlier.  Returns
  // bMatch; on false the objects stay untouched (a frame nobody reads, include/lld_amd.h).  The caller sets mnLastRelocFrameId (:1994).
  // seeds: one per candidate for its PnPsolver's rand() stream (default: its index; another length throws).  TrackLocalMap may follow on this object without SetFrameState.
  bool Relocalization(const TrackingMembers& tr, Frame& mCurrentFrame, const std::vector<KeyFrame*>& vpCandidateKFs, lld_bow_vocab* voc, int levelsup = 4,
                      const std::vector<uint32_t>* seeds = nullptr, RelocTrace* trace = nullptr);
  // The frame's pose and matches came from another routine (Tracking::TrackReferenceKeyFrame, src/Tracking.cc:770-816, or Relocalization): hands the
  // device what mCurrentFrame holds now (mTcw, mvpMapPoints / mvbOutlier, mvpMapLines / mvbOutlierLines) so that TrackLocalMap can follow.
  void SetFrameState(const TrackingMembers& tr, const Frame& mCurrentFrame);
  // bool Tracking::TrackLocalMap() from SearchLocalPoints() on; local_line_descs[i]: the descriptor AddLinesFrom compares local_lines[i] with.
  // Returns mnMatchesInliers through the pointer; the two final tests of the reference (:1212-1219) stay with the caller.
  void TrackLocalMap(const TrackingMembers& tr, Frame& mCurrentFrame, const std::vector<MapPoint*>& mvpLocalMapPoints, const std::vector<MapLine*>& local_lines,
                     const std::vector<lld_slam::Mat>& local_line_descs, int* mnMatchesInliers, TrackTrace* trace = nullptr);
  // bool Tracking::TrackLocalMap() WITH its UpdateLocalMap() (src/Tracking.cc:1126-1220, :1667-1835) on a map that is resident on the device
  // (MapOnDevice, lld_map_adapter.h): lld_frame_track_update_local_map + lld_frame_track_local_map_resident + one download.  Nothing is gathered:
  // the vote, the local keyframes, points and lines and stage 2's inputs are read from the map's tables.  Written back, as the host routine and
  // the TrackLocalMap above leave them: lm.mvpLocalKeyFrames / mvpLocalMapPoints / local_lines / local_line_descs / mpReferenceKF (kept when no
  // keyframe qualified), mCurrentFrame.mpReferenceKF, the mnTrackReferenceForFrame marks, a bad MapPoint taken out of mvpMapPoints (:1743), and
  // everything the TrackLocalMap above writes.  `map` must hold what the objects hold now (MapOnDevice::Update*).  A local map beyond the
  // map's limits (lld_local_map_result.status) throws, the objects untouched but for the bad MapPoints taken out; rec: the call's record, optional.
  void TrackLocalMap(const TrackingMembers& tr, Frame& mCurrentFrame, MapOnDevice& map, LocalMapMembers& lm, int* mnMatchesInliers, TrackTrace* trace = nullptr,
                     lld_local_map_result* rec = nullptr);
  // int Tracking::MatchLinesLastKF(bool do_skip_addnew, KeyFrame* pKF) (src/Tracking.cc:1449-1611) with mLastFrame on the device too (lld_frame_new_map_lines):
  // no gather - lines, partners, descriptors, poses, what the frames hold and what this frame tracked are read where the chain left them - then the
  // object bookkeeping of :1597-1604 from the call's result, as lld_line_adapter's MatchLinesLastKF does it from host arrays.  New MapLines take
  // their mnId from MapLine::nNextId in creation order; the device gave the same ids (a mismatch throws).  "Tracked by this frame" (:1518) is what
  // the device recorded: the lines its stages assigned, or the held lines after SetFrameState.  Returns mapline_cnt + cnt0.
  int MatchLinesLastKF(const TrackingMembers& tr, Frame& mCurrentFrame, FrameOnDevice& lastOnDevice, KeyFrame* pKF, lld_slam::Map* mpMap,
                       std::vector<MapLine*>* created = nullptr, std::vector<int>* match_trace = nullptr);
  // The tail of Tracking::Track after a successful TrackLocalMap on this object (src/Tracking.cc:446-476) as ONE device call (lld_frame_track_finish),
  // split where the reference's caller acts in between:
  //   NeedNewKeyFrame    the cleaning of VO matches on the objects (:446-453), then the call: counts, decision, the new stereo points and the outlier
  //                      drop happen on the device, on the state TrackLocalMap left there.  Returns NeedNewKeyFrame()'s value; *interruptBA: the
  //                      caller calls mpLocalMapper->InterruptBA() (:1296).  KeyFrameMade(): need && d.setNotStopOk.
  //   CreateNewKeyFrame  when KeyFrameMade(): pKF = new KeyFrame(mCurrentFrame, ..) is the caller's (:1375); the loop of :1399-1429 from the call's
  //                      result - `new MapPoint(x3D, pKF, mpMap)` per created entry in visiting order, so that mnId is the id the device gave (a mismatch
  //                      throws), AddObservation, pKF->AddMapPoint, mpMap->AddMapPoint, mvpMapPoints (ComputeDistinctiveDescriptors / UpdateNormalAndDepth
  //                      of the new points: the caller's, as lld_landmark_adapter's RefreshMapPoints) - then MatchLinesLastKF (:1433) when lastOnDevice.
  //   DropOutliers       :472-476 on the objects (the device has dropped them already).
  bool NeedNewKeyFrame(const TrackingMembers& tr, const KeyFrameDecision& d, Frame& mCurrentFrame, bool* interruptBA, FinishTrace* trace = nullptr);
  bool KeyFrameMade() const { return finish_made_; }
  void CreateNewKeyFrame(const TrackingMembers& tr, Frame& mCurrentFrame, KeyFrame* pKF, lld_slam::Map* mpMap, FrameOnDevice* lastOnDevice,
                         std::vector<MapPoint*>* created = nullptr);
  void DropOutliers(Frame& mCurrentFrame) const;
  // void Tracking::UpdateLastFrame() from :830 on, on the object that was the current frame of the last Track() (lld_frame_create_stereo_points,
  // LLD_POINTS_LAST_FRAME): mLastFrame.SetPose(Tlr*pRef->GetPose()) is the caller's (:825) and travels with the call; the temporal MapPoints are
  // news'd here in visiting order (MapPoint(x3D, mpMap, &mLastFrame, i) has no double: the three-argument constructor with a NULL keyframe stands
  // in), entered into mLastFrame.mvpMapPoints and appended to mlpTemporalPoints.
  void UpdateLastFrame(const TrackingMembers& tr, float mThDepth, Frame& mLastFrame, lld_slam::Map* mpMap, std::vector<MapPoint*>* mlpTemporalPoints);

 private:
  void create(const Frame& F);
  FinishTrace finish_;               // the result NeedNewKeyFrame fetched, for CreateNewKeyFrame
  bool finish_made_ = false;       // lld_frame_create of the keypoint side, the stage parameters
  lld_ctx* ctx_;
  lld_frame* f_ = nullptr;
  int nt_ = 0, nl_ = 0, dim_ = 1;
  lld_track_params params_;
};

}  // namespace lld_adapter
#endif
