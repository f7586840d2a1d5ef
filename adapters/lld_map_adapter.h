// lld_map_adapter.h — host adapter that keeps a live Map of SLAM objects mirrored in an lld_map (include/lld_amd.h, "the resident map"), so that
// Tracking::UpdateLocalMap (src/Tracking.cc:1667-1835) and TrackLocalMap run on the device between the tracking stages
// (FrameOnDevice::TrackLocalMap(.., MapOnDevice&, ..) in lld_tracking_adapter.h).
//   Upload(Map*)        after Map::clear() or at start-up: every keyframe, MapPoint and MapLine of the map.
//   UpdatePoints(..)    what LocalMapping, a BA or a loop correction changed about MapPoints: position, normal, distances, descriptor, bad flag,
//                       observations (the whole row of each listed point travels).
//   UpdateKeyFrames(..) a new keyframe, or one whose matches, best covisibles, children, parent or bad flag changed (all four lists travel).
//   UpdateLines(..)     MapLines likewise.
// Slots: the slot of a KeyFrame, MapPoint or MapLine is its mnId - the ids lld_tracking_adapter already names MapPoints and MapLines by on the
// device, so every stage-1 routine of FrameOnDevice is followed unchanged.  order_key of a keyframe is its pointer value: the device visits
// the voted keyframes and the children in the order std::map<KeyFrame*,int> / std::set<KeyFrame*> iterate.  An object that is referenced by a
// row but was never sent stays "never set" on the device: a temporal MapPoint votes for nothing, a keyframe or line counts as bad.
// The caller holds Map::mMutexMapUpdate as the reference does around the same changes.  One context, one host thread.
#ifndef LLD_MAP_ADAPTER_H
#define LLD_MAP_ADAPTER_H

#include <vector>

#include "../include/lld_amd.h"
#include "lld_optimizer_adapter.h"      // LbaTrace (and the object model: LLD_ADAPTER_OBJECTS_HEADER)

namespace lld_adapter {

class MapOnDevice {
 public:
  MapOnDevice(lld_ctx* ctx, const lld_map_limits& limits);
  ~MapOnDevice();
  MapOnDevice(const MapOnDevice&) = delete;
  MapOnDevice& operator=(const MapOnDevice&) = delete;

  void Upload(lld_slam::Map* pMap);
  void UpdatePoints(const std::vector<lld_slam::MapPoint*>& points);
  void UpdateKeyFrames(const std::vector<lld_slam::KeyFrame*>& keyframes);
  void UpdateLines(const std::vector<lld_slam::MapLine*>& lines);

  // ---- covisibility on the mirrored map (lld_map_covisibility): no gather, no upload of the map
  // From here on Upload / UpdatePoints / UpdateKeyFrames also send what KeyFrameCulling reads: the keypoint index of every observation and
  // MapPoint::Observations() with the points, mvKeysUn[i].octave / mvDepth[i] / mThDepth with the keyframes.  Call it before the first Upload
  // (rows sent earlier carry none of it and KeyFrameCulling then throws).  Without it the three calls behave exactly as before.
  void EnableCovisibility() { covis_ = true; }
  // pKF->UpdateConnections() for every keyframe of the list, in list order, with one device call on the resident tables: what
  // lld_adapter::UpdateConnections (lld_covisibility_adapter.h) applies - members, AddConnection on the neighbours, first-connection parent and
  // AddChild - and then the map is brought up to date: the device wrote the queries' own cov rows, the neighbours' go through
  // lld_map_set_covisibles, a keyframe with a new parent or child through UpdateKeyFrames.  The listed keyframes and their MapPoints must be
  // current in the map.  Returns the number of keyframes the rule wrote.  A keyframe with more than LLD_MAP_COVIS_MAX_CONNECTED covisible
  // keyframes gets nothing written, neither its members nor its cov row in the map; all the others are applied and pushed first, so objects
  // and map agree.  Then such keyframes are returned in `overflowed` for the caller's pKF->UpdateConnections() + UpdateKeyFrames, or, when
  // `overflowed` is NULL, the call throws.
  int UpdateConnections(const std::vector<lld_slam::KeyFrame*>& vpKFs, std::vector<lld_slam::KeyFrame*>* overflowed = nullptr);
  // LocalMapping::KeyFrameCulling for pCurrentKF, walked as lld_adapter::KeyFrameCulling walks it: one device call for the keyframes that
  // remain, SetBadFlag on the first redundant one, then what that changed is pushed and the rest is counted again: its MapPoints' rows, its
  // own row, its former neighbours' cov rows, and for the spanning-tree repair of KeyFrame::SetBadFlag (KeyFrame.cc:505-560) the whole rows of
  // its former parent, of its children and of the parents they have afterwards.  Returns the flagged keyframes in order.
  std::vector<lld_slam::KeyFrame*> KeyFrameCulling(lld_slam::KeyFrame* pCurrentKF, bool bMonocular, int* n_calls = nullptr);

  // ---- local bundle adjustment on the mirrored map (lld_map_local_ba): the window is assembled on the device's tables
  // From here on Upload / UpdateKeyFrames / UpdateLines also send what the window reads beyond the covisibility tables (which this enables
  // too): mnId, pose, mvKeysUn[i].pt / mvuRight[i] and the keylines with their stereo partners per keyframe, the observation rows and
  // Observations() per MapLine.  Call it before the first Upload (LocalBundleAdjustment throws on a map whose rows carry none of it).
  void EnableBundleAdjustment() { covis_ = true; ba_ = true; }
  // Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap, gamma) as lld_adapter::LocalBundleAdjustment (lld_optimizer_adapter.h) makes it,
  // with the window of src/Optimizer.cc:938-1218 assembled by the device instead of walked on the objects: one call, then the same erase
  // lists and write-back under the map mutex, then the rows that changed are pushed - the local keyframes' poses (lld_map_set_keyframe_poses),
  // the local points and lines (UpdatePoints / UpdateLines: positions and the rows an erased observation shortened) and the keyframes that
  // lost a match (UpdateKeyFrames).  pKF, its covisible keyframes and everything they see must be current in the map.  The visit marks
  // (mnBALocalForKF / mnBAFixedForKF) are set on the objects as the reference sets them.  mvInvLevelSigma2 is read from pKF: one table for
  // all keyframes, as ORBextractor makes it.  The trace's window and output are filled only when a trace is asked for.
  void LocalBundleAdjustment(lld_slam::KeyFrame* pKF, bool* pbStopFlag, lld_slam::Map* pMap, double gamma = 1.0, LbaTrace* trace = nullptr);

  // ---- the per-landmark refresh on the mirrored map (lld_map_refresh_points / _lines): no gather, nothing pushed back
  // From here on Upload / UpdateKeyFrames also send mDescriptors and mDescriptorsLines (one row per entry of the point and line rows) and
  // Upload / UpdatePoints the points' mpRefKF.  It implies the covisibility and bundle-adjustment tables: the normal part reads the camera
  // centres, the octaves and the index rows.  Call it before the first Upload.
  void EnableRefresh() { covis_ = true; ba_ = true; refresh_ = true; }
  // MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth for the listed points (flags: LLD_LANDMARK_DESCRIPTOR, LLD_LANDMARK_NORMAL_DEPTH
  // or both) as lld_adapter::RefreshMapPoints (lld_landmark_adapter.h) makes them, in ONE device call on the resident tables, then
  // mDescriptor / mNormalVector / mfMinDistance / mfMaxDistance of exactly the objects the call updated are written.  The map already holds
  // the result.  The points, their observers and their reference keyframes must be current in the map; NULL entries are skipped, a point
  // may be listed once.  mvScaleFactors is read from the first listed point's mpRefKF: one table for all keyframes.  Returns the number of
  // points written, as lld_adapter::RefreshMapPoints does.  A point the device flags (LLD_MAP_REFRESH_*: no mpRefKF, or the map lacks a
  // row it needs) is left alone, as lld_adapter::RefreshMapPoints leaves a point without mpRefKF alone.
  int RefreshMapPoints(const std::vector<lld_slam::MapPoint*>& vpMapPoints, unsigned flags);
  // MapLine::ComputeDistinctiveDescriptors for the listed lines, likewise; returns the number of lines written.
  int ComputeDistinctiveDescriptors(const std::vector<lld_slam::MapLine*>& vpMapLines);

  // ---- ORBmatcher::Fuse and LocalMapping::SearchInNeighbors on the mirrored map (lld_map_fuse): no gather, nothing pushed back
  // (EnableRefresh before the first Upload: the search reads the keyframes' keypoints, octaves and descriptors.)
  // int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, const float th) as lld_adapter::ORBmatcher::Fuse
  // (lld_matcher_adapter.h) makes it, in ONE device call: the search on the map's rows, the add / Replace bookkeeping on the map's rows, the
  // survivors' descriptors.  The objects then follow from the call's action / other, in list order: AddObservation + AddMapPoint, or
  // MapPoint::Replace in the direction the call took (mnFound / mnVisible travel inside Replace), and the survivors' mDescriptor is read
  // back from the map.  pKF, the listed points and the points pKF holds must be current in the map; a NULL entry is a NULL entry.  With
  // pSourceKF the candidates are that keyframe's point row as the MAP holds it - vpMapPoints must be its GetMapPointMatches() - and no
  // list travels.  Returns nFused.
  int Fuse(lld_slam::KeyFrame* pKF, const std::vector<lld_slam::MapPoint*>& vpMapPoints, float th = 3.0f, lld_slam::KeyFrame* pSourceKF = nullptr);
  // LocalMapping::SearchInNeighbors (src/LocalMapping.cc:455-535, nn = 10) for pKF: the target list with the mnFuseTargetForKF marks, one
  // Fuse per target with pKF's matches (the first as pKF's row in the map, the later ones as the list copied before the first, as the
  // reference holds it: a Replace may have changed the row meanwhile), the candidate list with the mnFuseCandidateForKF marks, one Fuse into
  // pKF, then RefreshMapPoints over pKF's matches and UpdateConnections({pKF}).  Returns the sum of the Fuse calls' return values.
  int SearchInNeighbors(lld_slam::KeyFrame* pKF);

  // slot -> object (NULL: never sent)
  lld_slam::KeyFrame* KeyFrameOf(int slot) const { return slot >= 0 && slot < (int)kf_.size() ? kf_[slot] : nullptr; }
  lld_slam::MapPoint* PointOf(int slot) const { return slot >= 0 && slot < (int)pt_.size() ? pt_[slot] : nullptr; }
  lld_slam::MapLine* LineOf(int slot) const { return slot >= 0 && slot < (int)ln_.size() ? ln_[slot] : nullptr; }
  const lld_map_limits& limits() const { return limits_; }
  lld_map* get() const { return m_; }

 private:
  lld_map* m_ = nullptr;
  lld_map_limits limits_;
  std::vector<lld_slam::KeyFrame*> kf_;
  std::vector<lld_slam::MapPoint*> pt_;
  std::vector<lld_slam::MapLine*> ln_;
  bool covis_ = false, ba_ = false, refresh_ = false;
  void SetCovisibles(const std::vector<lld_slam::KeyFrame*>& keyframes);
};

}  // namespace lld_adapter
#endif
