// lld_slam_objects.h — a minimal object model for COMPILING and RUNNING the host adapters (adapters/lld_optimizer_adapter.cc,
// adapters/lld_matcher_adapter.cc) without the reference's dependencies.
//
// These are this repository's own test doubles, not reference headers: each class carries only the members the adapter touches,
// under the names the reference uses (include/KeyFrame.h, MapPoint.h, MapLine.h, Frame.h, Map.h), so that the adapter source reads
// like a patch of src/Optimizer.cc and compiles unchanged against the real classes once OpenCV / Eigen are present
// (build with -DLLD_ADAPTER_OBJECTS_HEADER='"your_header.h"').  `Mat` stands in for the CV_32F cv::Mat the reference stores poses and
// points in (same accessors: ptr<float>(), at<float>(i), at<float>(r, c), clone()), `Vector3d` for Eigen::Vector3d (operator()(i)).
//
// What is deliberately kept from the reference's data model, because the adapter's correctness depends on it:
//   * observations are std::map<KeyFrame*, size_t>: iteration is in POINTER order (SURVEY hazard 13);
//   * poses and points are float32, lines are double (Converter.cc defines the f32 <-> f64 boundary);
//   * KeyFrame::mnBALocalForKF / mnBAFixedForKF and MapPoint / MapLine::mnBALocalForKF are the visit marks of Optimizer.cc:938-1018.
#ifndef LLD_SLAM_OBJECTS_H
#define LLD_SLAM_OBJECTS_H

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

// ---- DBoW2::FeatureVector stand-in (Thirdparty/DBoW2/DBoW2/FeatureVector.h: a std::map<NodeId, std::vector<unsigned int>>)
namespace DBoW2 {
class FeatureVector : public std::map<unsigned int, std::vector<unsigned int> > {};
}

namespace lld_slam {

// ---- cv::Mat (CV_32F) stand-in: row-major floats with shared-nothing value semantics (the reference clones on every Get/Set)
class Mat {
 public:
  Mat() : rows(0), cols(0) {}
  Mat(int r, int c) : rows(r), cols(c), d_((size_t)r * c, 0.f) {}
  Mat(int r, int c, const float* src) : rows(r), cols(c), d_(src, src + (size_t)r * c) {}
  int rows, cols;
  bool empty() const { return d_.empty(); }
  Mat clone() const { return *this; }
  template <class T> T* ptr(int r = 0) { return reinterpret_cast<T*>(d_.data()) + (size_t)r * cols; }
  template <class T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(d_.data()) + (size_t)r * cols; }
  template <class T> T& at(int i) { return d_[(size_t)i]; }
  template <class T> const T& at(int i) const { return d_[(size_t)i]; }
  template <class T> T& at(int r, int c) { return d_[(size_t)r * cols + c]; }
  template <class T> const T& at(int r, int c) const { return d_[(size_t)r * cols + c]; }
 private:
  std::vector<float> d_;
};

// ---- Eigen::Vector3d stand-in
struct Vector3d {
  double v[3];
  Vector3d() : v{0, 0, 0} {}
  Vector3d(double x, double y, double z) : v{x, y, z} {}
  double& operator()(int i) { return v[i]; }
  double operator()(int i) const { return v[i]; }
};

// ---- cv::Mat (CV_8U) stand-in for ORB descriptors: one 32-byte row per keypoint (Frame::mDescriptors, MapPoint::GetDescriptor)
class MatU8 {
 public:
  MatU8() : rows(0), cols(0) {}
  MatU8(int r, int c) : rows(r), cols(c), d_(((size_t)r * c + 3) / 4, 0u) {}
  int rows, cols;
  bool empty() const { return rows == 0; }
  MatU8 clone() const { return *this; }
  MatU8 row(int r) const { MatU8 m(1, cols); std::memcpy(m.d_.data(), ptr<unsigned char>(r), (size_t)cols); return m; }
  template <class T> T* ptr(int r = 0) { return reinterpret_cast<T*>(reinterpret_cast<unsigned char*>(d_.data()) + (size_t)r * cols); }
  template <class T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(reinterpret_cast<const unsigned char*>(d_.data()) + (size_t)r * cols); }
 private:
  std::vector<unsigned int> d_;                                    // 4-byte aligned like cv::Mat's rows of 32
};

// ---- g2o::Sim3 stand-in (Thirdparty/g2o/g2o/types/sim3.h): rotation quaternion (x, y, z, w), translation, scale.  The adapters only carry it
struct Sim3 {
  double q[4], t[3], s;
  Sim3() : q{0, 0, 0, 1}, t{0, 0, 0}, s(1.0) {}
};

struct Point2f { float x, y; };
struct Point3f { float x, y, z; Point3f() : x(0.f), y(0.f), z(0.f) {} Point3f(float a, float b, float c) : x(a), y(b), z(c) {} };   // cv::Point3f
struct KeyPoint { Point2f pt; int octave; float angle; KeyPoint() : pt{0.f, 0.f}, octave(0), angle(0.f) {} };   // cv::KeyPoint: pt, octave, angle
struct KeyLine {                                                   // cv::line_descriptor::KeyLine (LineMatching.h:27): end points and octave
  float startPointX, startPointY, endPointX, endPointY; int octave;
  KeyLine() : startPointX(0), startPointY(0), endPointX(0), endPointY(0), octave(0) {}
};

class MapPoint;
class MapLine;
class Map;

class KeyFrame {
 public:
  unsigned long mnId = 0;
  unsigned long mnBALocalForKF = 0, mnBAFixedForKF = 0;            // KeyFrame.h: visit marks of LocalBundleAdjustment
  unsigned long mnTrackReferenceForFrame = 0;                      // KeyFrame.h: the mark of Tracking::UpdateLocalKeyFrames (Tracking.cc:1773)
  unsigned long mnFuseTargetForKF = 0;                             // KeyFrame.h: the mark of LocalMapping::SearchInNeighbors (LocalMapping.cc:469)
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  Mat mK;                                                          // 3x3 CV_32F
  std::vector<KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;                                     // negative: monocular keypoint
  std::vector<float> mvInvLevelSigma2;
  std::vector<KeyLine> mvLinesLeft, mvLinesRight;
  std::vector<int> line_matches;                                   // index into mvLinesRight, -1: no stereo partner

  Mat GetPose() const { return Tcw.clone(); }
  void SetPose(const Mat& T) { Tcw = T.clone(); n_set_pose++; }
  bool isBad() const { return mbBad; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() const { return mvpOrderedConnectedKeyFrames; }
  std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
  std::vector<MapLine*> GetMapLineMatches() const { return mvpMapLines; }
  void EraseMapPointMatch(MapPoint* p) { for (auto& q : mvpMapPoints) if (q == p) q = nullptr; }
  void EraseMapPointMatch(const size_t& idx) { mvpMapPoints[idx] = nullptr; }
  void EraseMapLineMatch(MapLine* l) { for (auto& q : mvpMapLines) if (q == l) q = nullptr; }
  void AddMapLine(MapLine* pML, const size_t& idx) { if (mvpMapLines.size() <= idx) mvpMapLines.resize(idx + 1, nullptr); mvpMapLines[idx] = pML; }   // KeyFrame.cc
  // what the matchers read (include/KeyFrame.h): keypoint descriptors, the image bounds and grid constants, the scale pyramid, the
  // pose pieces; and what ORBmatcher::Fuse writes
  MatU8 mDescriptors;
  Mat mDescriptorsLines;                                           // one LBD descriptor (CV_32F row) per left line (KeyFrame.h)
  DBoW2::FeatureVector mFeatVec;                                   // vocabulary node -> keypoint indices (KeyFrame::ComputeBoW)
  int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;               // KeyFrame.h:196-199 (const int there)
  float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
  int mnScaleLevels = 0;
  float mfScaleFactor = 0, mfLogScaleFactor = 0;
  std::vector<float> mvScaleFactors, mvLevelSigma2;
  Mat GetRotation() const { Mat R(3, 3); for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R.at<float>(r, c) = Tcw.at<float>(r, c); return R; }
  Mat GetTranslation() const { Mat t(3, 1); for (int r = 0; r < 3; r++) t.at<float>(r) = Tcw.at<float>(r, 3); return t; }
  Mat GetCameraCenter() const { return Ow.clone(); }
  bool IsInImage(const float& x, const float& y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }   // KeyFrame.cc:633-636
  void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }
  MapPoint* GetMapPoint(const size_t& idx) const { return mvpMapPoints[idx]; }
  std::set<MapPoint*> GetMapPoints() const { std::set<MapPoint*> s; for (size_t i = 0; i < mvpMapPoints.size(); i++) if (mvpMapPoints[i]) s.insert(mvpMapPoints[i]); return s; }   // KeyFrame.cc:277-291 (bad points are filtered there; the doubles of the tests hold none)
  void ReplaceMapPointMatch(const size_t& idx, MapPoint* pMP) { mvpMapPoints[idx] = pMP; }
  Mat Ow;                                                          // 3x1, set with the pose by the reference (KeyFrame::SetPose)
  // what LocalMapping::CreateNewMapPoints reads on top (include/KeyFrame.h)
  int N = 0;                                                       // number of keypoints
  float mb = 0, invfx = 0, invfy = 0;
  std::vector<KeyPoint> mvKeys;                                    // the raw keypoints UnprojectStereo reads (KeyFrame.cc:643)
  std::vector<float> mvDepth;                                      // negative: no depth
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& n) const {   // KeyFrame.cc:182-190
    if ((int)mvpOrderedConnectedKeyFrames.size() < n) return mvpOrderedConnectedKeyFrames;
    return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + n);
  }
  // KeyFrame.cc:638-654: Twc.rowRange(0,3).colRange(0,3)*x3Dc+Twc.rowRange(0,3).col(3) = Rwc*x3Dc (one gemm, double accumulation) + Ow
  Mat UnprojectStereo(int i) const {
    const float z = mvDepth[i];
    if (!(z > 0)) return Mat();
    const float u = mvKeys[i].pt.x, v = mvKeys[i].pt.y;
    const float c[3] = {(u - cx) * z * invfx, (v - cy) * z * invfy, z};
    Mat x3D(3, 1);
    for (int r = 0; r < 3; r++) {
      double acc = (double)Tcw.at<float>(0, r) * (double)c[0];
      acc += (double)Tcw.at<float>(1, r) * (double)c[1];
      acc += (double)Tcw.at<float>(2, r) * (double)c[2];
      x3D.at<float>(r) = (float)acc + Ow.at<float>(r);
    }
    return x3D;
  }
  inline float ComputeSceneMedianDepth(const int q) const;          // KeyFrame.cc:656-686, defined below MapPoint

  // what KeyFrame::UpdateConnections and LocalMapping::KeyFrameCulling read and write on top (include/KeyFrame.h)
  float mThDepth = 0;
  std::map<KeyFrame*, int> mConnectedKeyFrameWeights;              // pointer-ordered, as in the reference
  std::vector<int> mvOrderedWeights;
  bool mbFirstConnection = true;
  KeyFrame* mpParent = nullptr;
  std::set<KeyFrame*> mspChildrens;
  void AddChild(KeyFrame* pKF) { mspChildrens.insert(pKF); }
  void UpdateBestCovisibles() {                                     // KeyFrame.cc:146-165: sort of (weight, pointer), then push_front
    std::vector<std::pair<int, KeyFrame*> > vPairs;
    vPairs.reserve(mConnectedKeyFrameWeights.size());
    for (std::map<KeyFrame*, int>::iterator mit = mConnectedKeyFrameWeights.begin(), mend = mConnectedKeyFrameWeights.end(); mit != mend; mit++)
      vPairs.push_back(std::make_pair(mit->second, mit->first));
    std::sort(vPairs.begin(), vPairs.end());
    mvpOrderedConnectedKeyFrames.clear(); mvOrderedWeights.clear();
    for (size_t i = vPairs.size(); i-- > 0;) { mvpOrderedConnectedKeyFrames.push_back(vPairs[i].second); mvOrderedWeights.push_back(vPairs[i].first); }
  }
  void AddConnection(KeyFrame* pKF, const int& weight) {           // KeyFrame.cc:131-144
    std::map<KeyFrame*, int>::iterator it = mConnectedKeyFrameWeights.find(pKF);
    if (it != mConnectedKeyFrameWeights.end() && it->second == weight) return;
    mConnectedKeyFrameWeights[pKF] = weight;
    UpdateBestCovisibles();
  }
  void EraseConnection(KeyFrame* pKF) {                             // KeyFrame.cc: erase, then re-sort
    if (mConnectedKeyFrameWeights.erase(pKF)) UpdateBestCovisibles();
  }
  inline void SetBadFlag();                                         // KeyFrame.cc:476-: defined below MapPoint

  // what LoopClosing::RunGlobalBundleAdjustment reads and writes on top (include/KeyFrame.h:145-148, :90-92)
  Mat mTcwGBA, mTcwBefGBA;
  unsigned long mnBAGlobalForKF = 0;
  std::set<KeyFrame*> GetChilds() const { return mspChildrens; }
  KeyFrame* GetParent() const { return mpParent; }

  // (test access)
  Mat Tcw;
  bool mbBad = false;
  int n_set_pose = 0;
  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
  std::vector<MapPoint*> mvpMapPoints;                             // per keypoint, nullptr = none
  std::vector<MapLine*> mvpMapLines;                               // per left line
};

class MapPoint {
 public:
  MapPoint() {}
  // MapPoint(const cv::Mat &Pos, KeyFrame *pRefKF, Map* pMap)   (MapPoint.cc:32-44)
  MapPoint(const Mat& Pos, KeyFrame* pRefKF, Map* pMap) { mNormalVector = Mat(3, 1); mWorldPos = Pos.clone(); mpRefKF = pRefKF; mpMap = pMap; mnId = nNextId()++; }
  static unsigned long& nNextId() { static unsigned long n = 0; return n; }
  Map* mpMap = nullptr;
  unsigned long mnId = 0;
  unsigned long mnBALocalForKF = 0;
  static std::mutex mGlobalMutex;
  Mat GetWorldPos() const { return mWorldPos.clone(); }
  void SetWorldPos(const Mat& p) { mWorldPos = p.clone(); n_set_pos++; }
  std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
  void EraseObservation(KeyFrame* kf) { mObservations.erase(kf); }
  bool isBad() const { return mbBad; }
  void UpdateNormalAndDepth() { n_update_normal++; }
  // what the matchers read and write (include/MapPoint.h)
  Mat GetNormal() const { return mNormalVector.clone(); }
  MatU8 GetDescriptor() const { return mDescriptor.clone(); }
  float GetMinDistanceInvariance() const { return 0.8f * mfMinDistance; }
  float GetMaxDistanceInvariance() const { return 1.2f * mfMaxDistance; }
  int Observations() const { return nObs; }
  bool IsInKeyFrame(KeyFrame* pKF) const { return mObservations.count(pKF) != 0; }
  int GetIndexInKeyFrame(KeyFrame* pKF) const { std::map<KeyFrame*, size_t>::const_iterator it = mObservations.find(pKF); return it == mObservations.end() ? -1 : (int)it->second; }
  void IncreaseVisible(int n = 1) { mnVisible += n; }
  void IncreaseFound(int n = 1) { mnFound += n; }
  void AddObservation(KeyFrame* pKF, size_t idx) {                  // MapPoint.cc:67-78
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    if (pKF->mvuRight[idx] >= 0) nObs += 2; else nObs++;
  }
  void Replace(MapPoint* pMP) {                                     // MapPoint.cc:176-220 (without the map / descriptor upkeep)
    if (pMP->mnId == this->mnId) return;
    const std::map<KeyFrame*, size_t> obs = mObservations;
    mObservations.clear(); mbBad = true; mpReplaced = pMP;
    for (std::map<KeyFrame*, size_t>::const_iterator mit = obs.begin(); mit != obs.end(); ++mit) {
      KeyFrame* pKF = mit->first;
      if (!pMP->IsInKeyFrame(pKF)) { pKF->ReplaceMapPointMatch(mit->second, pMP); pMP->AddObservation(pKF, mit->second); }
      else pKF->EraseMapPointMatch(mit->second);
    }
    pMP->IncreaseFound(mnFound); pMP->IncreaseVisible(mnVisible);
  }
  Mat mNormalVector;                                               // 3x1 CV_32F
  MatU8 mDescriptor;                                               // 1x32
  float mfMinDistance = 0, mfMaxDistance = 0;                      // protected in the reference: the patch adds the two getters below
  float GetMinDistance() const { return mfMinDistance; }
  float GetMaxDistance() const { return mfMaxDistance; }
  int nObs = 0, mnVisible = 1, mnFound = 1;
  MapPoint* mpReplaced = nullptr;
  // variables used by the tracking (MapPoint.h:88-96)
  float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0, mTrackViewCos = 0;
  bool mbTrackInView = false;
  int mnTrackScaleLevel = 0;
  unsigned long mnLastFrameSeen = 0;
  unsigned long mnTrackReferenceForFrame = 0;                      // the mark of Tracking::UpdateLocalPoints (Tracking.cc:1700)
  unsigned long mnFuseCandidateForKF = 0;                          // MapPoint.h: the mark of LocalMapping::SearchInNeighbors (LocalMapping.cc:510)

  // variables used by loop closing (MapPoint.h:103-107)
  unsigned long mnCorrectedByKF = 0, mnCorrectedReference = 0;
  Mat mPosGBA;
  unsigned long mnBAGlobalForKF = 0;
  KeyFrame* GetReferenceKeyFrame() const { return mpRefKF; }

  Mat mWorldPos;                                                   // 3x1 CV_32F
  KeyFrame* mpRefKF = nullptr;                                     // MapPoint.h: the reference keyframe UpdateNormalAndDepth reads
  std::map<KeyFrame*, size_t> mObservations;                       // pointer-ordered, as in the reference
  bool mbBad = false;
  int n_set_pos = 0, n_update_normal = 0;
};

// KeyFrame.cc:656-686.  The reference indexes an empty vector when the keyframe holds no MapPoint; here that yields 0.
inline float KeyFrame::ComputeSceneMedianDepth(const int q) const {
  std::vector<float> vDepths;
  vDepths.reserve(mvpMapPoints.size());
  const float zcw = Tcw.at<float>(2, 3);
  for (size_t i = 0; i < mvpMapPoints.size(); i++) {
    if (!mvpMapPoints[i]) continue;
    const Mat x3Dw = mvpMapPoints[i]->GetWorldPos();
    double acc = (double)Tcw.at<float>(2, 0) * (double)x3Dw.at<float>(0);    // Rcw2.dot(x3Dw): the double sum
    acc += (double)Tcw.at<float>(2, 1) * (double)x3Dw.at<float>(1);
    acc += (double)Tcw.at<float>(2, 2) * (double)x3Dw.at<float>(2);
    vDepths.push_back((float)(acc + (double)zcw));
  }
  if (vDepths.empty()) return 0.f;
  std::sort(vDepths.begin(), vDepths.end());
  return vDepths[(vDepths.size() - 1) / q];
}

// KeyFrame.cc:476-565 without the spanning-tree repair: the connections are erased on both sides and the keyframe's observations
// are erased from its map points as MapPoint::EraseObservation does it (nObs drops by 2 for a stereo keypoint, by 1 otherwise; a
// point left with nObs <= 2 becomes bad).  That is what changes the counts of the keyframes KeyFrameCulling visits afterwards.
inline void KeyFrame::SetBadFlag() {
  if (mnId == 0) return;
  for (std::map<KeyFrame*, int>::iterator mit = mConnectedKeyFrameWeights.begin(), mend = mConnectedKeyFrameWeights.end(); mit != mend; mit++)
    mit->first->EraseConnection(this);
  for (size_t i = 0; i < mvpMapPoints.size(); i++) {
    MapPoint* pMP = mvpMapPoints[i];
    if (!pMP) continue;
    const int idx = pMP->GetIndexInKeyFrame(this);
    if (idx < 0) continue;
    pMP->nObs -= ((size_t)idx < mvuRight.size() && mvuRight[idx] >= 0) ? 2 : 1;
    pMP->EraseObservation(this);
    if (pMP->nObs <= 2) pMP->mbBad = true;
  }
  mConnectedKeyFrameWeights.clear();
  mvpOrderedConnectedKeyFrames.clear();
  mbBad = true;
}

class MapLine {
 public:
  MapLine() {}
  // MapLine(const Eigen::Vector3d& X0, const Eigen::Vector3d& line_dir, KeyFrame* pRefKF, Map* pMap, int idx)   (include/MapLine.h; Tracking.cc:1598)
  MapLine(const Vector3d& X0, const Vector3d& line_dir, KeyFrame* pRefKF, Map* pMap, int idx) : mpRefKF(pRefKF), mpMap(pMap), ref_idx(idx), mX0(X0), mDir(line_dir) { mnId = nNextId()++; }
  static unsigned long& nNextId() { static unsigned long n = 0; return n; }
  void AddObservation(KeyFrame* pKF, size_t idx) { mObservations[pKF] = idx; }
  void ComputeDistinctiveDescriptors() { n_distinctive++; }
  KeyFrame* mpRefKF = nullptr; Map* mpMap = nullptr; int ref_idx = -1; int n_distinctive = 0;
  unsigned long mnId = 0;
  unsigned long mnBALocalForKF = 0;
  void GetMinimalPos(Vector3d* X0, Vector3d* dir) const { *X0 = mX0; *dir = mDir; }
  void GetMainPoints3D(Vector3d* X1, Vector3d* X2) const { *X1 = mX1; *X2 = mX2; }   // the 3D end points the depth test of Tracking::AddLinesFrom maps (:1064-1072)
  Vector3d mX1, mX2;
  long mnTrackReferenceForFrame = -1;                              // MapLine.h: the mark of Tracking::UpdateLocalPoints (Tracking.cc:1720)
  void GetDescriptor(Mat* d) const { *d = mDescriptor.clone(); }   // MapLine.cc
  long tracked_last_id = -1;                                       // MapLine.h: the frame that last took this line (Tracking.cc:1019, :1118)
  void SetMinimalPos(const Vector3d& X0, const Vector3d& dir) { mX0 = X0; mDir = dir; n_set_pos++; }
  std::map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
  int Observations() const { return (int)mObservations.size(); }
  void EraseObservation(KeyFrame* kf) { mObservations.erase(kf); }
  bool isBad() const { return mbBad; }

  Vector3d mX0, mDir;
  Mat mDescriptor;                                                 // 1 x dim CV_32F (MapLine.h), written by ComputeDistinctiveDescriptors
  std::map<KeyFrame*, size_t> mObservations;
  bool mbBad = false;
  int n_set_pos = 0;
};

class Frame {                                                      // what PoseOptimization reads and writes (include/Frame.h)
 public:
  int N = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0, mbf = 0;
  Mat mK, mTcw;
  std::vector<KeyPoint> mvKeysUn;
  std::vector<float> mvuRight;
  std::vector<float> mvInvLevelSigma2;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  std::vector<KeyLine> mvLinesLeft, mvLinesRight;
  std::vector<int> line_matches;
  std::vector<MapLine*> mvpMapLines;
  std::vector<bool> mvbOutlierLines;
  KeyFrame* mpReferenceKF = nullptr;                               // Frame.h: set with Tracking::mpReferenceKF (Tracking.cc:1833)
  Mat mDescriptorsLines;                                           // one LBD descriptor (CV_32F row) per left line
  Mat mDescriptorsLinesRight;                                      // ... per right line (Frame.h; read by the Frame constructor's MatchLines, src/Frame.cc:122)
  void SetPose(const Mat& T) { mTcw = T.clone(); n_set_pose++; UpdatePoseMatrices(); }
  int n_set_pose = 0;
  // what the matchers read (include/Frame.h).  The image bounds and grid constants are static members of the reference's Frame;
  // the adapter reaches them through an object (F.mnMinX), which compiles for both
  unsigned long mnId = 0;
  float mb = 0;
  std::vector<KeyPoint> mvKeys;
  std::vector<float> mvDepth;
  MatU8 mDescriptors;
  DBoW2::FeatureVector mFeatVec;
  float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0, mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
  int mnScaleLevels = 0;
  float mfScaleFactor = 0, mfLogScaleFactor = 0;
  std::vector<float> mvScaleFactors, mvLevelSigma2;
  Mat mRcw, mtcw, mOw;
  void UpdatePoseMatrices() {                                       // Frame.cc:325-331: mOw = -mRcw.t()*mtcw is one gemm (double accumulation)
    if (mTcw.empty()) return;
    mRcw = Mat(3, 3); mtcw = Mat(3, 1); mOw = Mat(3, 1);
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) mRcw.at<float>(r, c) = mTcw.at<float>(r, c); mtcw.at<float>(r) = mTcw.at<float>(r, 3); }
    for (int r = 0; r < 3; r++) {
      double acc = 0.0;
      for (int k = 0; k < 3; k++) acc += (double)mRcw.at<float>(k, r) * (double)mtcw.at<float>(k);
      mOw.at<float>(r) = (float)(-acc);
    }
  }
};

class Map {
 public:
  std::mutex mMutexMapUpdate;
  void AddMapLine(MapLine* pML) { mspMapLines.insert(pML); }       // Map.cc
  std::set<MapLine*> mspMapLines;
  void AddMapPoint(MapPoint* pMP) { mspMapPoints.insert(pMP); }    // Map.cc
  std::set<MapPoint*> mspMapPoints;
  // what the loop-closing thread reads on top (include/Map.h)
  void AddKeyFrame(KeyFrame* pKF) { mspKeyFrames.insert(pKF); }
  std::set<KeyFrame*> mspKeyFrames;
  std::vector<KeyFrame*> GetAllKeyFrames() const { return std::vector<KeyFrame*>(mspKeyFrames.begin(), mspKeyFrames.end()); }
  std::vector<MapLine*> GetAllMapLines() const { return std::vector<MapLine*>(mspMapLines.begin(), mspMapLines.end()); }
  std::vector<MapPoint*> GetAllMapPoints() const { return std::vector<MapPoint*>(mspMapPoints.begin(), mspMapPoints.end()); }
  std::vector<KeyFrame*> mvpKeyFrameOrigins;
};

}  // namespace lld_slam
#endif
