// loop_correct_harness.cpp — the loop-closing thread's three map corrections on KeyFrame / MapPoint / Map test doubles, twice over:
//   the adapter    adapters/lld_loopclosing_adapter.cc: one device call each (lld_loop_correct, lld_essential_graph_apply, lld_global_ba_apply)
//   the host route the loops of src/LoopClosing.cc:440-518, src/Optimizer.cc:1601-1653 and src/LoopClosing.cc:678-739 in compiled C++ on
//                  the same doubles, with UpdateNormalAndDepth through lld_adapter::RefreshMapPoints: one call per connected keyframe in
//                  CorrectLoop, one call after the loop for the essential graph.
// usage: loop_correct_harness scene.bin out.bin [reps [flat]]
// scene.bin is written by tests/loopcorr_scenes.py (object_scene_blob); out.bin holds every member either route wrote, adapter first.
// With reps > 0 the two routes alternate on fresh copies of the objects and one JSON line with the median wall times is printed.
// With `flat` after reps nothing is built from objects: the new call and the route before it alternate on the scene's flat arrays,
// timed with HIP events (time_flat below), and out.bin is not written.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <list>
#include <string>
#include <vector>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>               // the events of the flat-array timing; everything else here needs no HIP header

#include "../adapters/lld_landmark_adapter.h"
#include "../adapters/lld_loopclosing_adapter.h"

using lld_adapter::KeyFrameAndPose;
using lld_slam::KeyFrame;
using lld_slam::Map;
using lld_slam::MapPoint;
using lld_slam::Mat;
using lld_slam::Sim3;

namespace {

// ------------------------------------------------------------------ the scene file
struct Reader {
  std::vector<char> buf; size_t at = 0;
  explicit Reader(const char* path) { std::ifstream f(path, std::ios::binary); buf.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()); }
  template <class T> T get() { T v; if (at + sizeof(T) > buf.size()) { std::fprintf(stderr, "scene file too short\n"); std::exit(2); } std::memcpy(&v, &buf[at], sizeof(T)); at += sizeof(T); return v; }
  template <class T> std::vector<T> many(size_t n) { std::vector<T> v(n); for (size_t i = 0; i < n; i++) v[i] = get<T>(); return v; }
};

struct Scene {
  int kind = 0, n_kf = 0, n_levels = 0, n_points = 0;
  std::vector<float> level_scale, tcw, pos, normal, mn, mx;
  std::vector<int> bad, ref_kf, ref_level;
  std::vector<std::vector<int> > obs;
  // kind 1
  int cur = 0; std::vector<int> conn, already; double scw[8]; std::vector<std::vector<int> > lists;
  // kind 2
  std::vector<double> before, after; std::vector<int> corr_kf;
  // kind 3
  std::vector<int> kf_in_gba, parent, origins, pt_in_gba; std::vector<float> tcw_gba, pos_gba;
};

Scene read_scene(const char* path) {
  Reader R(path);
  Scene S;
  S.kind = R.get<int>(); S.n_kf = R.get<int>(); S.n_levels = R.get<int>(); S.n_points = R.get<int>();
  S.level_scale = R.many<float>(S.n_levels);
  S.tcw = R.many<float>((size_t)12 * S.n_kf);
  S.obs.resize(S.n_points);
  for (int p = 0; p < S.n_points; p++) {
    S.bad.push_back(R.get<int>());
    for (int q = 0; q < 3; q++) S.pos.push_back(R.get<float>());
    S.ref_kf.push_back(R.get<int>()); S.ref_level.push_back(R.get<int>());
    for (int q = 0; q < 3; q++) S.normal.push_back(R.get<float>());
    S.mn.push_back(R.get<float>()); S.mx.push_back(R.get<float>());
    S.obs[p] = R.many<int>(R.get<int>());
  }
  if (S.kind == 1) {
    const int n_conn = R.get<int>(); S.cur = R.get<int>();
    S.conn = R.many<int>(n_conn);
    for (int q = 0; q < 8; q++) S.scw[q] = R.get<double>();
    S.lists.resize(n_conn);
    for (int r = 0; r < n_conn; r++) S.lists[r] = R.many<int>(R.get<int>());
    S.already = R.many<int>(S.n_points);
  } else if (S.kind == 2) {
    S.before = R.many<double>((size_t)8 * S.n_kf); S.after = R.many<double>((size_t)8 * S.n_kf); S.corr_kf = R.many<int>(S.n_points);
  } else {
    for (int k = 0; k < S.n_kf; k++) {
      S.kf_in_gba.push_back(R.get<int>());
      for (int q = 0; q < 12; q++) S.tcw_gba.push_back(R.get<float>());
      S.parent.push_back(R.get<int>());
    }
    S.origins = R.many<int>(R.get<int>());
    for (int p = 0; p < S.n_points; p++) { S.pt_in_gba.push_back(R.get<int>()); for (int q = 0; q < 3; q++) S.pos_gba.push_back(R.get<float>()); }
  }
  return S;
}

// ------------------------------------------------------------------ float cv::Mat forms (the gemm rule: double sum in index order, one rounding)
Mat pose_mat(const float* rows) { Mat T(4, 4); for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) T.at<float>(r, c) = rows[4 * r + c]; T.at<float>(3, 3) = 1.f; return T; }
void centre_of(const Mat& T, float* ow) {                      // Ow = -Rwc*tcw (KeyFrame.cc:84-85)
  for (int i = 0; i < 3; i++) {
    double s = (double)T.at<float>(0, i) * (double)T.at<float>(0, 3);
    s += (double)T.at<float>(1, i) * (double)T.at<float>(1, 3);
    s += (double)T.at<float>(2, i) * (double)T.at<float>(2, 3);
    ow[i] = -(float)s;
  }
}
Mat inverse_of(const Mat& T) {                                 // Twc (KeyFrame.cc:87-89)
  float ow[3]; centre_of(T, ow);
  Mat W(4, 4);
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) W.at<float>(i, j) = T.at<float>(j, i); W.at<float>(i, 3) = ow[i]; }
  W.at<float>(3, 3) = 1.f;
  return W;
}
Mat mul44(const Mat& A, const Mat& B) {
  Mat C(4, 4);
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = (double)A.at<float>(i, 0) * (double)B.at<float>(0, j);
      s += (double)A.at<float>(i, 1) * (double)B.at<float>(1, j);
      s += (double)A.at<float>(i, 2) * (double)B.at<float>(2, j);
      s += (double)A.at<float>(i, 3) * (double)B.at<float>(3, j);
      C.at<float>(i, j) = (float)s;
    }
  return C;
}
void set_pose(KeyFrame* pKF, const Mat& T) {                    // KeyFrame::SetPose: the double's SetPose plus the Ow the reference derives
  pKF->SetPose(T);
  float ow[3]; centre_of(T, ow);
  pKF->Ow = Mat(3, 1, ow);
}

// ------------------------------------------------------------------ Eigen quaternions and g2o::Sim3 on the host, as sim3.h writes them
struct V3 { double x, y, z; };
V3 cross(const V3& a, const V3& b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V3 rotate(const double* q, const V3& v) {                       // Eigen q * v
  const V3 qv{q[0], q[1], q[2]};
  V3 uv = cross(qv, v);
  uv = V3{uv.x + uv.x, uv.y + uv.y, uv.z + uv.z};
  const V3 c = cross(qv, uv);
  return V3{(v.x + q[3] * uv.x) + c.x, (v.y + q[3] * uv.y) + c.y, (v.z + q[3] * uv.z) + c.z};
}
void quat_from_R(const double R[3][3], double* q) {             // Eigen's Quaterniond(Matrix3d)
  double t = R[0][0] + R[1][1] + R[2][2];
  if (t > 0.0) {
    t = std::sqrt(t + 1.0); q[3] = 0.5 * t; t = 0.5 / t;
    q[0] = (R[2][1] - R[1][2]) * t; q[1] = (R[0][2] - R[2][0]) * t; q[2] = (R[1][0] - R[0][1]) * t;
  } else {
    int i = 0;
    if (R[1][1] > R[0][0]) i = 1;
    if (R[2][2] > R[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
    q[i] = 0.5 * t; t = 0.5 / t;
    q[3] = (R[k][j] - R[j][k]) * t; q[j] = (R[j][i] + R[i][j]) * t; q[k] = (R[k][i] + R[i][k]) * t;
  }
}
void quat_to_R(const double* q, double R[3][3]) {               // Eigen's toRotationMatrix
  const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0][0] = 1.0 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
  R[1][0] = txy + twz; R[1][1] = 1.0 - (txx + tzz); R[1][2] = tyz - twx;
  R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1.0 - (txx + tyy);
}
Sim3 sim3_of_pose(const Mat& T) {                               // Sim3(toMatrix3d(R), toVector3d(t), 1.0)
  double R[3][3];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = (double)T.at<float>(i, j);
  Sim3 S; quat_from_R(R, S.q);
  for (int i = 0; i < 3; i++) S.t[i] = (double)T.at<float>(i, 3);
  S.s = 1.0;
  return S;
}
Sim3 sim3_mul(const Sim3& a, const Sim3& b) {                   // sim3.h:264-272
  Sim3 r;
  r.q[3] = a.q[3] * b.q[3] - a.q[0] * b.q[0] - a.q[1] * b.q[1] - a.q[2] * b.q[2];
  r.q[0] = a.q[3] * b.q[0] + a.q[0] * b.q[3] + a.q[1] * b.q[2] - a.q[2] * b.q[1];
  r.q[1] = a.q[3] * b.q[1] + a.q[1] * b.q[3] + a.q[2] * b.q[0] - a.q[0] * b.q[2];
  r.q[2] = a.q[3] * b.q[2] + a.q[2] * b.q[3] + a.q[0] * b.q[1] - a.q[1] * b.q[0];
  const V3 v = rotate(a.q, V3{b.t[0], b.t[1], b.t[2]});
  r.t[0] = a.s * v.x + a.t[0]; r.t[1] = a.s * v.y + a.t[1]; r.t[2] = a.s * v.z + a.t[2];
  r.s = a.s * b.s;
  return r;
}
Sim3 sim3_inverse(const Sim3& a) {                              // sim3.h:222-224
  Sim3 r;
  r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
  const double m = -1. / a.s;
  const V3 v = rotate(r.q, V3{m * a.t[0], m * a.t[1], m * a.t[2]});
  r.t[0] = v.x; r.t[1] = v.y; r.t[2] = v.z; r.s = 1. / a.s;
  return r;
}
V3 sim3_map(const Sim3& S, const V3& x) { const V3 r = rotate(S.q, x); return V3{S.s * r.x + S.t[0], S.s * r.y + S.t[1], S.s * r.z + S.t[2]}; }
Mat se3_of_sim3(const Sim3& S) {                                // toCvSE3(R, t*(1./s))
  double R[3][3]; quat_to_R(S.q, R);
  const double inv = 1. / S.s;
  Mat T(4, 4);
  for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) T.at<float>(i, j) = (float)R[i][j]; T.at<float>(i, 3) = (float)(S.t[i] * inv); }
  T.at<float>(3, 3) = 1.f;
  return T;
}
void correct_point(MapPoint* pMP, const Sim3& Siw, const Sim3& Swi) {
  const Mat P3Dw = pMP->GetWorldPos();
  const V3 Q = sim3_map(Swi, sim3_map(Siw, V3{(double)P3Dw.at<float>(0), (double)P3Dw.at<float>(1), (double)P3Dw.at<float>(2)}));
  Mat c(3, 1); c.at<float>(0) = (float)Q.x; c.at<float>(1) = (float)Q.y; c.at<float>(2) = (float)Q.z;
  pMP->SetWorldPos(c);
}

// ------------------------------------------------------------------ the object graph of a scene
struct World {
  std::vector<KeyFrame> kfs;                                   // one allocation each: ascending index = ascending pointer
  std::vector<MapPoint> pts;
  Map map;
  KeyFrame* cur = nullptr;
  std::vector<KeyFrame*> connected;
  Sim3 scw;
  KeyFrameAndPose before, after, corrected, non_corrected;
  unsigned long nLoopKF = 77;
};

void build(const Scene& S, World& W) {
  W.kfs.assign(S.n_kf, KeyFrame()); W.pts.assign(S.n_points, MapPoint());
  for (int k = 0; k < S.n_kf; k++) {
    KeyFrame& F = W.kfs[k];
    F.mnId = (unsigned long)k + 1;
    set_pose(&F, pose_mat(&S.tcw[12 * (size_t)k]));
    F.n_set_pose = 0;
    F.mnScaleLevels = S.n_levels; F.mvScaleFactors = S.level_scale;
    F.mvKeysUn.assign(1, lld_slam::KeyPoint()); F.mvKeysUn[0].octave = k % S.n_levels;   // keypoint 0: what an absent pRefKF reads
    W.map.AddKeyFrame(&F);
  }
  for (int p = 0; p < S.n_points; p++) {
    MapPoint& M = W.pts[p];
    M.mnId = (unsigned long)p; M.mbBad = S.bad[p] != 0;
    M.mWorldPos = Mat(3, 1, &S.pos[3 * (size_t)p]); M.mNormalVector = Mat(3, 1, &S.normal[3 * (size_t)p]);
    M.mfMinDistance = S.mn[p]; M.mfMaxDistance = S.mx[p];
    M.mpRefKF = &W.kfs[S.ref_kf[p]];
    for (size_t o = 0; o < S.obs[p].size(); o++) {
      KeyFrame& F = W.kfs[S.obs[p][o]];
      lld_slam::KeyPoint kp; kp.octave = S.obs[p][o] == S.ref_kf[p] ? S.ref_level[p] : (int)((p + o) % S.n_levels);
      M.mObservations[&F] = F.mvKeysUn.size();
      F.mvKeysUn.push_back(kp);
    }
    W.map.AddMapPoint(&M);
  }
  if (S.kind == 1) {
    W.cur = &W.kfs[S.conn[S.cur]];
    for (size_t r = 0; r < S.conn.size(); r++) {
      KeyFrame& F = W.kfs[S.conn[r]];
      if (&F != W.cur) W.connected.push_back(&F);
      for (size_t e = 0; e < S.lists[r].size(); e++) F.mvpMapPoints.push_back(&W.pts[S.lists[r][e]]);
      F.mvpMapPoints.push_back(nullptr);
    }
    W.connected.push_back(W.cur);                               // (:438)
    for (int q = 0; q < 4; q++) W.scw.q[q] = S.scw[q];
    for (int q = 0; q < 3; q++) W.scw.t[q] = S.scw[4 + q];
    W.scw.s = S.scw[7];
    for (int p = 0; p < S.n_points; p++) if (S.already[p]) W.pts[p].mnCorrectedByKF = W.cur->mnId;
  } else if (S.kind == 2) {
    W.cur = &W.kfs[0];
    for (int k = 0; k < S.n_kf; k++) {
      Sim3 b, a;
      for (int q = 0; q < 4; q++) { b.q[q] = S.before[8 * (size_t)k + q]; a.q[q] = S.after[8 * (size_t)k + q]; }
      for (int q = 0; q < 3; q++) { b.t[q] = S.before[8 * (size_t)k + 4 + q]; a.t[q] = S.after[8 * (size_t)k + 4 + q]; }
      b.s = S.before[8 * (size_t)k + 7]; a.s = S.after[8 * (size_t)k + 7];
      W.before[&W.kfs[k]] = b; W.after[&W.kfs[k]] = a;
    }
    for (int p = 0; p < S.n_points; p++)
      if (S.corr_kf[p] != S.ref_kf[p]) { W.pts[p].mnCorrectedByKF = W.cur->mnId; W.pts[p].mnCorrectedReference = W.kfs[S.corr_kf[p]].mnId; }
  } else {
    for (int k = 0; k < S.n_kf; k++) {
      KeyFrame& F = W.kfs[k];
      if (S.kf_in_gba[k]) { F.mnBAGlobalForKF = W.nLoopKF; F.mTcwGBA = pose_mat(&S.tcw_gba[12 * (size_t)k]); }
      if (S.parent[k] >= 0) { F.mpParent = &W.kfs[S.parent[k]]; W.kfs[S.parent[k]].AddChild(&F); }
    }
    for (size_t q = 0; q < S.origins.size(); q++) W.map.mvpKeyFrameOrigins.push_back(&W.kfs[S.origins[q]]);
    for (int p = 0; p < S.n_points; p++)
      if (S.pt_in_gba[p]) { W.pts[p].mnBAGlobalForKF = W.nLoopKF; W.pts[p].mPosGBA = Mat(3, 1, &S.pos_gba[3 * (size_t)p]); }
  }
}

// ------------------------------------------------------------------ the host route: the reference's loops
void host_correct_loop(const lld_amd::Context& ctx, World& W) {          // src/LoopClosing.cc:440-518
  KeyFrame* mpCurrentKF = W.cur;
  KeyFrameAndPose& CorrectedSim3 = W.corrected; KeyFrameAndPose& NonCorrectedSim3 = W.non_corrected;
  CorrectedSim3[mpCurrentKF] = W.scw;
  const Mat Twc = inverse_of(mpCurrentKF->GetPose());
  for (std::vector<KeyFrame*>::iterator vit = W.connected.begin(), vend = W.connected.end(); vit != vend; vit++) {
    KeyFrame* pKFi = *vit;
    const Mat Tiw = pKFi->GetPose();
    if (pKFi != mpCurrentKF) CorrectedSim3[pKFi] = sim3_mul(sim3_of_pose(mul44(Tiw, Twc)), W.scw);
    NonCorrectedSim3[pKFi] = sim3_of_pose(Tiw);
  }
  for (KeyFrameAndPose::iterator mit = CorrectedSim3.begin(), mend = CorrectedSim3.end(); mit != mend; mit++) {
    KeyFrame* pKFi = mit->first;
    const Sim3 g2oCorrectedSiw = mit->second, g2oCorrectedSwi = sim3_inverse(g2oCorrectedSiw), g2oSiw = NonCorrectedSim3[pKFi];
    const std::vector<MapPoint*> vpMPsi = pKFi->GetMapPointMatches();
    std::vector<MapPoint*> corrected;
    for (size_t iMP = 0, endMPi = vpMPsi.size(); iMP < endMPi; iMP++) {
      MapPoint* pMPi = vpMPsi[iMP];
      if (!pMPi) continue;
      if (pMPi->isBad()) continue;
      if (pMPi->mnCorrectedByKF == mpCurrentKF->mnId) continue;
      correct_point(pMPi, g2oSiw, g2oCorrectedSwi);
      pMPi->mnCorrectedByKF = mpCurrentKF->mnId;
      pMPi->mnCorrectedReference = pKFi->mnId;
      corrected.push_back(pMPi);
    }
    lld_adapter::RefreshMapPoints(ctx, corrected, LLD_LANDMARK_NORMAL_DEPTH);   // UpdateNormalAndDepth of this keyframe's points: ONE call per pKFi
    set_pose(pKFi, se3_of_sim3(g2oCorrectedSiw));
  }
}

void host_essential_graph(const lld_amd::Context& ctx, World& W) {       // src/Optimizer.cc:1601-1653
  const std::vector<KeyFrame*> vpKFs = W.map.GetAllKeyFrames();
  const std::vector<MapPoint*> vpMPs = W.map.GetAllMapPoints();
  std::map<unsigned long, Sim3> vScw, vCorrectedSwc;
  for (size_t i = 0; i < vpKFs.size(); i++) {
    KeyFrame* pKFi = vpKFs[i];
    const Sim3 CorrectedSiw = W.after[pKFi];
    vScw[pKFi->mnId] = W.before[pKFi];
    vCorrectedSwc[pKFi->mnId] = sim3_inverse(CorrectedSiw);
    set_pose(pKFi, se3_of_sim3(CorrectedSiw));
  }
  for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {
    MapPoint* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    const unsigned long nIDr = pMP->mnCorrectedByKF == W.cur->mnId ? pMP->mnCorrectedReference : pMP->GetReferenceKeyFrame()->mnId;
    correct_point(pMP, vScw[nIDr], vCorrectedSwc[nIDr]);
  }
  lld_adapter::RefreshMapPoints(ctx, vpMPs, LLD_LANDMARK_NORMAL_DEPTH);         // pMP->UpdateNormalAndDepth() of every point: one call
}

void host_global_ba(World& W) {                                          // src/LoopClosing.cc:678-739
  const unsigned long nLoopKF = W.nLoopKF;
  std::list<KeyFrame*> lpKFtoCheck(W.map.mvpKeyFrameOrigins.begin(), W.map.mvpKeyFrameOrigins.end());
  while (!lpKFtoCheck.empty()) {
    KeyFrame* pKF = lpKFtoCheck.front();
    const std::set<KeyFrame*> sChilds = pKF->GetChilds();
    const Mat Twc = inverse_of(pKF->GetPose());
    for (std::set<KeyFrame*>::const_iterator sit = sChilds.begin(); sit != sChilds.end(); sit++) {
      KeyFrame* pChild = *sit;
      if (pChild->mnBAGlobalForKF != nLoopKF) {
        const Mat Tchildc = mul44(pChild->GetPose(), Twc);
        pChild->mTcwGBA = mul44(Tchildc, pKF->mTcwGBA);
        pChild->mnBAGlobalForKF = nLoopKF;
      }
      lpKFtoCheck.push_back(pChild);
    }
    pKF->mTcwBefGBA = pKF->GetPose();
    set_pose(pKF, pKF->mTcwGBA);
    lpKFtoCheck.pop_front();
  }
  const std::vector<MapPoint*> vpMPs = W.map.GetAllMapPoints();
  for (size_t i = 0; i < vpMPs.size(); i++) {
    MapPoint* pMP = vpMPs[i];
    if (pMP->isBad()) continue;
    if (pMP->mnBAGlobalForKF == nLoopKF) { pMP->SetWorldPos(pMP->mPosGBA); continue; }
    KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
    if (pRefKF->mnBAGlobalForKF != nLoopKF) continue;
    const Mat& Tb = pRefKF->mTcwBefGBA; const Mat Tn = pRefKF->GetPose(); const Mat Ow = pRefKF->GetCameraCenter(); const Mat P = pMP->GetWorldPos();
    float Xc[3]; Mat out(3, 1);
    for (int r = 0; r < 3; r++) {                               // Xc = Rcw*P + tcw
      double s = (double)Tb.at<float>(r, 0) * (double)P.at<float>(0);
      s += (double)Tb.at<float>(r, 1) * (double)P.at<float>(1);
      s += (double)Tb.at<float>(r, 2) * (double)P.at<float>(2);
      Xc[r] = (float)s + Tb.at<float>(r, 3);
    }
    for (int r = 0; r < 3; r++) {                               // Rwc*Xc + twc
      double s = (double)Tn.at<float>(0, r) * (double)Xc[0];
      s += (double)Tn.at<float>(1, r) * (double)Xc[1];
      s += (double)Tn.at<float>(2, r) * (double)Xc[2];
      out.at<float>(r) = (float)s + Ow.at<float>(r);
    }
    pMP->SetWorldPos(out);
  }
}

void run(const lld_amd::Context& ctx, int kind, World& W, bool adapter) {
  if (kind == 1) { if (adapter) lld_adapter::CorrectLoopPoses(ctx, W.cur, W.scw, W.connected, W.corrected, W.non_corrected); else host_correct_loop(ctx, W); }
  else if (kind == 2) { if (adapter) lld_adapter::ApplyEssentialGraph(ctx, &W.map, W.cur, W.before, W.after); else host_essential_graph(ctx, W); }
  else { if (adapter) lld_adapter::UpdateMapAfterGlobalBA(ctx, &W.map, W.nLoopKF); else host_global_ba(W); }
}

// ------------------------------------------------------------------ every member either route wrote, as doubles
void put_mat(std::vector<double>& o, const Mat& M, int rows, int cols) {
  for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) o.push_back(M.empty() ? 0.0 : (double)M.at<float>(r, c));
}
void put_sim3(std::vector<double>& o, const KeyFrameAndPose& m, KeyFrame* k) {
  KeyFrameAndPose::const_iterator it = m.find(k);
  o.push_back(it != m.end() ? 1.0 : 0.0);
  const Sim3 S = it != m.end() ? it->second : Sim3();
  for (int q = 0; q < 4; q++) o.push_back(S.q[q]);
  for (int q = 0; q < 3; q++) o.push_back(S.t[q]);
  o.push_back(S.s);
}
void dump(World& W, std::vector<double>& o) {
  for (size_t k = 0; k < W.kfs.size(); k++) {                    // 12 + 3 + 12 + 12 + 2 + 9 + 9 = 59 per keyframe
    KeyFrame& F = W.kfs[k];
    put_mat(o, F.Tcw, 3, 4); put_mat(o, F.Ow, 3, 1); put_mat(o, F.mTcwGBA, 3, 4); put_mat(o, F.mTcwBefGBA, 3, 4);
    o.push_back((double)F.mnBAGlobalForKF); o.push_back((double)F.n_set_pose);
    put_sim3(o, W.corrected, &F); put_sim3(o, W.non_corrected, &F);
  }
  for (size_t p = 0; p < W.pts.size(); p++) {                    // 3 + 3 + 5 = 11 per point
    MapPoint& M = W.pts[p];
    put_mat(o, M.mWorldPos, 3, 1); put_mat(o, M.mNormalVector, 3, 1);
    o.push_back((double)M.mfMinDistance); o.push_back((double)M.mfMaxDistance); o.push_back((double)M.mnCorrectedByKF);
    o.push_back((double)M.mnCorrectedReference); o.push_back((double)M.n_set_pos);
  }
}

double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

// ------------------------------------------------------------------ the same three corrections on FLAT arrays, for the timing: one new call
// against the route that existed before it (the host loop in compiled C++ with lld_mappoint_refresh for UpdateNormalAndDepth: one call per
// connected keyframe for CorrectLoop, one after the loop for the essential graph, none for the global BA).  HIP events on the context's stream
// around the whole window of either route, host work between the calls included.
struct Flat {
  lld_amd::MapCorrPoints P;
  std::vector<float> pos, normal, mn, mx;                       // what a route leaves
  std::vector<float> tiw, ow;
};

lld_amd::MapCorrPoints flat_points(const Scene& S) {
  lld_amd::MapCorrPoints P;
  P.pos = S.pos; P.bad.assign(S.bad.begin(), S.bad.end()); P.ref_kf.assign(S.ref_kf.begin(), S.ref_kf.end());
  P.ref_level.assign(S.ref_level.begin(), S.ref_level.end()); P.level_scale = S.level_scale;
  P.obs_start.assign(1, 0);
  for (int p = 0; p < S.n_points; p++) { P.obs_kf.insert(P.obs_kf.end(), S.obs[p].begin(), S.obs[p].end()); P.obs_start.push_back((int32_t)P.obs_kf.size()); }
  return P;
}
void correct_flat(float* X, const Sim3& Siw, const Sim3& Swi) {
  const V3 Q = sim3_map(Swi, sim3_map(Siw, V3{(double)X[0], (double)X[1], (double)X[2]}));
  X[0] = (float)Q.x; X[1] = (float)Q.y; X[2] = (float)Q.z;
}
Sim3 sim3_of8(const double* d) { Sim3 S; for (int q = 0; q < 4; q++) S.q[q] = d[q]; for (int q = 0; q < 3; q++) S.t[q] = d[4 + q]; S.s = d[7]; return S; }
// UpdateNormalAndDepth of the points `idx` through one lld_mappoint_refresh on the centres `ow`
void refresh_flat(const lld_amd::Context& ctx, const lld_amd::MapCorrPoints& P, const std::vector<int>& idx, const std::vector<float>& ow, Flat& F) {
  if (idx.empty()) return;
  lld_amd::MapPointBatch b;
  lld_amd::MapPointRefreshOutput io;
  const size_t n = idx.size();
  b.obs_start.assign(1, 0); b.kf_ow = ow; b.kf_bad.assign(ow.size() / 3, 0); b.level_scale = P.level_scale;
  b.pos.resize(3 * n); b.bad.resize(n); b.ref_kf.resize(n); b.ref_level.resize(n);
  io.normal.resize(3 * n); io.min_distance.resize(n); io.max_distance.resize(n);
  for (size_t i = 0; i < n; i++) {
    const int p = idx[i];
    b.obs_kf.insert(b.obs_kf.end(), P.obs_kf.begin() + P.obs_start[p], P.obs_kf.begin() + P.obs_start[p + 1]);
    b.obs_start.push_back((int32_t)b.obs_kf.size());
    std::memcpy(&b.pos[3 * i], &F.pos[3 * (size_t)p], 12); b.bad[i] = P.bad[p]; b.ref_kf[i] = P.ref_kf[p]; b.ref_level[i] = P.ref_level[p];
    std::memcpy(&io.normal[3 * i], &F.normal[3 * (size_t)p], 12); io.min_distance[i] = F.mn[p]; io.max_distance[i] = F.mx[p];
  }
  lld_amd::MapPointRefresh(ctx, b, LLD_LANDMARK_NORMAL_DEPTH, io);
  for (size_t i = 0; i < n; i++) {
    if (!(io.updated[i] & LLD_LANDMARK_NORMAL_DEPTH)) continue;
    const int p = idx[i];
    std::memcpy(&F.normal[3 * (size_t)p], &io.normal[3 * i], 12); F.mn[p] = io.min_distance[i]; F.mx[p] = io.max_distance[i];
  }
}
void flat_begin(const Scene& S, Flat& F) {
  F.pos = S.pos; F.normal = S.normal; F.mn = S.mn; F.mx = S.mx;
  F.ow.resize(3 * (size_t)S.n_kf); F.tiw = S.tcw;
  for (int k = 0; k < S.n_kf; k++) centre_of(pose_mat(&S.tcw[12 * (size_t)k]), &F.ow[3 * (size_t)k]);
}
void pose_rows_of(const Mat& T, float* o) { for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) o[4 * r + c] = T.at<float>(r, c); }

void flat_host(const lld_amd::Context& ctx, const Scene& S, Flat& F, const std::vector<std::vector<int> >& childs) {
  flat_begin(S, F);
  if (S.kind == 1) {                                             // :440-518, one refresh per connected keyframe
    const size_t nc = S.conn.size();
    const Sim3 Scw = sim3_of8(S.scw);
    const Mat Twc = inverse_of(pose_mat(&S.tcw[12 * (size_t)S.conn[S.cur]]));
    std::vector<Sim3> corrected(nc), non(nc);
    for (size_t r = 0; r < nc; r++) {
      const Mat Tiw = pose_mat(&S.tcw[12 * (size_t)S.conn[r]]);
      corrected[r] = (int)r == S.cur ? Scw : sim3_mul(sim3_of_pose(mul44(Tiw, Twc)), Scw);
      non[r] = sim3_of_pose(Tiw);
    }
    std::vector<int> already = S.already, mine;
    for (size_t r = 0; r < nc; r++) {
      const Sim3 Swi = sim3_inverse(corrected[r]);
      mine.clear();
      for (size_t e = 0; e < S.lists[r].size(); e++) {
        const int p = S.lists[r][e];
        if (S.bad[p] || already[p]) continue;
        correct_flat(&F.pos[3 * (size_t)p], non[r], Swi); already[p] = 1; mine.push_back(p);
      }
      refresh_flat(ctx, F.P, mine, F.ow, F);
      const Mat T = se3_of_sim3(corrected[r]);
      pose_rows_of(T, &F.tiw[12 * (size_t)S.conn[r]]); centre_of(T, &F.ow[3 * (size_t)S.conn[r]]);
    }
  } else if (S.kind == 2) {                                      // Optimizer.cc:1601-1653, one refresh after the loop
    std::vector<Sim3> swc((size_t)S.n_kf);
    for (int k = 0; k < S.n_kf; k++) {
      const Sim3 A = sim3_of8(&S.after[8 * (size_t)k]);
      swc[k] = sim3_inverse(A);
      const Mat T = se3_of_sim3(A);
      pose_rows_of(T, &F.tiw[12 * (size_t)k]); centre_of(T, &F.ow[3 * (size_t)k]);
    }
    std::vector<int> all;
    for (int p = 0; p < S.n_points; p++) {
      all.push_back(p);
      if (S.bad[p]) continue;
      const int r = S.corr_kf[p];
      correct_flat(&F.pos[3 * (size_t)p], sim3_of8(&S.before[8 * (size_t)r]), swc[r]);
    }
    refresh_flat(ctx, F.P, all, F.ow, F);
  } else {                                                       // LoopClosing.cc:678-739
    std::vector<Mat> tcw, gba, bef((size_t)S.n_kf);
    std::vector<int> mark = S.kf_in_gba;
    for (int k = 0; k < S.n_kf; k++) { tcw.push_back(pose_mat(&S.tcw[12 * (size_t)k])); gba.push_back(pose_mat(&S.tcw_gba[12 * (size_t)k])); }
    std::list<int> q(S.origins.begin(), S.origins.end());
    while (!q.empty()) {
      const int k = q.front();
      const Mat Twc = inverse_of(tcw[k]);
      for (size_t c = 0; c < childs[k].size(); c++) {
        const int ch = childs[k][c];
        if (!mark[ch]) { gba[ch] = mul44(mul44(tcw[ch], Twc), gba[k]); mark[ch] = 1; }
        q.push_back(ch);
      }
      bef[k] = tcw[k]; tcw[k] = gba[k];
      pose_rows_of(tcw[k], &F.tiw[12 * (size_t)k]); centre_of(tcw[k], &F.ow[3 * (size_t)k]);
      q.pop_front();
    }
    for (int p = 0; p < S.n_points; p++) {
      if (S.bad[p]) continue;
      float* X = &F.pos[3 * (size_t)p];
      if (S.pt_in_gba[p]) { std::memcpy(X, &S.pos_gba[3 * (size_t)p], 12); continue; }
      const int r = S.ref_kf[p];
      if (!mark[r]) continue;
      const Mat& Tb = bef[r]; const Mat& Tn = tcw[r];
      float Xc[3], out[3];
      for (int i = 0; i < 3; i++) {
        double s = (double)Tb.at<float>(i, 0) * (double)X[0]; s += (double)Tb.at<float>(i, 1) * (double)X[1]; s += (double)Tb.at<float>(i, 2) * (double)X[2];
        Xc[i] = (float)s + Tb.at<float>(i, 3);
      }
      for (int i = 0; i < 3; i++) {
        double s = (double)Tn.at<float>(0, i) * (double)Xc[0]; s += (double)Tn.at<float>(1, i) * (double)Xc[1]; s += (double)Tn.at<float>(2, i) * (double)Xc[2];
        out[i] = (float)s + F.ow[3 * (size_t)r + i];
      }
      std::memcpy(X, out, 12);
    }
  }
}

// The flat input tables of the new calls: what a caller whose map already lives in arrays holds.  Built once, outside the timed window
// (the host route reads the scene's arrays in place as well).
struct Batches { lld_amd::LoopCorrectBatch loop; lld_amd::EssentialGraphApplyBatch graph; lld_amd::GlobalBAApplyBatch gba; };

void build_batches(const Scene& S, const lld_amd::MapCorrPoints& P, Batches& B) {
  if (S.kind == 1) {
    lld_amd::LoopCorrectBatch& b = B.loop;
    b.cur = S.cur; std::memcpy(b.scw, S.scw, sizeof b.scw); b.kf_tcw = S.tcw; b.conn.assign(S.conn.begin(), S.conn.end());
    b.kf_start.assign(1, 0);
    for (size_t r = 0; r < S.lists.size(); r++) { b.kf_point.insert(b.kf_point.end(), S.lists[r].begin(), S.lists[r].end()); b.kf_start.push_back((int32_t)b.kf_point.size()); }
    b.already.assign(S.already.begin(), S.already.end()); b.points = P;
  } else if (S.kind == 2) {
    lld_amd::EssentialGraphApplyBatch& b = B.graph;
    b.sim3_before = S.before; b.sim3_after = S.after; b.corr_kf.assign(S.corr_kf.begin(), S.corr_kf.end()); b.points = P;
  } else {
    lld_amd::GlobalBAApplyBatch& b = B.gba;
    b.kf_tcw = S.tcw; b.kf_tcw_gba = S.tcw_gba; b.kf_in_gba.assign(S.kf_in_gba.begin(), S.kf_in_gba.end()); b.parent.assign(S.parent.begin(), S.parent.end());
    b.origins.assign(S.origins.begin(), S.origins.end()); b.pos = S.pos; b.pos_gba = S.pos_gba; b.bad.assign(S.bad.begin(), S.bad.end());
    b.in_gba.assign(S.pt_in_gba.begin(), S.pt_in_gba.end()); b.ref_kf.assign(S.ref_kf.begin(), S.ref_kf.end());
  }
}

void flat_device(const lld_amd::Context& ctx, const Scene& S, const Batches& B, Flat& F) {
  F.pos = S.pos; F.normal = S.normal; F.mn = S.mn; F.mx = S.mx; F.tiw = S.tcw;
  if (S.kind == 1) {
    const lld_amd::LoopCorrectBatch& b = B.loop;
    lld_amd::LoopCorrectOutput o;
    o.pos = F.pos; o.normal = F.normal; o.min_distance = F.mn; o.max_distance = F.mx;
    lld_amd::CorrectLoop(ctx, b, o);
    F.pos = o.pos; F.normal = o.normal; F.mn = o.min_distance; F.mx = o.max_distance;
    for (size_t r = 0; r < S.conn.size(); r++) std::memcpy(&F.tiw[12 * (size_t)S.conn[r]], &o.tiw_corrected[12 * r], 48);
  } else if (S.kind == 2) {
    const lld_amd::EssentialGraphApplyBatch& b = B.graph;
    lld_amd::EssentialGraphApplyOutput o;
    o.pos = F.pos; o.normal = F.normal; o.min_distance = F.mn; o.max_distance = F.mx;
    lld_amd::ApplyEssentialGraph(ctx, b, o);
    F.pos = o.pos; F.normal = o.normal; F.mn = o.min_distance; F.mx = o.max_distance; F.tiw = o.tiw;
  } else {
    const lld_amd::GlobalBAApplyBatch& b = B.gba;
    lld_amd::GlobalBAApplyOutput o;
    o.pos = F.pos; o.tcw_new = S.tcw;
    lld_amd::ApplyGlobalBA(ctx, b, o);
    F.pos = o.pos; F.tiw = o.tcw_new;
  }
}

#define HIP_OK(x) do { if ((x) != hipSuccess) { std::fprintf(stderr, "%s failed\n", #x); std::exit(3); } } while (0)

int time_flat(const lld_amd::Context& ctx, const Scene& S, int reps) {
  std::vector<std::vector<int> > childs((size_t)S.n_kf);
  if (S.kind == 3) for (int k = 0; k < S.n_kf; k++) if (S.parent[k] >= 0) childs[S.parent[k]].push_back(k);
  Flat F[2];
  F[0].P = F[1].P = flat_points(S);
  Batches B;
  build_batches(S, F[1].P, B);
  hipStream_t stream = static_cast<hipStream_t>(lld_ctx_stream(ctx.get()));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
  std::vector<double> ms[2];
  for (int i = 0; i < 2 * reps + 4; i++) {                       // the routes alternate; the first two pairs warm up
    const int dev = i & 1;
    HIP_OK(hipEventRecord(e0, stream));
    if (dev) flat_device(ctx, S, B, F[1]); else flat_host(ctx, S, F[0], childs);
    HIP_OK(hipEventRecord(e1, stream));
    HIP_OK(hipEventSynchronize(e1));
    float t = 0.f; HIP_OK(hipEventElapsedTime(&t, e0, e1));
    if (i >= 4) ms[dev].push_back((double)t);
  }
  const bool equal = F[0].pos == F[1].pos && F[0].normal == F[1].normal && F[0].mn == F[1].mn && F[0].mx == F[1].mx && F[0].tiw == F[1].tiw;
  std::vector<double> d = ms[1], h = ms[0];
  std::sort(d.begin(), d.end()); std::sort(h.begin(), h.end());
  std::printf("{\"kind\": %d, \"n_kf\": %d, \"n_points\": %d, \"reps\": %d, \"timer\": \"HIP events on the context's stream around the whole window\", "
              "\"outputs_bit_equal\": %s, \"one_call_ms\": %.4f, \"one_call_iqr_ms\": %.4f, \"previous_route_ms\": %.4f, \"previous_route_iqr_ms\": %.4f}\n",
              S.kind, S.n_kf, S.n_points, reps, equal ? "true" : "false", median(d), d[(3 * d.size()) / 4] - d[d.size() / 4], median(h),
              h[(3 * h.size()) / 4] - h[h.size() / 4]);
  HIP_OK(hipEventDestroy(e0)); HIP_OK(hipEventDestroy(e1));
  return equal ? 0 : 4;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s scene.bin out.bin [reps]\n", argv[0]); return 2; }
  const Scene S = read_scene(argv[1]);
  const int reps = argc > 3 ? std::atoi(argv[3]) : 0;
  lld_amd::Context ctx(0);
  if (argc > 4 && std::string(argv[4]) == "flat") return time_flat(ctx, S, reps);
  std::vector<double> out;
  for (int adapter = 1; adapter >= 0; adapter--) {
    World W; build(S, W);
    run(ctx, S.kind, W, adapter != 0);
    dump(W, out);
  }
  std::ofstream f(argv[2], std::ios::binary);
  const int head[2] = {S.n_kf, S.n_points};
  f.write(reinterpret_cast<const char*>(head), sizeof head);
  f.write(reinterpret_cast<const char*>(out.data()), (std::streamsize)(out.size() * sizeof(double)));
  if (reps > 0) {
    std::vector<double> ms[2];
    for (int i = 0; i < 2 * reps + 2; i++) {                     // the two routes alternate; the first pair warms up
      const int adapter = i & 1;
      World W; build(S, W);
      const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
      run(ctx, S.kind, W, adapter != 0);                          // both end in a stream synchronise (or touch no device at all)
      const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (i >= 2) ms[adapter].push_back(dt);
    }
    std::vector<double> a = ms[1], h = ms[0];
    std::sort(a.begin(), a.end()); std::sort(h.begin(), h.end());
    std::printf("{\"kind\": %d, \"n_kf\": %d, \"n_points\": %d, \"reps\": %d, \"adapter_ms\": %.4f, \"adapter_iqr_ms\": %.4f, \"host_ms\": %.4f, \"host_iqr_ms\": %.4f}\n",
                S.kind, S.n_kf, S.n_points, reps, median(a), a[(3 * a.size()) / 4] - a[a.size() / 4], median(h), h[(3 * h.size()) / 4] - h[h.size() / 4]);
  }
  return 0;
}
