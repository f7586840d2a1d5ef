// local_map_objects.cpp — the object mode of local_map_harness: Tracking::TrackLocalMap with its UpdateLocalMap on live KeyFrame / MapPoint /
// MapLine / Frame test doubles, two ways on two copies of one graph:
//   host    UpdateLocalMap's two loops (local_map_host.cpp) on tables gathered from the objects, written back into the objects the way
//           src/Tracking.cc:1684-1834 does, then the existing FrameOnDevice::TrackLocalMap on the lists;
//   device  MapOnDevice::Upload once, then FrameOnDevice::TrackLocalMap(.., MapOnDevice&, ..).
// A second frame follows after the same change to both graphs (points moved, points turned bad, a keyframe's matches and covisibles
// changed), which the device route learns through MapOnDevice::UpdatePoints / UpdateKeyFrames.  The frame enters through SetFrameState with
// what a TrackedFrame's stage 1 left (local_map_harness.cpp ran it).  After each frame both graphs are dumped: the members UpdateLocalMap and
// TrackLocalMap write.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../adapters/lld_map_adapter.h"
#include "../adapters/lld_tracking_adapter.h"
#include "local_map_harness.h"
#include "local_map_host.h"

namespace {

using lld_slam::Frame;
using lld_slam::KeyFrame;
using lld_slam::MapLine;
using lld_slam::MapPoint;
using lld_slam::Mat;
using lld_slam::MatU8;

struct Graph {
  std::vector<KeyFrame> kfs;                        // in one block, slots in descending order: pointer order is the reverse of slot order in both copies
  std::vector<KeyFrame*> kf_of;                     // by slot, NULL: the map file holds no keyframe there
  std::vector<MapPoint> pts; std::vector<MapLine> lns;
  lld_slam::Map map;
  lld_adapter::LocalMapMembers lm;
};

void build_graph(Graph& G, const HarnessInput& in) {
  const lld_amd::DeviceMap::KeyFrameRows& K = *in.K;
  const int nk = in.L.max_keyframes, np = in.L.max_points, nln = in.L.max_lines, dim = in.L.line_dim;
  std::vector<int> slots;
  for (int s = nk - 1; s >= 0; s--) if (K.order_key[s] != 0) slots.push_back(s);
  G.kfs.resize(slots.size()); G.kf_of.assign(nk, nullptr); G.pts.resize(np); G.lns.resize(nln);
  for (size_t p = 0; p < slots.size(); p++) { G.kfs[p].mnId = slots[p]; G.kfs[p].mbBad = K.bad[slots[p]] != 0; G.kf_of[slots[p]] = &G.kfs[p]; }
  for (size_t p = 0; p < slots.size(); p++) {
    const int s = slots[p]; KeyFrame& kf = G.kfs[p];
    if (K.parent[s] >= 0) kf.mpParent = G.kf_of[K.parent[s]];
    for (int j = K.cov_start[s]; j < K.cov_start[s + 1]; j++) kf.mvpOrderedConnectedKeyFrames.push_back(G.kf_of[K.cov[j]]);
    for (int j = K.child_start[s]; j < K.child_start[s + 1]; j++) kf.mspChildrens.insert(G.kf_of[K.child[j]]);
    for (int j = K.point_start[s]; j < K.point_start[s + 1]; j++) kf.mvpMapPoints.push_back(K.point[j] < 0 ? nullptr : &G.pts[K.point[j]]);
    for (int j = K.line_start[s]; j < K.line_start[s + 1]; j++) kf.mvpMapLines.push_back(K.line[j] < 0 ? nullptr : &G.lns[K.line[j]]);
    G.map.AddKeyFrame(&kf);
  }
  for (int s = 0; s < np; s++) {
    MapPoint& P = G.pts[s];
    P.mnId = s; P.mWorldPos = Mat(3, 1, &(*in.p_pos)[3 * s]); P.mNormalVector = Mat(3, 1, &(*in.p_nrm)[3 * s]);
    P.mfMinDistance = (*in.p_mind)[s]; P.mfMaxDistance = (*in.p_maxd)[s];
    P.mDescriptor = MatU8(1, 32); std::memcpy(P.mDescriptor.ptr<unsigned char>(), &(*in.p_desc)[8 * s], 32);
    P.mbBad = (*in.pt_state)[s] == 2;
    for (int o = (*in.obs_start)[s]; o < (*in.obs_start)[s + 1]; o++) { P.mObservations[G.kf_of[(*in.obs)[o]]] = 0; P.nObs++; }
    if ((*in.pt_state)[s]) G.map.AddMapPoint(&P);
  }
  for (int s = 0; s < nln; s++) {
    MapLine& Ln = G.lns[s];
    Ln.mnId = s; Ln.mbBad = (*in.ln_bad)[s] != 0;
    const double* a = &(*in.l_x0)[3 * s]; const double* d = &(*in.l_dir)[3 * s]; const double* p1 = &(*in.l_x1)[3 * s]; const double* p2 = &(*in.l_x2)[3 * s];
    Ln.mX0 = lld_slam::Vector3d(a[0], a[1], a[2]); Ln.mDir = lld_slam::Vector3d(d[0], d[1], d[2]);
    Ln.mX1 = lld_slam::Vector3d(p1[0], p1[1], p1[2]); Ln.mX2 = lld_slam::Vector3d(p2[0], p2[1], p2[2]);
    Ln.mDescriptor = Mat(1, dim, &(*in.l_desc)[(size_t)s * dim]);
    G.map.AddMapLine(&Ln);
  }
}

// mCurrentFrame as a stage 1 left it: keypoints, lines, pose, the MapPoints and MapLines it holds
void build_frame(Frame& F, Graph& G, const HarnessInput& in, unsigned long id) {
  const int nt = in.nt, nl = in.nl;
  F.N = nt; F.mnId = id; F.fx = (float)in.dc[0]; F.fy = (float)in.dc[1]; F.cx = (float)in.dc[2]; F.cy = (float)in.dc[3]; F.mbf = (float)in.dc[4]; F.mb = F.mbf / F.fx;
  F.mvKeysUn.resize(nt);
  for (int k = 0; k < nt; k++) {
    F.mvKeysUn[k].pt.x = (*in.t_xy)[2 * k]; F.mvKeysUn[k].pt.y = (*in.t_xy)[2 * k + 1]; F.mvKeysUn[k].octave = (*in.t_oct)[k]; F.mvKeysUn[k].angle = (*in.t_ang)[k];
  }
  F.mvKeys = F.mvKeysUn; F.mvuRight = *in.t_ur; F.mvInvLevelSigma2 = *in.inv_sigma2; F.mvScaleFactors = *in.scale;
  F.mvLevelSigma2.resize(in.n_levels);
  for (int l = 0; l < in.n_levels; l++) F.mvLevelSigma2[l] = 1.f / (*in.inv_sigma2)[l];
  F.mDescriptors = MatU8(nt, 32);
  if (nt) std::memcpy(F.mDescriptors.ptr<unsigned char>(), in.t_desc->data(), (size_t)nt * 32);
  F.mnMinX = in.fc[0]; F.mnMinY = in.fc[1]; F.mnMaxX = in.fc[2]; F.mnMaxY = in.fc[3]; F.mfGridElementWidthInv = in.fc[4]; F.mfGridElementHeightInv = in.fc[5];
  F.mnScaleLevels = in.n_levels; F.mfScaleFactor = in.n_levels > 1 ? (*in.scale)[1] : 1.f; F.mfLogScaleFactor = in.log_scale_factor;
  F.mvLinesLeft.resize(nl); F.mvLinesRight.resize(in.nr);
  for (int i = 0; i < nl; i++) {
    const float* s = &(*in.ln_left)[4 * i];
    F.mvLinesLeft[i].startPointX = s[0]; F.mvLinesLeft[i].startPointY = s[1]; F.mvLinesLeft[i].endPointX = s[2]; F.mvLinesLeft[i].endPointY = s[3]; F.mvLinesLeft[i].octave = (*in.ln_lo)[i];
  }
  for (int i = 0; i < in.nr; i++) {
    const float* s = &(*in.ln_right)[4 * i];
    F.mvLinesRight[i].startPointX = s[0]; F.mvLinesRight[i].startPointY = s[1]; F.mvLinesRight[i].endPointX = s[2]; F.mvLinesRight[i].endPointY = s[3]; F.mvLinesRight[i].octave = (*in.ln_ro)[i];
  }
  F.line_matches.assign(in.ln_lm->begin(), in.ln_lm->end());
  if (nl) F.mDescriptorsLines = Mat(nl, in.dim, in.ln_desc->data());
  F.mvpMapPoints.assign(nt, nullptr); F.mvbOutlier.assign(nt, false); F.mvpMapLines.assign(nl, nullptr); F.mvbOutlierLines.assign(nl, false);
  for (int k = 0; k < nt; k++) if (in.kp_id[k] >= 0) F.mvpMapPoints[k] = &G.pts[in.kp_id[k]];
  for (int i = 0; i < nl; i++) if (in.ln_id[i] >= 0) { F.mvpMapLines[i] = &G.lns[in.ln_id[i]]; F.mvpMapLines[i]->tracked_last_id = (long)id; }   // (:1117)
  F.SetPose(Mat(4, 4, in.Tcw));
}

// Tracking::UpdateLocalMap on the objects through the flat loops: gather, run, write back (:1684-1834)
void host_update_local_map(Graph& G, Frame& Cur, const lld_map_limits& L) {
  const int nk = L.max_keyframes, np = L.max_points, nln = L.max_lines;
  std::vector<uint64_t> key(nk, 0); std::vector<uint8_t> kbad(nk, 1), state(np, 0), lbad(nln + 1, 1); std::vector<int32_t> parent(nk, -1);
  std::vector<int32_t> cs(1, 0), cv, hs(1, 0), hv, ps(1, 0), pv, ls(1, 0), lv, os(1, 0), ov;
  for (int s = 0; s < nk; s++) {
    KeyFrame* kf = G.kf_of[s];
    if (kf) {
      key[s] = (uint64_t)reinterpret_cast<uintptr_t>(kf); kbad[s] = kf->isBad(); parent[s] = kf->GetParent() ? (int32_t)kf->GetParent()->mnId : -1;
      const std::vector<KeyFrame*> nb = kf->GetBestCovisibilityKeyFrames(10);
      for (size_t j = 0; j < nb.size(); j++) cv.push_back((int32_t)nb[j]->mnId);
      const std::set<KeyFrame*> ch = kf->GetChilds();
      for (std::set<KeyFrame*>::const_iterator it = ch.begin(); it != ch.end(); ++it) hv.push_back((int32_t)(*it)->mnId);
      const std::vector<MapPoint*> mps = kf->GetMapPointMatches();
      for (size_t j = 0; j < mps.size(); j++) pv.push_back(mps[j] ? (int32_t)mps[j]->mnId : -1);
      const std::vector<MapLine*> mls = kf->GetMapLineMatches();
      for (size_t j = 0; j < mls.size(); j++) lv.push_back(mls[j] ? (int32_t)mls[j]->mnId : -1);
    }
    cs.push_back((int32_t)cv.size()); hs.push_back((int32_t)hv.size()); ps.push_back((int32_t)pv.size()); ls.push_back((int32_t)lv.size());
  }
  for (int s = 0; s < np; s++) {
    MapPoint& P = G.pts[s];
    if (G.map.mspMapPoints.count(&P)) {
      state[s] = P.isBad() ? 2 : 1;
      const std::map<KeyFrame*, size_t> obs = P.GetObservations();
      for (std::map<KeyFrame*, size_t>::const_iterator it = obs.begin(); it != obs.end(); ++it) ov.push_back((int32_t)it->first->mnId);
    }
    os.push_back((int32_t)ov.size());
  }
  for (int s = 0; s < nln; s++) lbad[s] = G.lns[s].isBad();
  cv.push_back(0); hv.push_back(0); pv.push_back(0); lv.push_back(0); ov.push_back(0);
  local_map_host::Tables T;
  T.n_keyframes = nk; T.n_points = np; T.n_lines = nln; T.kf_key = key.data(); T.kf_bad = kbad.data(); T.kf_parent = parent.data();
  T.cov_start = cs.data(); T.cov = cv.data(); T.child_start = hs.data(); T.child = hv.data(); T.point_start = ps.data(); T.point = pv.data();
  T.line_start = ls.data(); T.line = lv.data(); T.pt_state = state.data(); T.obs_start = os.data(); T.obs = ov.data(); T.ln_bad = lbad.data();
  local_map_host::State S;
  for (size_t i = 0; i < G.lm.mvpLocalKeyFrames.size(); i++) S.local_keyframes.push_back((int32_t)G.lm.mvpLocalKeyFrames[i]->mnId);
  std::vector<int32_t> ids(Cur.N + 1, -1);
  for (int k = 0; k < Cur.N; k++) if (Cur.mvpMapPoints[k]) ids[k] = (int32_t)Cur.mvpMapPoints[k]->mnId;
  local_map_host::Result R;
  local_map_host::update_local_map(T, S, ids.data(), Cur.N, L.max_local_points, L.max_local_lines, R);
  if (R.status) throw std::runtime_error("the host route overflowed: the scene is not meant to");
  for (int k = 0; k < Cur.N; k++) if (ids[k] < 0) Cur.mvpMapPoints[k] = nullptr;                        // (:1743)
  lld_adapter::LocalMapMembers& lm = G.lm;
  lm.mvpLocalKeyFrames.clear(); lm.mvpLocalMapPoints.clear(); lm.local_lines.clear(); lm.local_line_descs.clear();
  for (size_t i = 0; i < S.local_keyframes.size(); i++) {
    KeyFrame* kf = G.kf_of[S.local_keyframes[i]];
    lm.mvpLocalKeyFrames.push_back(kf);
    if (!R.vote_empty) kf->mnTrackReferenceForFrame = Cur.mnId;
  }
  if (R.ref_keyframe >= 0) { lm.mpReferenceKF = G.kf_of[R.ref_keyframe]; Cur.mpReferenceKF = lm.mpReferenceKF; }
  for (size_t i = 0; i < R.local_points.size(); i++) { MapPoint* p = &G.pts[R.local_points[i]]; lm.mvpLocalMapPoints.push_back(p); p->mnTrackReferenceForFrame = Cur.mnId; }
  for (size_t i = 0; i < R.local_lines.size(); i++) {
    MapLine* l = &G.lns[R.local_lines[i]];
    lm.local_lines.push_back(l); l->mnTrackReferenceForFrame = (long)Cur.mnId;
    Mat d; l->GetDescriptor(&d); lm.local_line_descs.push_back(d);
  }
}

std::vector<int32_t> dump(const Graph& G, const Frame& Cur, int inliers) {
  std::vector<int32_t> v;
  const lld_adapter::LocalMapMembers& lm = G.lm;
  v.push_back((int32_t)lm.mvpLocalKeyFrames.size()); v.push_back((int32_t)lm.mvpLocalMapPoints.size()); v.push_back((int32_t)lm.local_lines.size());
  v.push_back(lm.mpReferenceKF ? (int32_t)lm.mpReferenceKF->mnId : -1); v.push_back(Cur.mpReferenceKF ? (int32_t)Cur.mpReferenceKF->mnId : -1); v.push_back(inliers);
  for (size_t i = 0; i < lm.mvpLocalKeyFrames.size(); i++) v.push_back((int32_t)lm.mvpLocalKeyFrames[i]->mnId);
  for (size_t i = 0; i < lm.mvpLocalMapPoints.size(); i++) v.push_back((int32_t)lm.mvpLocalMapPoints[i]->mnId);
  for (size_t i = 0; i < lm.local_lines.size(); i++) { v.push_back((int32_t)lm.local_lines[i]->mnId); v.push_back(lm.local_line_descs[i].cols); }
  for (int k = 0; k < Cur.N; k++) { v.push_back(Cur.mvpMapPoints[k] ? (int32_t)Cur.mvpMapPoints[k]->mnId : -1); v.push_back(Cur.mvbOutlier[k]); }
  for (size_t i = 0; i < Cur.mvpMapLines.size(); i++) { v.push_back(Cur.mvpMapLines[i] ? (int32_t)Cur.mvpMapLines[i]->mnId : -1); v.push_back(Cur.mvbOutlierLines[i]); }
  int32_t T[16]; std::memcpy(T, Cur.mTcw.ptr<float>(), sizeof T); v.insert(v.end(), T, T + 16);
  for (size_t s = 0; s < G.pts.size(); s++) {
    const MapPoint& P = G.pts[s];
    v.push_back(P.mnVisible); v.push_back(P.mnFound); v.push_back((int32_t)P.mnLastFrameSeen); v.push_back(P.mbTrackInView); v.push_back((int32_t)P.mnTrackReferenceForFrame);
  }
  for (size_t s = 0; s < G.lns.size(); s++) { v.push_back((int32_t)G.lns[s].tracked_last_id); v.push_back((int32_t)G.lns[s].mnTrackReferenceForFrame); }
  for (size_t s = 0; s < G.kf_of.size(); s++) v.push_back(G.kf_of[s] ? (int32_t)G.kf_of[s]->mnTrackReferenceForFrame : -1);
  return v;
}

// LocalMapping between two frames, the same on both graphs: MapPoints the frame does not hold move or turn bad, one keyframe takes further
// matches (which gain an observation) and a new best covisible.  Returns what changed.
void change_map(Graph& G, const HarnessInput& in, std::vector<MapPoint*>& points, std::vector<KeyFrame*>& keyframes) {
  std::vector<uint8_t> held(G.pts.size(), 0);
  for (int k = 0; k < in.nt; k++) if (in.kp_id[k] >= 0) held[in.kp_id[k]] = 1;
  std::vector<MapPoint*> free_live;
  for (size_t s = 0; s < G.pts.size(); s++) if (!held[s] && G.map.mspMapPoints.count(&G.pts[s]) && !G.pts[s].isBad()) free_live.push_back(&G.pts[s]);
  if (free_live.size() < 70 || G.kfs.size() < 3) throw std::runtime_error("the scene is too small for the second frame's change");
  KeyFrame* kf = &G.kfs[1];
  for (size_t i = 0; i < 65; i++) {
    MapPoint* p = free_live[i];
    if (i < 30) { Mat P = p->GetWorldPos(); P.at<float>(0) += 0.05f; p->SetWorldPos(P); }
    else if (i < 45) p->mbBad = true;
    else { kf->mvpMapPoints.push_back(p); p->mObservations[kf] = kf->mvpMapPoints.size() - 1; p->nObs++; }
    points.push_back(p);
  }
  kf->mvpOrderedConnectedKeyFrames.insert(kf->mvpOrderedConnectedKeyFrames.begin(), &G.kfs[G.kfs.size() - 1]);
  keyframes.push_back(kf);
}

}  // namespace

int run_objects(lld_amd::Context& ctx, const HarnessInput& in, const char* out_path) {
  Graph A, B;                                       // A: the host route, B: the device route
  build_graph(A, in); build_graph(B, in);
  lld_adapter::TrackingMembers tr; tr.gamma = in.dc[5]; tr.mdThr = in.dc[7];
  lld_adapter::MapOnDevice map(ctx.get(), in.L);
  map.Upload(&B.map);
  std::vector<std::vector<int32_t> > dumps;
  bool same = true;
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 1) {
      std::vector<MapPoint*> pa, pb; std::vector<KeyFrame*> ka, kb;
      change_map(A, in, pa, ka); change_map(B, in, pb, kb);
      map.UpdatePoints(pb); map.UpdateKeyFrames(kb);
    }
    const unsigned long id = 7 + pass;
    int inl_a = 0, inl_b = 0;
    Frame Fa, Fb;
    build_frame(Fa, A, in, id); build_frame(Fb, B, in, id);
    {
      lld_adapter::FrameOnDevice dev(ctx.get(), Fa);
      dev.SetFrameState(tr, Fa);
      host_update_local_map(A, Fa, in.L);
      dev.TrackLocalMap(tr, Fa, A.lm.mvpLocalMapPoints, A.lm.local_lines, A.lm.local_line_descs, &inl_a);
    }
    {
      lld_adapter::FrameOnDevice dev(ctx.get(), Fb);
      dev.SetFrameState(tr, Fb);
      dev.TrackLocalMap(tr, Fb, map, B.lm, &inl_b);
    }
    dumps.push_back(dump(A, Fa, inl_a)); dumps.push_back(dump(B, Fb, inl_b));
    same = same && dumps[2 * pass] == dumps[2 * pass + 1];
    std::printf("objects, frame %d: %zu keyframes, %zu points, %zu lines, %d inliers; routes %s\n", pass + 1, B.lm.mvpLocalKeyFrames.size(), B.lm.mvpLocalMapPoints.size(),
                B.lm.local_lines.size(), inl_b, dumps[2 * pass] == dumps[2 * pass + 1] ? "equal" : "DIFFER");
  }
  std::FILE* f = std::fopen(out_path, "wb");
  if (!f) throw std::runtime_error("cannot open the output file");
  int32_t head[5] = {4, (int32_t)dumps[0].size(), (int32_t)dumps[1].size(), (int32_t)dumps[2].size(), (int32_t)dumps[3].size()};
  std::fwrite(head, 4, 5, f);
  for (size_t d = 0; d < dumps.size(); d++) std::fwrite(dumps[d].data(), 4, dumps[d].size(), f);
  std::fclose(f);
  return same ? 0 : 3;
}
