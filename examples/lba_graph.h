// lba_graph.h — the object graph the local-BA harnesses run on (adapter_harness.cpp `ba`, map_ba_harness.cpp): KeyFrame / MapPoint / MapLine
// test doubles (adapters/lld_slam_objects.h) built from a flat window.
//
// The graph is deliberately awkward: keyframes sit at shuffled places of one array (std::map<KeyFrame*, ...> iterates by ADDRESS, so the
// pointer order is a shuffle of the camera order - and the same shuffle in every graph built from the same seed, which is what lets two
// copies of a graph be compared bit for bit), their mnIds are a permutation of the input's camera order, one covisible keyframe has mnId 0
// (fixed although local), and there are objects the reference skips: a bad MapPoint, a MapLine with two observations, a bad observing
// KeyFrame that is also a covisible one, keypoints without a landmark.
#ifndef LLD_EXAMPLES_LBA_GRAPH_H
#define LLD_EXAMPLES_LBA_GRAPH_H

#include <algorithm>
#include <cmath>
#include <map>
#include <random>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../adapters/lld_optimizer_adapter.h"

namespace lba_graph {

using namespace lld_slam;

inline std::vector<float> level_table() { std::vector<float> t(8); lld_orb_inv_level_sigma2(1.2f, 8, t.data()); return t; }
inline int octave_of(const std::vector<float>& table, double inv_sigma2) {
  int best = 0; double d = 1e300;
  for (int o = 0; o < (int)table.size(); o++) { const double e = std::abs((double)table[o] - inv_sigma2); if (e < d) { d = e; best = o; } }
  return best;
}
inline Mat pose_mat(const double* qt7) { float T[16]; lld_se3_to_tcw_f32(qt7, T); return Mat(4, 4, T); }
inline Mat k_mat(float fx, float fy, float cx, float cy) { Mat K(3, 3); K.at<float>(0, 0) = fx; K.at<float>(1, 1) = fy; K.at<float>(0, 2) = cx; K.at<float>(1, 2) = cy; K.at<float>(2, 2) = 1.f; return K; }
inline KeyLine key_line(const double* seg, int octave) { KeyLine k; k.startPointX = (float)seg[0]; k.startPointY = (float)seg[1]; k.endPointX = (float)seg[2]; k.endPointY = (float)seg[3]; k.octave = octave; return k; }

// mnIds of the objects the reference skips (the defaults are the ones adapter_harness has always used; a caller whose slots are mnIds,
// like MapOnDevice, passes small ones)
struct OddIds { unsigned long bad_kf = 777, bad_mp = 999999, short_ml = 888888; };

struct Graph {
  std::vector<KeyFrame> kf_pool; std::vector<MapPoint> mp_pool; std::vector<MapLine> ml_pool;
  std::vector<KeyFrame*> kf;                 // by camera index of the input window
  KeyFrame* bad_kf = nullptr; KeyFrame* pKF = nullptr;
  std::vector<MapPoint*> mp; MapPoint* bad_mp = nullptr;
  std::vector<MapLine*> ml; MapLine* short_ml = nullptr;
  std::map<const KeyFrame*, int> kf_orig; std::map<const MapPoint*, int> mp_orig; std::map<const MapLine*, int> ml_orig;
  std::map<std::pair<const KeyFrame*, const MapPoint*>, int> ptobs_orig;
  std::map<std::pair<const KeyFrame*, const MapLine*>, int> lnobs_orig;
  Graph() {}
  Graph(const Graph&) = delete;
  Graph& operator=(const Graph&) = delete;

  // camg: fx fy cx cy bf
  void build(const lld_amd::BAWindow& w, const double* camg, std::mt19937& rng, const OddIds& odd = OddIds()) {
    const int n_cams = w.n_cams(), n_free = w.n_free_cams, n_pts = w.n_points(), n_lns = w.n_lines();
    if (n_free < 1) throw std::runtime_error("the graph needs a free camera (pKF)");
    const std::vector<float> table = level_table();

    // ---- keyframes: at shuffled places, mnIds a permutation of the input order; the first fixed camera becomes mnId 0 and local
    std::vector<int> alloc_order(n_cams + 1);
    for (int i = 0; i <= n_cams; i++) alloc_order[i] = i;
    std::shuffle(alloc_order.begin(), alloc_order.end(), rng);
    kf_pool = std::vector<KeyFrame>(n_cams + 1);
    std::vector<KeyFrame*> kf_store(n_cams + 1);
    for (int place = 0; place <= n_cams; place++) kf_store[alloc_order[place]] = &kf_pool[place];
    kf.assign(n_cams, nullptr);
    for (int c = 0; c < n_cams; c++) kf[c] = kf_store[c];
    bad_kf = kf_store[n_cams];                                                     // an observer the reference skips
    std::vector<int> perm(n_free);
    for (int i = 0; i < n_free; i++) perm[i] = i;
    std::shuffle(perm.begin(), perm.end(), rng);
    for (int c = 0; c < n_cams; c++) {
      KeyFrame& K = *kf[c];
      K.mnId = c < n_free ? (unsigned long)(5 + 2 * perm[c]) : (c == n_free ? 0ul : (unsigned long)(1000 + c));
      K.fx = (float)camg[0]; K.fy = (float)camg[1]; K.cx = (float)camg[2]; K.cy = (float)camg[3]; K.mbf = (float)camg[4];
      K.mK = k_mat(K.fx, K.fy, K.cx, K.cy);
      K.mvInvLevelSigma2 = table;
      K.Tcw = pose_mat(&w.cam_qt[7 * (size_t)c]);
      kf_orig[&K] = c;
    }
    bad_kf->mnId = odd.bad_kf; bad_kf->mbBad = true; bad_kf->mvInvLevelSigma2 = table; bad_kf->Tcw = pose_mat(&w.cam_qt[0]);
    bad_kf->fx = (float)camg[0]; bad_kf->mK = k_mat((float)camg[0], (float)camg[1], (float)camg[2], (float)camg[3]);
    // pKF = the free camera with the largest mnId; every other free camera and the mnId-0 one are covisible (in shuffled order)
    pKF = kf[0];
    for (int c = 1; c < n_free; c++) if (kf[c]->mnId > pKF->mnId) pKF = kf[c];
    for (int c = 0; c < n_cams; c++) if (kf[c] != pKF && (c < n_free || c == n_free)) pKF->mvpOrderedConnectedKeyFrames.push_back(kf[c]);
    std::shuffle(pKF->mvpOrderedConnectedKeyFrames.begin(), pKF->mvpOrderedConnectedKeyFrames.end(), rng);
    pKF->mvpOrderedConnectedKeyFrames.push_back(bad_kf);                           // a bad covisible keyframe: marked local, never a camera

    // ---- map points and their observations
    mp_pool = std::vector<MapPoint>(n_pts + 1);
    mp.assign(n_pts, nullptr);
    for (int p = 0; p < n_pts; p++) {
      MapPoint& M = mp_pool[p];
      mp[p] = &M;
      M.mnId = (unsigned long)(3 * p + 1);
      M.mWorldPos = Mat(3, 1);
      for (int k = 0; k < 3; k++) M.mWorldPos.at<float>(k) = (float)w.pt_xyz[3 * (size_t)p + k];
      mp_orig[&M] = p;
      for (int o = w.pt_obs_start[p]; o < w.pt_obs_start[p + 1]; o++) {
        KeyFrame& K = *kf[w.pt_obs_cam[o]];
        KeyPoint kp; kp.pt.x = (float)w.pt_obs_uvr[3 * (size_t)o]; kp.pt.y = (float)w.pt_obs_uvr[3 * (size_t)o + 1]; kp.octave = octave_of(table, w.pt_obs_inv_sigma2[o]);
        if (K.mvKeysUn.size() % 5 == 2) { K.mvKeysUn.push_back(kp); K.mvuRight.push_back(-1.f); K.mvpMapPoints.push_back(nullptr); }   // a keypoint without a MapPoint in between
        M.mObservations[&K] = K.mvKeysUn.size();
        K.mvKeysUn.push_back(kp); K.mvuRight.push_back((float)w.pt_obs_uvr[3 * (size_t)o + 2]); K.mvpMapPoints.push_back(&M);
        ptobs_orig[std::make_pair((const KeyFrame*)&K, (const MapPoint*)&M)] = o;
      }
      if (p % 7 == 3) {                                                             // the bad keyframe also observes this point: skipped by the reference
        KeyPoint kp; kp.pt.x = 10.f; kp.pt.y = 10.f; kp.octave = 0;
        M.mObservations[bad_kf] = bad_kf->mvKeysUn.size();
        bad_kf->mvKeysUn.push_back(kp); bad_kf->mvuRight.push_back(5.f); bad_kf->mvpMapPoints.push_back(&M);
      }
    }
    bad_mp = &mp_pool[n_pts];                                                       // a bad MapPoint among pKF's matches: never enters the window
    bad_mp->mnId = odd.bad_mp; bad_mp->mbBad = true; bad_mp->mWorldPos = Mat(3, 1);
    { KeyPoint kp; kp.pt.x = 1.f; kp.pt.y = 2.f; kp.octave = 0; bad_mp->mObservations[pKF] = pKF->mvKeysUn.size(); pKF->mvKeysUn.push_back(kp); pKF->mvuRight.push_back(1.f); pKF->mvpMapPoints.push_back(bad_mp); }

    // ---- map lines
    ml_pool = std::vector<MapLine>(n_lns + 1);
    ml.assign(n_lns, nullptr);
    for (int l = 0; l < n_lns; l++) {
      MapLine& L = ml_pool[l];
      ml[l] = &L;
      L.mnId = (unsigned long)(2 * l + 7);
      L.mX0 = Vector3d(w.line_x0[3 * (size_t)l], w.line_x0[3 * (size_t)l + 1], w.line_x0[3 * (size_t)l + 2]);
      L.mDir = Vector3d(w.line_dir[3 * (size_t)l], w.line_dir[3 * (size_t)l + 1], w.line_dir[3 * (size_t)l + 2]);
      ml_orig[&L] = l;
      for (int o = w.ln_obs_start[l]; o < w.ln_obs_start[l + 1]; o++) {
        KeyFrame& K = *kf[w.ln_obs_cam[o]];
        const bool has_right = !(w.ln_obs_right[4 * (size_t)o] < 0);
        L.mObservations[&K] = K.mvLinesLeft.size();
        K.mvLinesLeft.push_back(key_line(&w.ln_obs_left[4 * (size_t)o], w.ln_obs_octave[2 * (size_t)o]));
        if (has_right) { K.line_matches.push_back((int)K.mvLinesRight.size()); K.mvLinesRight.push_back(key_line(&w.ln_obs_right[4 * (size_t)o], w.ln_obs_octave[2 * (size_t)o + 1])); }
        else K.line_matches.push_back(-1);
        K.mvpMapLines.push_back(&L);
        lnobs_orig[std::make_pair((const KeyFrame*)&K, (const MapLine*)&L)] = o;
      }
    }
    short_ml = &ml_pool[n_lns];                                                     // a MapLine with two observations: below the `Observations() < 4` bar (:972)
    short_ml->mnId = odd.short_ml; short_ml->mX0 = Vector3d(1, 2, 3); short_ml->mDir = Vector3d(1, 0, 0);
    for (int c = 0; c < std::min(2, n_free); c++) {
      KeyFrame& K = *kf[c];
      short_ml->mObservations[&K] = K.mvLinesLeft.size();
      const double seg[4] = {10, 10, 50, 50};
      K.mvLinesLeft.push_back(key_line(seg, 0)); K.line_matches.push_back(-1); K.mvpMapLines.push_back(short_ml);
    }
  }
};

}  // namespace lba_graph

#endif
