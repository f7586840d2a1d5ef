// map_ba_harness.cpp — Optimizer::LocalBundleAdjustment on the resident map against the host adapter, on two identical copies of one object
// graph (lba_graph.h: the graph adapter_harness runs `ba` on).  Copy A goes through lld_adapter::LocalBundleAdjustment
// (adapters/lld_optimizer_adapter.cc: the window is walked on the objects), copy B through MapOnDevice::LocalBundleAdjustment
// (adapters/lld_map_adapter.cc: the window is assembled by lld_map_local_ba on the device's tables).
//
//   map_ba_harness check <in> [seed]          two calls on each copy (pKF, then one of its neighbours as pKF: the second proves that the map
//                                             followed the first call's write-back); the traces' windows and outputs and both graphs must be
//                                             identical byte for byte after each.  Prints one line per call and `differences N`; exit 2 if N > 0.
//   map_ba_harness time <in> <reps> [seed]    host clock of both routes, alternating in one process: with the stop flag raised (both return
//                                             before solving: the window assembly alone) and lowered (the whole call with write-back and
//                                             push-back).  Prints one JSON object.
//   map_ba_harness apply <scene> <answer> [solve]   flat tables, no object graph: a scene file (map_ba_apply_scene.h; tests/map_ba_apply_scenes.py
//                                             writes it) is uploaded through lld_amd::DeviceMap, the window assembled, the file's result - or
//                                             with `solve` the result of DeviceMap::LocalBa on it, then also written to <answer>.result -
//                                             applied by DeviceMap::ApplyLocalBa, and the outputs and all six row pools as the device holds
//                                             them written to <answer>.  Exit 2 when the window is not the scene's.
//   map_ba_harness apply_time <scene> <reps>  the write-back alone, two routes alternating in one process on the scene's map, both given the
//                                             result of ONE untimed solve: (A) DeviceMap::ApplyLocalBa; (B) map_ba_apply_host.cpp's tail on the
//                                             host's tables, then the lld_map_set_* calls for the rows that changed.  Before every
//                                             repetition, untimed, the map is cleared, uploaded again and the window assembled.  HIP events
//                                             on the context's stream around the whole route.  Prints one JSON object.
// Input files of check and time are the ones examples/harness.cpp reads in `ba` mode.
#ifndef __HIP_PLATFORM_AMD__
#define __HIP_PLATFORM_AMD__ 1
#endif
#include <hip/hip_runtime_api.h>               // the events of apply_time; everything else here needs no HIP header

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../adapters/lld_map_adapter.h"
#include "lba_graph.h"
#include "map_ba_apply_scene.h"

std::mutex lld_slam::MapPoint::mGlobalMutex;

using namespace lld_slam;
using lba_graph::Graph;

namespace {

struct Reader {
  FILE* f;
  explicit Reader(const char* path) : f(std::fopen(path, "rb")) { if (!f) throw std::runtime_error(std::string("cannot open ") + path); }
  ~Reader() { std::fclose(f); }
  template <class T> void get(T* p, size_t n) { if (n && std::fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short read"); }
  template <class T> void get(std::vector<T>& v, size_t n) { v.resize(n); get(v.data(), n); }
};

struct Problem { lld_amd::BAWindow w; double camg[6]; };

void read_problem(const char* in, Problem& P) {
  Reader r(in);
  int32_t h[8]; r.get(h, 8);                   // n_cams n_free n_points n_pt_obs n_lines n_ln_obs stop 0
  r.get(P.camg, 6);                            // fx fy cx cy bf gamma
  lld_amd::BAWindow& w = P.w;
  w.n_free_cams = h[1];
  r.get(w.cam_qt, 7 * (size_t)h[0]);
  r.get(w.pt_xyz, 3 * (size_t)h[2]); r.get(w.pt_obs_start, (size_t)h[2] + 1); r.get(w.pt_obs_cam, h[3]);
  r.get(w.pt_obs_uvr, 3 * (size_t)h[3]); r.get(w.pt_obs_inv_sigma2, h[3]);
  r.get(w.line_x0, 3 * (size_t)h[4]); r.get(w.line_dir, 3 * (size_t)h[4]); r.get(w.ln_obs_start, (size_t)h[4] + 1);
  r.get(w.ln_obs_cam, h[5]); r.get(w.ln_obs_left, 4 * (size_t)h[5]); r.get(w.ln_obs_right, 4 * (size_t)h[5]);
  r.get(w.ln_obs_octave, 2 * (size_t)h[5]);
}

// the skipped objects get small mnIds: a MapOnDevice's slots are mnIds
lba_graph::OddIds small_ids(const lld_amd::BAWindow& w) {
  lba_graph::OddIds o;
  o.bad_kf = 1000 + w.n_cams() + 1; o.bad_mp = 3 * (unsigned long)w.n_points() + 2; o.short_ml = 2 * (unsigned long)w.n_lines() + 8;
  return o;
}

lld_map_limits limits_for(const Graph& G, const lld_amd::BAWindow& w) {
  lld_map_limits L; std::memset(&L, 0, sizeof L);
  size_t kp = 0, kl = 0;
  for (size_t i = 0; i < G.kf_pool.size(); i++) { kp += G.kf_pool[i].mvpMapPoints.size(); kl += G.kf_pool[i].mvpMapLines.size(); }
  L.max_keyframes = 1000 + w.n_cams() + 2; L.max_points = 3 * w.n_points() + 3; L.max_lines = 2 * w.n_lines() + 9; L.line_dim = 8;
  L.max_observations = (int32_t)kp + 64; L.max_kf_points = (int32_t)kp + 64; L.max_kf_lines = (int32_t)kl + 64; L.max_children = 16;
  L.max_local_points = w.n_points() + 16; L.max_local_lines = w.n_lines() + 16;
  return L;
}

void fill_map(Graph& G, Map& map) {
  for (size_t i = 0; i < G.kf_pool.size(); i++) map.AddKeyFrame(&G.kf_pool[i]);
  for (size_t i = 0; i < G.mp_pool.size(); i++) map.AddMapPoint(&G.mp_pool[i]);
  for (size_t i = 0; i < G.ml_pool.size(); i++) map.AddMapLine(&G.ml_pool[i]);
}

// the second call's pKF: the first covisible keyframe of pKF that is a free camera; its own covisible list is pKF and pKF's other covisible
// keyframes that are not bad, in reverse order
KeyFrame* second_pkf(Graph& G) {
  KeyFrame* p2 = nullptr;
  const std::vector<KeyFrame*> nb = G.pKF->mvpOrderedConnectedKeyFrames;
  for (size_t i = 0; i < nb.size() && !p2; i++) if (!nb[i]->isBad() && nb[i]->mnId != 0) p2 = nb[i];
  if (!p2) return nullptr;
  p2->mvpOrderedConnectedKeyFrames.assign(1, G.pKF);
  for (size_t i = nb.size(); i-- > 0;) if (nb[i] != p2 && !nb[i]->isBad()) p2->mvpOrderedConnectedKeyFrames.push_back(nb[i]);   // (the bad one is no neighbour now: it gets marked fixed)
  return p2;
}

int diffs = 0;
void differ(const char* what, long i) { if (diffs++ < 20) std::fprintf(stderr, "map_ba_harness: %s differs at %ld\n", what, i); }
template <class T> void same_vec(const std::vector<T>& a, const std::vector<T>& b, const char* what) {
  if (a.size() != b.size() || (!a.empty() && std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) != 0)) differ(what, (long)a.size());
}

void same_traces(const lld_adapter::LbaTrace& a, const lld_adapter::LbaTrace& b) {
  const lld_amd::BAWindow &x = a.window, &y = b.window;
  if (std::memcmp(&x.cam, &y.cam, sizeof x.cam) != 0 || x.n_free_cams != y.n_free_cams) differ("window.cam / n_free_cams", 0);
  same_vec(x.cam_qt, y.cam_qt, "window.cam_qt"); same_vec(x.pt_xyz, y.pt_xyz, "window.pt_xyz"); same_vec(x.pt_obs_start, y.pt_obs_start, "window.pt_obs_start");
  same_vec(x.pt_obs_cam, y.pt_obs_cam, "window.pt_obs_cam"); same_vec(x.pt_obs_uvr, y.pt_obs_uvr, "window.pt_obs_uvr");
  same_vec(x.pt_obs_inv_sigma2, y.pt_obs_inv_sigma2, "window.pt_obs_inv_sigma2"); same_vec(x.line_x0, y.line_x0, "window.line_x0"); same_vec(x.line_dir, y.line_dir, "window.line_dir");
  same_vec(x.ln_obs_start, y.ln_obs_start, "window.ln_obs_start"); same_vec(x.ln_obs_cam, y.ln_obs_cam, "window.ln_obs_cam"); same_vec(x.ln_obs_left, y.ln_obs_left, "window.ln_obs_left");
  same_vec(x.ln_obs_right, y.ln_obs_right, "window.ln_obs_right"); same_vec(x.ln_obs_octave, y.ln_obs_octave, "window.ln_obs_octave");
  const lld_amd::BAOutput &p = a.output, &q = b.output;
  same_vec(p.cam_qt, q.cam_qt, "output.cam_qt"); same_vec(p.pt_xyz, q.pt_xyz, "output.pt_xyz"); same_vec(p.line_x0, q.line_x0, "output.line_x0");
  same_vec(p.line_dir, q.line_dir, "output.line_dir"); same_vec(p.pt_obs_outlier, q.pt_obs_outlier, "output.pt_obs_outlier");
  same_vec(p.ln_edge_outlier, q.ln_edge_outlier, "output.ln_edge_outlier"); same_vec(p.line_removed, q.line_removed, "output.line_removed");
  if (std::memcmp(&p.stats, &q.stats, sizeof p.stats) != 0) differ("output.stats", 0);
  if (a.returned_before_optimising != b.returned_before_optimising || a.vToErase.size() != b.vToErase.size() || a.vToEraseLines.size() != b.vToEraseLines.size())
    differ("erase lists", (long)a.vToErase.size());
}

// object -> a number that means the same in both copies
struct Index {
  const Graph& G;
  explicit Index(const Graph& g) : G(g) {}
  int kf(const KeyFrame* k) const { if (!k) return -1; if (k == G.bad_kf) return -2; return G.kf_orig.at(k); }
  int mp(const MapPoint* p) const { if (!p) return -1; if (p == G.bad_mp) return -2; return G.mp_orig.at(p); }
  int ml(const MapLine* l) const { if (!l) return -1; if (l == G.short_ml) return -2; return G.ml_orig.at(l); }
};

void same_graphs(const Graph& A, const Graph& B) {
  const Index ia(A), ib(B);
  for (size_t i = 0; i < A.kf_pool.size(); i++) {
    const KeyFrame &a = A.kf_pool[i], &b = B.kf_pool[i];
    if (ia.kf(&a) != ib.kf(&b) || a.mnId != b.mnId) differ("keyframe placement", (long)i);
    if (std::memcmp(a.Tcw.ptr<float>(), b.Tcw.ptr<float>(), 64) != 0 || a.n_set_pose != b.n_set_pose) differ("keyframe pose", (long)a.mnId);
    if (a.mnBALocalForKF != b.mnBALocalForKF || a.mnBAFixedForKF != b.mnBAFixedForKF) differ("keyframe visit marks", (long)a.mnId);
    if (a.mvpMapPoints.size() != b.mvpMapPoints.size() || a.mvpMapLines.size() != b.mvpMapLines.size()) { differ("keyframe rows", (long)a.mnId); continue; }
    for (size_t j = 0; j < a.mvpMapPoints.size(); j++) if (ia.mp(a.mvpMapPoints[j]) != ib.mp(b.mvpMapPoints[j])) differ("keyframe point matches", (long)a.mnId);
    for (size_t j = 0; j < a.mvpMapLines.size(); j++) if (ia.ml(a.mvpMapLines[j]) != ib.ml(b.mvpMapLines[j])) differ("keyframe line matches", (long)a.mnId);
  }
  for (size_t i = 0; i < A.mp_pool.size(); i++) {
    const MapPoint &a = A.mp_pool[i], &b = B.mp_pool[i];
    if (std::memcmp(a.mWorldPos.ptr<float>(), b.mWorldPos.ptr<float>(), 12) != 0 || a.n_set_pos != b.n_set_pos || a.n_update_normal != b.n_update_normal) differ("point position", (long)i);
    if (a.mnBALocalForKF != b.mnBALocalForKF) differ("point visit mark", (long)i);
    std::map<KeyFrame*, size_t>::const_iterator x = a.mObservations.begin(), y = b.mObservations.begin();
    for (; x != a.mObservations.end() && y != b.mObservations.end(); ++x, ++y) if (ia.kf(x->first) != ib.kf(y->first) || x->second != y->second) differ("point observations", (long)i);
    if (a.mObservations.size() != b.mObservations.size()) differ("point observation count", (long)i);
  }
  for (size_t i = 0; i < A.ml_pool.size(); i++) {
    const MapLine &a = A.ml_pool[i], &b = B.ml_pool[i];
    if (std::memcmp(a.mX0.v, b.mX0.v, 24) != 0 || std::memcmp(a.mDir.v, b.mDir.v, 24) != 0 || a.n_set_pos != b.n_set_pos) differ("line position", (long)i);
    if (a.mnBALocalForKF != b.mnBALocalForKF) differ("line visit mark", (long)i);
    std::map<KeyFrame*, size_t>::const_iterator x = a.mObservations.begin(), y = b.mObservations.begin();
    for (; x != a.mObservations.end() && y != b.mObservations.end(); ++x, ++y) if (ia.kf(x->first) != ib.kf(y->first) || x->second != y->second) differ("line observations", (long)i);
    if (a.mObservations.size() != b.mObservations.size()) differ("line observation count", (long)i);
  }
}

void reset_marks(Graph& G) {
  for (size_t i = 0; i < G.kf_pool.size(); i++) G.kf_pool[i].mnBALocalForKF = G.kf_pool[i].mnBAFixedForKF = 0;
  for (size_t i = 0; i < G.mp_pool.size(); i++) G.mp_pool[i].mnBALocalForKF = 0;
  for (size_t i = 0; i < G.ml_pool.size(); i++) G.ml_pool[i].mnBALocalForKF = 0;
}

struct Pair {                                  // the two copies, the host adapter's map and the mirrored one
  Graph A, B; Map mapA, mapB;
  Pair(const Problem& P, unsigned seed) {
    const lba_graph::OddIds odd = small_ids(P.w);
    std::mt19937 ra(seed), rb(seed);
    A.build(P.w, P.camg, ra, odd); B.build(P.w, P.camg, rb, odd);
    fill_map(A, mapA); fill_map(B, mapB);
  }
};

int run_check(const char* in, unsigned seed) {
  Problem P; read_problem(in, P);
  Pair G(P, seed);
  same_graphs(G.A, G.B);
  if (diffs) { std::fprintf(stderr, "map_ba_harness: the two copies differ before any call\n"); return 2; }
  KeyFrame* pa[2] = {G.A.pKF, second_pkf(G.A)}; KeyFrame* pb[2] = {G.B.pKF, second_pkf(G.B)};
  lld_amd::Context ctx(0);
  lld_adapter::MapOnDevice M(ctx.get(), limits_for(G.B, P.w));
  M.EnableBundleAdjustment();
  M.Upload(&G.mapB);
  for (int call = 0; call < 2; call++) {
    if (!pa[call] || !pb[call]) { std::fprintf(stderr, "map_ba_harness: no second pKF\n"); return 1; }
    bool stopA = false, stopB = false;
    lld_adapter::LbaTrace ta, tb;
    lld_adapter::LocalBundleAdjustment(ctx.get(), pa[call], &stopA, &G.mapA, P.camg[5], &ta);
    M.LocalBundleAdjustment(pb[call], &stopB, &G.mapB, P.camg[5], &tb);
    same_traces(ta, tb);
    same_graphs(G.A, G.B);
    int addr_inversions = 0;
    for (size_t i = 1; i < tb.cams.size(); i++) if ((tb.cams[i] < tb.cams[i - 1]) != (tb.cams[i]->mnId < tb.cams[i - 1]->mnId)) addr_inversions++;
    std::printf("call %d: pKF %lu, %d cameras (%d free), %d points, %d point observations, %d lines, %d line observations; chi2 %.9g -> %.9g; %zu + %zu erased; "
                "%d address inversions; bad keyframe marked fixed %d\n", call, pb[call]->mnId, tb.window.n_cams(), tb.window.n_free_cams, tb.window.n_points(),
                (int)tb.window.pt_obs_cam.size(), tb.window.n_lines(), (int)tb.window.ln_obs_cam.size(), tb.output.stats.chi2_round1, tb.output.stats.chi2_final,
                tb.vToErase.size(), tb.vToEraseLines.size(), addr_inversions, (int)(G.B.bad_kf->mnBAFixedForKF == pb[call]->mnId));
  }
  std::printf("differences %d\n", diffs);
  return diffs ? 2 : 0;
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

int run_time(const char* in, int reps, unsigned seed) {
  Problem P; read_problem(in, P);
  Pair G(P, seed);
  lld_amd::Context ctx(0);
  lld_adapter::MapOnDevice M(ctx.get(), limits_for(G.B, P.w));
  M.EnableBundleAdjustment();
  M.Upload(&G.mapB);
  lld_adapter::LbaTrace shape;
  std::vector<double> t[2][2];                 // [stop raised, lowered][host, map]
  for (int whole = 0; whole < 2; whole++)
    for (int r = -3; r < reps; r++) {           // three warm-up rounds
      for (int k = 0; k < 2; k++) {
        const bool map_route = ((r + 3 + k) & 1) != 0;      // the order of the two routes alternates
        Graph& g = map_route ? G.B : G.A;
        reset_marks(g);
        bool stop = !whole;
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        if (map_route) M.LocalBundleAdjustment(g.pKF, &stop, &G.mapB, P.camg[5], nullptr);
        else lld_adapter::LocalBundleAdjustment(ctx.get(), g.pKF, &stop, &G.mapA, P.camg[5], nullptr);
        const double ms = ms_since(t0);
        if (r >= 0) t[whole][map_route ? 1 : 0].push_back(ms);
      }
      if (whole == 0 && r == -3) { bool stop = true; reset_marks(G.B); M.LocalBundleAdjustment(G.B.pKF, &stop, &G.mapB, P.camg[5], &shape); }
    }
  same_graphs(G.A, G.B);                         // both routes took the graph to the same place
  const char* names[2][2] = {{"assembly_host_ms", "assembly_map_ms"}, {"whole_host_ms", "whole_map_ms"}};
  std::printf("{\"n_cams\": %d, \"n_free_cams\": %d, \"n_points\": %d, \"n_pt_obs\": %d, \"n_lines\": %d, \"n_ln_obs\": %d, \"graph_differences\": %d", shape.window.n_cams(),
              shape.window.n_free_cams, shape.window.n_points(), (int)shape.window.pt_obs_cam.size(), shape.window.n_lines(), (int)shape.window.ln_obs_cam.size(), diffs);
  for (int whole = 0; whole < 2; whole++)
    for (int k = 0; k < 2; k++) {
      std::printf(", \"%s\": [", names[whole][k]);
      for (size_t i = 0; i < t[whole][k].size(); i++) std::printf("%s%.4f", i ? ", " : "", t[whole][k][i]);
      std::printf("]");
    }
  std::printf("}\n");
  return 0;
}

// ---- apply: flat tables through include/lld_amd.hpp
void upload_scene(lld_amd::DeviceMap& map, const map_ba_apply_scene::Scene& S) {
  const map_ba_apply_host::Map& M = S.M;
  lld_amd::DeviceMap::KeyFrameRows k; lld_amd::DeviceMap::KeyFrameFeatures f;
  std::vector<int32_t> kp_slot, kp_start(1, 0), kp_oct; std::vector<float> kp_depth, kp_th;
  k.cov_start.assign(1, 0); k.child_start.assign(1, 0); k.point_start.assign(1, 0); k.line_start.assign(1, 0);
  for (int s = 0; s < M.n_kf; s++) {
    if (!S.kf_set[s]) continue;
    k.slot.push_back(s); k.order_key.push_back(S.kf_key[s]); k.bad.push_back(S.kf_bad[s]); k.parent.push_back(-1);
    k.cov_start.push_back(0); k.child_start.push_back(0);
    k.point.insert(k.point.end(), S.kp_point.begin() + S.kp_start[s], S.kp_point.begin() + S.kp_start[s + 1]); k.point_start.push_back((int32_t)k.point.size());
    k.line.insert(k.line.end(), S.kl_line.begin() + S.kl_start[s], S.kl_line.begin() + S.kl_start[s + 1]); k.line_start.push_back((int32_t)k.line.size());
    if (S.kf_has_keypoints[s]) {
      kp_slot.push_back(s); kp_oct.insert(kp_oct.end(), S.kp_octave.begin() + S.kp_start[s], S.kp_octave.begin() + S.kp_start[s + 1]);
      kp_start.push_back((int32_t)kp_oct.size()); kp_th.push_back(0.f);
    }
    if (M.kf_feat[s]) {
      f.slot.push_back(s); f.mn_id.push_back(S.kf_mn_id[s]); f.Tcw.insert(f.Tcw.end(), M.kf_tcw.begin() + 16 * (size_t)s, M.kf_tcw.begin() + 16 * (size_t)s + 16);
      f.kp_uvr.insert(f.kp_uvr.end(), S.kp_uvr.begin() + 3 * (size_t)S.kp_start[s], S.kp_uvr.begin() + 3 * (size_t)S.kp_start[s + 1]); f.kp_start.push_back((int32_t)(f.kp_uvr.size() / 3));
      f.kl_left.insert(f.kl_left.end(), S.kl_left.begin() + 4 * (size_t)S.kl_start[s], S.kl_left.begin() + 4 * (size_t)S.kl_start[s + 1]);
      f.kl_right.insert(f.kl_right.end(), S.kl_right.begin() + 4 * (size_t)S.kl_start[s], S.kl_right.begin() + 4 * (size_t)S.kl_start[s + 1]);
      f.kl_octave.insert(f.kl_octave.end(), S.kl_octave.begin() + 2 * (size_t)S.kl_start[s], S.kl_octave.begin() + 2 * (size_t)S.kl_start[s + 1]);
      f.kl_start.push_back((int32_t)(f.kl_left.size() / 4));
    }
  }
  kp_depth.assign(kp_oct.size(), 0.f);
  map.SetKeyFrames(k);
  if (!kp_slot.empty()) map.SetKeyFrameKeypoints(kp_slot, kp_start, kp_oct, kp_depth, kp_th);
  if (!f.slot.empty()) map.SetKeyFrameFeatures(f);
  std::vector<int32_t> ps, pstart(1, 0), pkf, pidx, pn, pref; std::vector<float> pos, nrm, mind, maxd; std::vector<uint8_t> pbad;
  for (int s = 0; s < M.n_pt; s++) {
    if (!M.pt_state[s]) continue;
    ps.push_back(s); pbad.push_back(M.pt_state[s] == 2); pn.push_back(M.pt_nobs[s]); pref.push_back(M.pt_ref[s]); mind.push_back(M.pt_mind[s]); maxd.push_back(M.pt_maxd[s]);
    for (int c = 0; c < 3; c++) { pos.push_back(M.pt_pos[3 * (size_t)s + c]); nrm.push_back(M.pt_nrm[3 * (size_t)s + c]); }
    pkf.insert(pkf.end(), M.pt_obs_kf[s].begin(), M.pt_obs_kf[s].end()); pidx.insert(pidx.end(), M.pt_obs_idx[s].begin(), M.pt_obs_idx[s].end());
    pstart.push_back((int32_t)pkf.size());
  }
  if (!ps.empty()) {
    const std::vector<uint32_t> desc(8 * ps.size(), 0u);
    map.SetPoints(ps, pos.data(), nrm.data(), mind.data(), maxd.data(), desc.data(), pbad.data());
    map.SetObservationsIndexed(ps, pstart, pkf, pidx, pn);
    if (M.has_refs) map.SetPointRefs(ps, pref);
  }
  std::vector<int32_t> ls, os, ostart(1, 0), okf, oidx, on; std::vector<double> x0, dir, x2; std::vector<uint8_t> lbad;
  for (int s = 0; s < M.n_ln; s++) {
    if (!S.ln_set[s]) continue;
    ls.push_back(s); lbad.push_back(M.ln_bad[s]);
    for (int c = 0; c < 3; c++) { x0.push_back(M.ln_x0[3 * (size_t)s + c]); dir.push_back(M.ln_dir[3 * (size_t)s + c]); x2.push_back(x0.back() + dir.back()); }
    if (!S.ln_has_row[s]) continue;
    os.push_back(s); on.push_back(M.ln_nobs[s]);
    okf.insert(okf.end(), M.ln_obs_kf[s].begin(), M.ln_obs_kf[s].end()); oidx.insert(oidx.end(), M.ln_obs_idx[s].begin(), M.ln_obs_idx[s].end());
    ostart.push_back((int32_t)okf.size());
  }
  if (!ls.empty()) {
    const std::vector<float> desc((size_t)map.limits().line_dim * ls.size(), 0.f);
    map.SetLines(ls, x0.data(), dir.data(), x0.data(), x2.data(), desc.data(), lbad.data());
  }
  if (!os.empty()) map.SetLineObservations(os, ostart, okf, oidx, on);
}

int run_apply(const char* scene, const char* answer, bool solve) {
  using namespace map_ba_apply_scene;
  Scene S; read_scene(scene, S);
  lld_map_limits L;
  int32_t* lp = &L.max_keyframes;
  for (int k = 0; k < 10; k++) lp[k] = S.limits[k];
  lld_camera cam; cam.fx = S.cam[0]; cam.fy = S.cam[1]; cam.cx = S.cam[2]; cam.cy = S.cam[3]; cam.bf = S.cam[4];
  lld_amd::Context ctx(0);
  lld_amd::DeviceMap map(ctx, L);
  upload_scene(map, S);
  lld_ba_result res{};
  int counts[5];
  const map_ba_apply_host::Window& W = S.W;
  if (solve) {
    lld_amd::DeviceMap::LocalBaResult r = map.LocalBa(S.query, cam, S.sigma2);
    if (r.ids.status) { std::fprintf(stderr, "map_ba_harness: window status %d\n", r.ids.status); return 2; }
    const lld_ba_window& w = r.ids.window;
    if (w.n_cams != S.hdr[4] || w.n_points != S.hdr[6] || w.n_pt_obs != S.hdr[7] || w.n_lines != S.hdr[8] || w.n_ln_obs != S.hdr[9] || r.ids.n_local_cams != W.n_local ||
        std::memcmp(r.ids.cam_slot, W.cam_slot.data(), 4 * W.cam_slot.size()) || std::memcmp(r.ids.point_slot, W.point_slot.data(), 4 * W.point_slot.size()) ||
        std::memcmp(w.pt_obs_cam, W.pt_obs_cam.data(), 4 * W.pt_obs_cam.size()) || std::memcmp(w.ln_obs_cam, W.ln_obs_cam.data(), 4 * W.ln_obs_cam.size())) {
      std::fprintf(stderr, "map_ba_harness: the window is not the scene's\n"); return 2;
    }
    res = r.result;
    File rf((std::string(answer) + ".result").c_str(), "wb");
    rf.put(res.cam_qt, 7 * (size_t)w.n_cams); rf.put(res.pt_xyz, 3 * (size_t)w.n_points); rf.put(res.line_x0, 3 * (size_t)w.n_lines); rf.put(res.line_dir, 3 * (size_t)w.n_lines);
    rf.put(res.pt_obs_outlier, (size_t)w.n_pt_obs); rf.put(res.ln_edge_outlier, 2 * (size_t)w.n_ln_obs); rf.put(res.line_removed, (size_t)w.n_lines);
  } else {
    lld_amd::DeviceMap::BaWindowResult bw = map.BaWindow(S.query, cam, S.sigma2);
    if (bw.status || bw.cam_slot != W.cam_slot || bw.point_slot != W.point_slot || bw.window.pt_obs_start != W.pt_obs_start || bw.window.pt_obs_cam != W.pt_obs_cam ||
        bw.line_slot != W.line_slot || bw.window.ln_obs_start != W.ln_obs_start || bw.window.ln_obs_cam != W.ln_obs_cam || bw.n_local_cams != W.n_local) {
      std::fprintf(stderr, "map_ba_harness: the window is not the scene's (status %d)\n", bw.status); return 2;
    }
    res.cam_qt = S.cam_qt.data(); res.pt_xyz = S.R.pt_xyz.data(); res.line_x0 = S.R.line_x0.data(); res.line_dir = S.R.line_dir.data();
    res.pt_obs_outlier = S.R.pt_obs_outlier.data(); res.ln_edge_outlier = S.R.ln_edge_outlier.data(); res.line_removed = S.R.line_removed.data();
  }
  for (int k = 0; k < 5; k++) counts[k] = S.hdr[k == 0 ? 4 : 5 + k];
  const lld_amd::DeviceMap::ApplyResult a = map.ApplyLocalBa(res, counts[0], counts[1], counts[2], counts[3], counts[4], S.R.level_scale);
  File w(answer, "wb");
  const int32_t c6[6] = {a.n_local_cams, a.n_pt_obs_erased, a.n_ln_obs_erased, a.n_points_bad, a.n_lines_bad, a.n_index_skipped};
  w.put(c6, 6); w.put(a.tcw); w.put(a.ow); w.put(a.pt_pos); w.put(a.pt_normal); w.put(a.pt_min_distance); w.put(a.pt_max_distance); w.put(a.pt_n_obs); w.put(a.pt_ref_kf);
  w.put(a.pt_row_len); w.put(a.pt_flags); w.put(a.ln_bad); w.put(a.ln_n_obs); w.put(a.ln_row_len);
  const int kinds[6] = {LLD_MAP_ROWS_POINT_OBS, LLD_MAP_ROWS_POINT_IDX, LLD_MAP_ROWS_KF_POINTS, LLD_MAP_ROWS_KF_LINES, LLD_MAP_ROWS_LINE_OBS, LLD_MAP_ROWS_LINE_IDX};
  const int sizes[6] = {L.max_points, L.max_points, L.max_keyframes, L.max_keyframes, L.max_lines, L.max_lines};
  for (int k = 0; k < 6; k++) {
    std::vector<int32_t> slots(sizes[k]);
    for (int s = 0; s < sizes[k]; s++) slots[s] = s;
    const lld_amd::DeviceMap::Rows rows = map.DownloadRows(kinds[k], slots);
    put_rows(w, rows.start, rows.data);
  }
  std::printf("applied: %d + %d observations erased, %d points and %d lines gone bad, %d indices skipped\n", a.n_pt_obs_erased, a.n_ln_obs_erased, a.n_points_bad, a.n_lines_bad,
              a.n_index_skipped);
  return 0;
}

// route B's push-back: what the host tail changed goes through the setters, whole rows as they take them
void push_changed(lld_amd::DeviceMap& map, const map_ba_apply_scene::Scene& S, const map_ba_apply_host::Map& M, const map_ba_apply_host::Out& O, const std::vector<float>& tcw) {
  const map_ba_apply_host::Window& W = S.W;
  if (!O.changed_kf_rows.empty()) {                                   // keyframes that lost a match: the rows travel, features and keypoints stay
    lld_amd::DeviceMap::KeyFrameRows k;
    k.cov_start.assign(1, 0); k.child_start.assign(1, 0); k.point_start.assign(1, 0); k.line_start.assign(1, 0);
    for (size_t i = 0; i < O.changed_kf_rows.size(); i++) {
      const int s = O.changed_kf_rows[i];
      k.slot.push_back(s); k.order_key.push_back(S.kf_key[s]); k.bad.push_back(S.kf_bad[s]); k.parent.push_back(-1); k.cov_start.push_back(0); k.child_start.push_back(0);
      k.point.insert(k.point.end(), M.kf_points[s].begin(), M.kf_points[s].end()); k.point_start.push_back((int32_t)k.point.size());
      k.line.insert(k.line.end(), M.kf_lines[s].begin(), M.kf_lines[s].end()); k.line_start.push_back((int32_t)k.line.size());
    }
    map.SetKeyFrames(k);
  }
  map.SetKeyFramePoses(std::vector<int32_t>(W.cam_slot.begin(), W.cam_slot.begin() + W.n_local), tcw);
  const std::vector<int32_t>& P = W.point_slot;
  if (!P.empty()) {                                                   // every window point moved: position, normal, distances, bad flag (and its descriptor with them)
    std::vector<float> pos, nrm, mind, maxd; std::vector<uint8_t> bad;
    for (size_t q = 0; q < P.size(); q++) {
      const int s = P[q];
      for (int c = 0; c < 3; c++) { pos.push_back(M.pt_pos[3 * (size_t)s + c]); nrm.push_back(M.pt_nrm[3 * (size_t)s + c]); }
      mind.push_back(M.pt_mind[s]); maxd.push_back(M.pt_maxd[s]); bad.push_back(M.pt_state[s] == 2);
    }
    const std::vector<uint32_t> desc(8 * P.size(), 0u);
    map.SetPoints(P, pos.data(), nrm.data(), mind.data(), maxd.data(), desc.data(), bad.data());
  }
  if (!O.changed_pt_rows.empty()) {
    std::vector<int32_t> start(1, 0), kf, idx, n, ref;
    for (size_t i = 0; i < O.changed_pt_rows.size(); i++) {
      const int s = O.changed_pt_rows[i];
      kf.insert(kf.end(), M.pt_obs_kf[s].begin(), M.pt_obs_kf[s].end()); idx.insert(idx.end(), M.pt_obs_idx[s].begin(), M.pt_obs_idx[s].end());
      start.push_back((int32_t)kf.size()); n.push_back(M.pt_nobs[s]); ref.push_back(M.pt_ref[s]);
    }
    map.SetObservationsIndexed(O.changed_pt_rows, start, kf, idx, n);
    if (M.has_refs) map.SetPointRefs(O.changed_pt_rows, ref);
  }
  std::vector<int32_t> ls; std::vector<double> x0, dir, x2; std::vector<uint8_t> lbad;
  for (size_t l = 0; l < W.line_slot.size(); l++) {
    if (S.R.line_removed[l]) continue;
    const int s = W.line_slot[l];
    ls.push_back(s); lbad.push_back(M.ln_bad[s]);
    for (int c = 0; c < 3; c++) { x0.push_back(M.ln_x0[3 * (size_t)s + c]); dir.push_back(M.ln_dir[3 * (size_t)s + c]); x2.push_back(x0.back() + dir.back()); }
  }
  if (!ls.empty()) {
    const std::vector<float> desc((size_t)map.limits().line_dim * ls.size(), 0.f);
    map.SetLines(ls, x0.data(), dir.data(), x0.data(), x2.data(), desc.data(), lbad.data());
  }
  if (!O.changed_ln_rows.empty()) {
    std::vector<int32_t> start(1, 0), kf, idx, n;
    for (size_t i = 0; i < O.changed_ln_rows.size(); i++) {
      const int s = O.changed_ln_rows[i];
      kf.insert(kf.end(), M.ln_obs_kf[s].begin(), M.ln_obs_kf[s].end()); idx.insert(idx.end(), M.ln_obs_idx[s].begin(), M.ln_obs_idx[s].end());
      start.push_back((int32_t)kf.size()); n.push_back(M.ln_nobs[s]);
    }
    map.SetLineObservations(O.changed_ln_rows, start, kf, idx, n);
  }
}

#define HIP_OK(x) do { if ((x) != hipSuccess) throw std::runtime_error("HIP call failed: " #x); } while (0)

int run_apply_time(const char* scene, int reps) {
  using namespace map_ba_apply_scene;
  Scene S; read_scene(scene, S);
  lld_map_limits L;
  int32_t* lp = &L.max_keyframes;
  for (int k = 0; k < 10; k++) lp[k] = S.limits[k];
  lld_camera cam; cam.fx = S.cam[0]; cam.fy = S.cam[1]; cam.cx = S.cam[2]; cam.cy = S.cam[3]; cam.bf = S.cam[4];
  lld_amd::Context ctx(0);
  lld_amd::DeviceMap map(ctx, L);
  upload_scene(map, S);
  const map_ba_apply_host::Window& W = S.W;
  // one solve, untimed: both routes get its result
  const size_t nc = S.hdr[4], np = S.hdr[6], npo = S.hdr[7], nl = S.hdr[8], nlo = S.hdr[9];
  {
    lld_amd::DeviceMap::LocalBaResult r = map.LocalBa(S.query, cam, S.sigma2);
    const lld_ba_window& w = r.ids.window;
    if (r.ids.status || (size_t)w.n_cams != nc || (size_t)w.n_points != np || (size_t)w.n_pt_obs != npo || (size_t)w.n_lines != nl || (size_t)w.n_ln_obs != nlo ||
        std::memcmp(r.ids.point_slot, W.point_slot.data(), 4 * np) || std::memcmp(w.pt_obs_cam, W.pt_obs_cam.data(), 4 * npo)) {
      std::fprintf(stderr, "map_ba_harness: the window is not the scene's\n"); return 2;
    }
    S.cam_qt.assign(r.result.cam_qt, r.result.cam_qt + 7 * nc); S.R.pt_xyz.assign(r.result.pt_xyz, r.result.pt_xyz + 3 * np);
    S.R.line_x0.assign(r.result.line_x0, r.result.line_x0 + 3 * nl); S.R.line_dir.assign(r.result.line_dir, r.result.line_dir + 3 * nl);
    S.R.pt_obs_outlier.assign(r.result.pt_obs_outlier, r.result.pt_obs_outlier + npo); S.R.ln_edge_outlier.assign(r.result.ln_edge_outlier, r.result.ln_edge_outlier + 2 * nlo);
    S.R.line_removed.assign(r.result.line_removed, r.result.line_removed + nl);
  }
  lld_ba_result res{};
  res.cam_qt = S.cam_qt.data(); res.pt_xyz = S.R.pt_xyz.data(); res.line_x0 = S.R.line_x0.data(); res.line_dir = S.R.line_dir.data();
  res.pt_obs_outlier = S.R.pt_obs_outlier.data(); res.ln_edge_outlier = S.R.ln_edge_outlier.data(); res.line_removed = S.R.line_removed.data();
  hipStream_t sm = reinterpret_cast<hipStream_t>(lld_ctx_stream(ctx.get()));
  hipEvent_t e0, e1; HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
  std::vector<double> t[2];
  int erased[2] = {0, 0}, bad[2] = {0, 0};
  for (int r = -3; r < reps; r++)
    for (int k = 0; k < 2; k++) {
      const int route = (r + 3 + k) & 1;                              // the order of the two routes alternates
      map.Clear(); upload_scene(map, S);                              // untimed: every repetition meets the same map ...
      map.BaWindow(S.query, cam, S.sigma2);                           // ... and the window staged
      map_ba_apply_host::Map M = S.M;
      HIP_OK(hipStreamSynchronize(sm));
      HIP_OK(hipEventRecord(e0, sm));
      if (route == 0) {
        const lld_amd::DeviceMap::ApplyResult a = map.ApplyLocalBa(res, (int)nc, (int)np, (int)npo, (int)nl, (int)nlo, S.R.level_scale);
        erased[0] = a.n_pt_obs_erased + a.n_ln_obs_erased; bad[0] = a.n_points_bad + a.n_lines_bad;
      } else {
        map_ba_apply_host::Result R = S.R;
        R.tcw.assign(16 * (size_t)W.n_local, 0.f);
        for (int c = 0; c < W.n_local; c++) lld_se3_to_tcw_f32(S.cam_qt.data() + 7 * (size_t)c, &R.tcw[16 * (size_t)c]);
        map_ba_apply_host::Out O;
        map_ba_apply_host::apply(M, W, R, O);
        push_changed(map, S, M, O, R.tcw);
        erased[1] = O.n_pt_obs_erased + O.n_ln_obs_erased; bad[1] = O.n_points_bad + O.n_lines_bad;
      }
      HIP_OK(hipEventRecord(e1, sm));
      HIP_OK(hipEventSynchronize(e1));
      float ms = 0.f; HIP_OK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 0) t[route].push_back(ms);
    }
  HIP_OK(hipEventDestroy(e0)); HIP_OK(hipEventDestroy(e1));
  std::printf("{\"n_cams\": %zu, \"n_local_cams\": %d, \"n_points\": %zu, \"n_pt_obs\": %zu, \"n_lines\": %zu, \"n_ln_obs\": %zu, \"erased\": [%d, %d], \"gone_bad\": [%d, %d]", nc, W.n_local, np,
              npo, nl, nlo, erased[0], erased[1], bad[0], bad[1]);
  const char* names[2] = {"apply_ms", "host_tail_and_setters_ms"};
  for (int k = 0; k < 2; k++) {
    std::printf(", \"%s\": [", names[k]);
    for (size_t i = 0; i < t[k].size(); i++) std::printf("%s%.4f", i ? ", " : "", t[k][i]);
    std::printf("]");
  }
  std::printf("}\n");
  return erased[0] == erased[1] && bad[0] == bad[1] ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc >= 3 && std::string(argv[1]) == "check") return run_check(argv[2], argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    if (argc >= 4 && std::string(argv[1]) == "time") return run_time(argv[2], std::atoi(argv[3]), argc > 4 ? (unsigned)std::atoi(argv[4]) : 1u);
    if (argc >= 4 && std::string(argv[1]) == "apply_time") return run_apply_time(argv[2], std::atoi(argv[3]));
    if (argc >= 4 && std::string(argv[1]) == "apply") return run_apply(argv[2], argv[3], argc > 4 && std::string(argv[4]) == "solve");
    std::fprintf(stderr, "usage: map_ba_harness check <in> [seed] | time <in> <reps> [seed] | apply <scene> <answer> [solve] | apply_time <scene> <reps>\n");
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "map_ba_harness: %s\n", e.what());
    return 1;
  }
}
