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
// Input files are the ones examples/harness.cpp reads in `ba` mode.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../adapters/lld_map_adapter.h"
#include "lba_graph.h"

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

}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc >= 3 && std::string(argv[1]) == "check") return run_check(argv[2], argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    if (argc >= 4 && std::string(argv[1]) == "time") return run_time(argv[2], std::atoi(argv[3]), argc > 4 ? (unsigned)std::atoi(argv[4]) : 1u);
    std::fprintf(stderr, "usage: map_ba_harness check <in> [seed] | time <in> <reps> [seed]\n");
    return 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "map_ba_harness: %s\n", e.what());
    return 1;
  }
}
