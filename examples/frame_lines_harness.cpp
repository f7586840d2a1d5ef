// frame_lines_harness.cpp — the stereo Frame's lines matched on the device and MatchLinesLastKF between two resident frames, from compiled C++, twice:
//   1. over include/lld_amd.hpp: TrackedFrame::BuildLines / DownloadLines on two frames, SetState, MatchLinesLastKF on the pair, then TrackLocalMap
//      (an empty local map) + Download on the current frame, whose stage-2 record shows the created lines as the chain sees them;
//   2. through adapters/lld_tracking_adapter.cc on live Frame / KeyFrame / MapLine / Map test doubles: the FrameOnDevice constructor that takes
//      TwoFrameLineMatcher's parameters (against lld_adapter::TwoFrameLineMatcher::MatchLines on the host arrays) and FrameOnDevice::MatchLinesLastKF
//      (against lld_adapter::MatchLinesLastKF on an identical second object graph).
// usage: frame_lines_harness <scene.bin> <out.bin>; the layouts are those of tests/frame_lines_scenes.py write_pair_scene / read_pair_result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "../adapters/lld_line_adapter.h"
#include "../adapters/lld_tracking_adapter.h"
#include "../include/lld_amd.hpp"

using namespace lld_slam;

namespace {

template <class T> std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n + 1);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short scene file\n"); std::exit(2); }
  v.resize(n);
  return v;
}
template <class T> void wr(FILE* f, const T* p, size_t n) { if (n) std::fwrite(p, sizeof(T), n, f); }
void wr_ints(FILE* f, const std::vector<int>& v) { std::vector<int32_t> w(v.begin(), v.end()); wr(f, w.data(), w.size()); }

struct LineFrame {               // one frame of the scene file
  int nl, nr;
  std::vector<float> left, dl, right, dr, Tcw; std::vector<int32_t> lo, ro, id, id_adapter, tracked; std::vector<double> x0, dir, T_wc;
  lld_frame_view view;
  void read(FILE* in, int nl_, int nr_, int dim) {
    nl = nl_; nr = nr_;
    left = rd<float>(in, (size_t)nl * 4); lo = rd<int32_t>(in, nl); dl = rd<float>(in, (size_t)nl * dim);
    right = rd<float>(in, (size_t)nr * 4); ro = rd<int32_t>(in, nr); dr = rd<float>(in, (size_t)nr * dim);
    { const std::vector<char> b = rd<char>(in, sizeof view); std::memcpy(&view, b.data(), sizeof view); }
    Tcw = rd<float>(in, 16); T_wc = rd<double>(in, 16);
    id = rd<int32_t>(in, nl); id_adapter = rd<int32_t>(in, nl); x0 = rd<double>(in, (size_t)nl * 3); dir = rd<double>(in, (size_t)nl * 3);
    const int nt = rd<int32_t>(in, 1)[0];
    tracked = rd<int32_t>(in, nt);
  }
};

std::vector<KeyLine> key_lines(const std::vector<float>& seg, const std::vector<int32_t>& oct) {
  std::vector<KeyLine> kl(oct.size());
  for (size_t i = 0; i < oct.size(); i++) { kl[i].startPointX = seg[4 * i]; kl[i].startPointY = seg[4 * i + 1]; kl[i].endPointX = seg[4 * i + 2]; kl[i].endPointY = seg[4 * i + 3]; kl[i].octave = oct[i]; }
  return kl;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: frame_lines_harness <scene.bin> <out.bin>\n"); return 2; }
  try {
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(in, 8);
    const int nt = hd[0], nlev = hd[1], dim = hd[6], first_new_id = hd[7];
    const std::vector<float> bounds = rd<float>(in, 6), scale = rd<float>(in, nlev), sigma2 = rd<float>(in, nlev), inv_sigma2 = rd<float>(in, nlev);
    const std::vector<double> cam = rd<double>(in, 5), stereo = rd<double>(in, 12);     // fx fy cx cy bf; K[9] b tau minLineLength
    const std::vector<uint32_t> fdesc = rd<uint32_t>(in, (size_t)nt * 8);
    const std::vector<float> fxy = rd<float>(in, (size_t)nt * 2); const std::vector<int32_t> foct = rd<int32_t>(in, nt);
    const std::vector<float> fur = rd<float>(in, nt), fang = rd<float>(in, nt);
    LineFrame C, L;
    C.read(in, hd[2], hd[3], dim); L.read(in, hd[4], hd[5], dim);
    std::fclose(in);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    lld_amd::Context ctx(0);

    // ---------------------------------------------------------------- 1. include/lld_amd.hpp
    {
      lld_orb_search kp; std::memset(&kp, 0, sizeof kp);
      kp.nt = nt; kp.t_desc = fdesc.data(); kp.t_xy = fxy.data(); kp.t_octave = foct.data(); kp.t_uright = fur.data(); kp.t_angle = fang.data();
      kp.grid_min_x = bounds[0]; kp.grid_min_y = bounds[1]; kp.grid_width_inv = bounds[4]; kp.grid_height_inv = bounds[5]; kp.grid_cols = 64; kp.grid_rows = 48;
      kp.n_levels = nlev; kp.level_scale = scale.data(); kp.level_sigma2 = sigma2.data(); kp.level_inv_sigma2 = inv_sigma2.data();
      lld_amd::TrackedFrame cur(ctx, kp, nullptr), last(ctx, kp, nullptr);
      const std::vector<int32_t> no_point(nt + 1, -1); const std::vector<float> no_pos(3 * (size_t)nt + 3, 0.f);
      auto enter = [&](lld_amd::TrackedFrame& tf, const LineFrame& F) {
        lld_frame_lines_build b; std::memset(&b, 0, sizeof b);
        b.n_left = F.nl; b.left = F.left.data(); b.left_octave = F.lo.data(); b.desc_left = F.dl.data();
        b.n_right = F.nr; b.right = F.right.data(); b.right_octave = F.ro.data(); b.desc_right = F.dr.data();
        b.dim = dim; b.sx = 1.0 / bounds[2]; b.sy = 1.0 / bounds[3];
        for (int i = 0; i < 9; i++) b.stereo.K[i] = stereo[i];
        b.stereo.b = stereo[9]; b.stereo.tau = stereo[10]; b.stereo.min_line_length = (int32_t)stereo[11]; b.stereo.is_stereo = 1;
        tf.params.cam = lld_camera{cam[0], cam[1], cam[2], cam[3], cam[4]};
        tf.BuildLines(&b);
        lld_frame_held held; std::memset(&held, 0, sizeof held);
        held.kp_point_id = no_point.data(); held.kp_world_pos = no_pos.data();
        held.ln_line_id = F.id.data(); held.ln_x0 = F.x0.data(); held.ln_dir = F.dir.data();
        held.n_tracked = (int32_t)F.tracked.size(); held.tracked_line_id = F.tracked.empty() ? nullptr : F.tracked.data();
        tf.SetState(F.view, F.Tcw.data(), held);                            // (queued behind the build: nothing waited in between)
      };
      enter(cur, C); enter(last, L);
      std::vector<int> lm;
      cur.DownloadLines(&lm); wr_ints(out, lm);
      last.DownloadLines(&lm); wr_ints(out, lm);
      lld_amd::TrackedFrame::NewMapLines R;
      const int32_t ret = cur.MatchLinesLastKF(last, first_new_id, &R);
      const int32_t cnt[3] = {R.r.n_created, R.r.n_held, ret};
      wr(out, cnt, 3); wr(out, R.match_last.data(), C.nl); wr(out, R.new_id.data(), C.nl); wr(out, R.created.data(), C.nl);
      lld_map_points none; std::memset(&none, 0, sizeof none);
      cur.TrackLocalMap(none, nullptr, nullptr);
      lld_amd::TrackRecord r2;
      cur.Download(nullptr, &r2);
      wr(out, r2.ln_line_id.data(), C.nl);
    }

    // ---------------------------------------------------------------- 2. the adapters on live objects
    struct Graph {
      Frame Cur, Last; KeyFrame KF; Map map;
      std::map<int32_t, std::unique_ptr<MapLine> > lines; std::vector<std::unique_ptr<MapLine> > made;
    };
    auto frame_of = [&](Frame& F, const LineFrame& S, unsigned long id) {
      F.N = nt; F.mnId = id; F.fx = (float)cam[0]; F.fy = (float)cam[1]; F.cx = (float)cam[2]; F.cy = (float)cam[3]; F.mbf = (float)cam[4]; F.mb = F.mbf / F.fx;
      F.mvKeysUn.resize(nt);
      for (int k = 0; k < nt; k++) { F.mvKeysUn[k].pt.x = fxy[2 * k]; F.mvKeysUn[k].pt.y = fxy[2 * k + 1]; F.mvKeysUn[k].octave = foct[k]; F.mvKeysUn[k].angle = fang[k]; }
      F.mvKeys = F.mvKeysUn; F.mvuRight = fur; F.mvInvLevelSigma2 = inv_sigma2; F.mvScaleFactors = scale; F.mvLevelSigma2 = sigma2;
      F.mvpMapPoints.assign(nt, nullptr); F.mvbOutlier.assign(nt, false);
      F.mDescriptors = MatU8(nt, 32);
      if (nt) std::memcpy(F.mDescriptors.ptr<unsigned char>(), fdesc.data(), (size_t)nt * 32);
      F.mnMinX = bounds[0]; F.mnMinY = bounds[1]; F.mnMaxX = bounds[2]; F.mnMaxY = bounds[3]; F.mfGridElementWidthInv = bounds[4]; F.mfGridElementHeightInv = bounds[5];
      F.mnScaleLevels = nlev; F.mfScaleFactor = nlev > 1 ? scale[1] : 1.f; F.mfLogScaleFactor = S.view.log_scale_factor;
      F.mvLinesLeft = key_lines(S.left, S.lo); F.mvLinesRight = key_lines(S.right, S.ro);
      F.mDescriptorsLines = Mat(S.nl, dim, S.dl.data()); F.mDescriptorsLinesRight = Mat(S.nr, dim, S.dr.data());
      F.mvpMapLines.assign(S.nl, nullptr); F.mvbOutlierLines.assign(S.nl, false);
      F.SetPose(Mat(4, 4, S.Tcw.data()));
    };
    auto hold = [&](Graph& G, Frame& F, const LineFrame& S, bool tracked_by_cur) {
      for (int i = 0; i < S.nl; i++) {
        if (S.id_adapter[i] < 0) continue;
        std::unique_ptr<MapLine>& p = G.lines[S.id_adapter[i]];
        if (!p) { p.reset(new MapLine()); p->mnId = (unsigned long)S.id_adapter[i]; p->mX0 = Vector3d(S.x0[3 * i], S.x0[3 * i + 1], S.x0[3 * i + 2]); p->mDir = Vector3d(S.dir[3 * i], S.dir[3 * i + 1], S.dir[3 * i + 2]); }
        if (tracked_by_cur) p->tracked_last_id = (long)G.Cur.mnId;            // a line the current frame holds was tracked by it (:1117)
        F.mvpMapLines[i] = p.get();
      }
    };
    const double K[9] = {stereo[0], stereo[1], stereo[2], stereo[3], stereo[4], stereo[5], stereo[6], stereo[7], stereo[8]};
    lld_adapter::StereoLineParams sp; std::memcpy(sp.K, K, sizeof K); sp.b = stereo[9]; sp.tau = stereo[10]; sp.minLineLength = (int)stereo[11];
    lld_adapter::TrackingMembers tr;
    auto write_graph = [&](const Graph& G, int ret, const std::vector<MapLine*>& created, const std::vector<int>& match) {
      const int32_t r32 = ret, n_map = (int32_t)G.map.mspMapLines.size();
      wr(out, &r32, 1); wr(out, &n_map, 1); wr_ints(out, match);
      std::vector<int32_t> cid(C.nl + 1, -1), fid(C.nl + 1, -1), kid(C.nl + 1, -1), obs(C.nl + 1, -1); std::vector<double> x(3 * (size_t)C.nl + 3, 0.0), d(3 * (size_t)C.nl + 3, 0.0);
      for (int i = 0; i < C.nl; i++) {
        if (created[i]) {
          const MapLine* ml = created[i];
          cid[i] = (int32_t)ml->mnId;
          Vector3d a, b; ml->GetMinimalPos(&a, &b);
          for (int k = 0; k < 3; k++) { x[3 * i + k] = a(k); d[3 * i + k] = b(k); }
          // one observation, in pKF at index i; ref_idx = i; descriptors computed once; marked as tracked by the current frame
          const std::map<KeyFrame*, size_t> o = ml->GetObservations();
          obs[i] = (o.size() == 1 && o.begin()->first == &G.KF && (int)o.begin()->second == i && ml->ref_idx == i && ml->n_distinctive == 1 &&
                    ml->tracked_last_id == (long)G.Cur.mnId && G.map.mspMapLines.count(created[i])) ? 1 : 0;
        }
        if (G.Cur.mvpMapLines[i]) fid[i] = (int32_t)G.Cur.mvpMapLines[i]->mnId;
        if (i < (int)G.KF.mvpMapLines.size() && G.KF.mvpMapLines[i]) kid[i] = (int32_t)G.KF.mvpMapLines[i]->mnId;
      }
      wr(out, cid.data(), C.nl); wr(out, obs.data(), C.nl); wr(out, fid.data(), C.nl); wr(out, kid.data(), C.nl); wr(out, x.data(), 3 * (size_t)C.nl); wr(out, d.data(), 3 * (size_t)C.nl);
    };
    {
      // the device route
      Graph G;
      frame_of(G.Cur, C, 12); frame_of(G.Last, L, 11);
      lld_adapter::FrameOnDevice dcur(ctx.get(), G.Cur, sp), dlast(ctx.get(), G.Last, sp);
      wr_ints(out, G.Cur.line_matches);
      std::vector<int> host_lm;                                              // the host MatchLines adapter on the same objects
      lld_adapter::TwoFrameLineMatcher(ctx, K, sp.b, sp.tau, sp.minLineLength).MatchLines(G.Cur.mvLinesLeft, G.Cur.mvLinesRight, G.Cur.mDescriptorsLines,
                                                                                        G.Cur.mDescriptorsLinesRight, &host_lm);
      wr_ints(out, host_lm);
      hold(G, G.Cur, C, true); hold(G, G.Last, L, false);
      dcur.SetFrameState(tr, G.Cur); dlast.SetFrameState(tr, G.Last);
      MapLine::nNextId() = (unsigned long)first_new_id;
      std::vector<MapLine*> created; std::vector<int> match;
      const int ret = dcur.MatchLinesLastKF(tr, G.Cur, dlast, &G.KF, &G.map, &created, &match);
      for (MapLine* ml : created) if (ml) G.made.push_back(std::unique_ptr<MapLine>(ml));
      write_graph(G, ret, created, match);
      // the host route on a second, identical graph (line_matches as the device left them in the first)
      Graph H;
      frame_of(H.Cur, C, 12); frame_of(H.Last, L, 11);
      H.Cur.line_matches = G.Cur.line_matches; H.Last.line_matches = G.Last.line_matches;
      hold(H, H.Cur, C, true); hold(H, H.Last, L, false);
      MapLine::nNextId() = (unsigned long)first_new_id;
      lld_adapter::TrackingLines tl; std::memcpy(tl.K, K, sizeof K);
      tl.mb = H.Cur.mb; tl.mnMaxX = H.Cur.mnMaxX; tl.mnMaxY = H.Cur.mnMaxY; tl.mdThr = tr.mdThr; tl.monocular = false;
      std::vector<MapLine*> created_h; std::vector<int> match_h;
      const int ret_h = lld_adapter::MatchLinesLastKF(ctx, tl, H.Cur, H.Last, C.T_wc.data(), L.T_wc.data(), &H.KF, &H.map, &created_h, &match_h);
      for (MapLine* ml : created_h) if (ml) H.made.push_back(std::unique_ptr<MapLine>(ml));
      write_graph(H, ret_h, created_h, match_h);
    }
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "frame_lines_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
