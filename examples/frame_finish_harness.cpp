// frame_finish_harness.cpp — the tail of Tracking::Track (keyframe decision, new stereo points, outlier drop) on the resident frame, from compiled C++:
//   1. over include/lld_amd.hpp: TrackedFrame::SetState (what stage 2 left in the frame) + TrackedFrame::Finish;
//   2. the host loops of frame_finish_host.cpp on the same state: the route a caller ran before the device call existed;
//   3. through adapters/lld_tracking_adapter.cc on live Frame / KeyFrame / MapPoint / Map test doubles: FrameOnDevice::SetFrameState, NeedNewKeyFrame,
//      CreateNewKeyFrame, DropOutliers, and the object graph they leave; then FrameOnDevice::UpdateLastFrame on a second, identical graph.
// usage: frame_finish_harness <scene.bin> <out.bin>; the layouts are those of tests/frame_finish_scenes.py write_harness_scene / read_harness_result.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "../adapters/lld_tracking_adapter.h"
#include "../include/lld_amd.hpp"
#include "frame_finish_host.h"

using namespace lld_slam;

namespace {

template <class T> std::vector<T> rd(FILE* f, size_t n) {
  std::vector<T> v(n + 1);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short scene file\n"); std::exit(2); }
  v.resize(n);
  return v;
}
template <class T> void wr(FILE* f, const T* p, size_t n) { if (n) std::fwrite(p, sizeof(T), n, f); }

void wr_result(FILE* f, const lld_frame_finish_result& r, int n) {
  const int32_t sc[7] = {r.n_tracked_close, r.n_non_tracked_close, r.need, r.interrupt_ba, r.made, r.n_visited, r.n_created};
  wr(f, sc, 7); wr(f, r.created, n); wr(f, r.new_id, n); wr(f, r.x3d, 3 * (size_t)n); wr(f, r.kp_point_id, n); wr(f, r.order, n);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: frame_finish_harness <scene.bin> <out.bin>\n"); return 2; }
  try {
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(in, 8);
    const int nt = hd[0], nlev = hd[1], first_new_id = hd[2], force = hd[3];
    const std::vector<float> bounds = rd<float>(in, 8), scale = rd<float>(in, nlev), sigma2 = rd<float>(in, nlev), inv_sigma2 = rd<float>(in, nlev);
    const float th_depth = bounds[6];
    const std::vector<double> cam = rd<double>(in, 5);
    const std::vector<uint32_t> fdesc = rd<uint32_t>(in, (size_t)nt * 8);
    const std::vector<float> fxy = rd<float>(in, (size_t)nt * 2); const std::vector<int32_t> foct = rd<int32_t>(in, nt);
    const std::vector<float> fur = rd<float>(in, nt), fang = rd<float>(in, nt);
    lld_frame_view view;
    { const std::vector<char> b = rd<char>(in, sizeof view); std::memcpy(&view, b.data(), sizeof view); }
    const std::vector<float> Tcw = rd<float>(in, 16), depth = rd<float>(in, nt);
    const std::vector<int32_t> kp_id = rd<int32_t>(in, nt); const std::vector<float> kp_world = rd<float>(in, (size_t)nt * 3);
    const std::vector<uint8_t> kp_obs = rd<uint8_t>(in, nt), kp_out = rd<uint8_t>(in, nt);
    const std::vector<int32_t> dec = rd<int32_t>(in, 12); const std::vector<int64_t> ids = rd<int64_t>(in, 3);
    std::fclose(in);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    lld_amd::Context ctx(0);

    lld_frame_finish_params p; std::memset(&p, 0, sizeof p);
    p.th_depth = th_depth; p.first_new_id = first_new_id; p.force = force;
    p.only_tracking = dec[0]; p.mapper_stopped = dec[1]; p.mapper_idle = dec[2]; p.keyframes_in_queue = dec[3]; p.set_not_stop_ok = dec[4]; p.monocular = dec[5];
    p.max_frames = dec[6]; p.min_frames = dec[7]; p.n_keyframes = dec[8]; p.n_ref_matches = dec[9]; p.n_matches_inliers = dec[10]; p.sensor_rgbd = dec[11];
    p.frame_id = ids[0]; p.last_reloc_frame_id = ids[1]; p.last_keyframe_id = ids[2];
    p.depth = depth.data();

    // ---------------------------------------------------------------- 1. include/lld_amd.hpp
    {
      lld_orb_search kp; std::memset(&kp, 0, sizeof kp);
      kp.nt = nt; kp.t_desc = fdesc.data(); kp.t_xy = fxy.data(); kp.t_octave = foct.data(); kp.t_uright = fur.data(); kp.t_angle = fang.data();
      kp.grid_min_x = bounds[0]; kp.grid_min_y = bounds[1]; kp.grid_width_inv = bounds[4]; kp.grid_height_inv = bounds[5]; kp.grid_cols = 64; kp.grid_rows = 48;
      kp.n_levels = nlev; kp.level_scale = scale.data(); kp.level_sigma2 = sigma2.data(); kp.level_inv_sigma2 = inv_sigma2.data();
      lld_amd::TrackedFrame tf(ctx, kp, nullptr);
      tf.params.cam = lld_camera{cam[0], cam[1], cam[2], cam[3], cam[4]};
      lld_frame_held held; std::memset(&held, 0, sizeof held);
      held.kp_point_id = kp_id.data(); held.kp_world_pos = kp_world.data(); held.kp_has_obs = kp_obs.data(); held.kp_outlier = kp_out.data();
      tf.SetState(view, Tcw.data(), held);
      lld_amd::TrackedFrame::NewStereoPoints R;
      const bool need = tf.Finish(p, &R);
      if (need != (R.r.need != 0)) throw std::runtime_error("TrackedFrame::Finish: the return value is not `need`");
      wr_result(out, R.r, nt);
    }

    // ---------------------------------------------------------------- 2. the host loops on the same state
    {
      std::vector<int32_t> id = kp_id; std::vector<uint8_t> obs = kp_obs, outl = kp_out; std::vector<float> world = kp_world;
      id.resize(nt + 1); obs.resize(nt + 1); outl.resize(nt + 1); world.resize(3 * (size_t)nt + 3);
      for (int i = 0; i < nt; i++) if (id[i] < 0) obs[i] = 0;
      lld_amd::TrackedFrame::NewStereoPoints R;
      R.bind(nt);
      frame_finish_host_tail(nt, depth.data(), fxy.data(), &view, &p, id.data(), obs.data(), outl.data(), world.data(), &R.r);
      wr_result(out, R.r, nt);
    }

    // ---------------------------------------------------------------- 3. the adapter on live objects
    struct Graph { Frame F; KeyFrame KF; Map map; std::vector<std::unique_ptr<MapPoint> > held, made; };
    auto frame_of = [&](Graph& G, unsigned long id) {
      Frame& F = G.F;
      F.N = nt; F.mnId = id; F.fx = (float)cam[0]; F.fy = (float)cam[1]; F.cx = (float)cam[2]; F.cy = (float)cam[3]; F.mbf = (float)cam[4]; F.mb = F.mbf / F.fx;
      F.mvKeysUn.resize(nt);
      for (int k = 0; k < nt; k++) { F.mvKeysUn[k].pt.x = fxy[2 * k]; F.mvKeysUn[k].pt.y = fxy[2 * k + 1]; F.mvKeysUn[k].octave = foct[k]; F.mvKeysUn[k].angle = fang[k]; }
      F.mvKeys = F.mvKeysUn; F.mvuRight = fur; F.mvDepth = depth; F.mvInvLevelSigma2 = inv_sigma2; F.mvScaleFactors = scale; F.mvLevelSigma2 = sigma2;
      F.mvuRight.resize(nt + 1); F.mvDepth.resize(nt + 1);                    // (non-null data() for an empty frame)
      F.mvpMapPoints.assign(nt, nullptr); F.mvbOutlier.assign(nt, false);
      F.mDescriptors = MatU8(nt, 32);
      if (nt) std::memcpy(F.mDescriptors.ptr<unsigned char>(), fdesc.data(), (size_t)nt * 32);
      F.mnMinX = bounds[0]; F.mnMinY = bounds[1]; F.mnMaxX = bounds[2]; F.mnMaxY = bounds[3]; F.mfGridElementWidthInv = bounds[4]; F.mfGridElementHeightInv = bounds[5];
      F.mnScaleLevels = nlev; F.mfScaleFactor = nlev > 1 ? scale[1] : 1.f; F.mfLogScaleFactor = view.log_scale_factor;
      F.SetPose(Mat(4, 4, Tcw.data()));
      for (int k = 0; k < nt; k++) {
        F.mvbOutlier[k] = kp_out[k] != 0;
        if (kp_id[k] < 0) continue;
        G.held.push_back(std::unique_ptr<MapPoint>(new MapPoint()));
        MapPoint* mp = G.held.back().get();
        mp->mnId = (unsigned long)kp_id[k]; mp->nObs = kp_obs[k] ? 2 : 0; mp->mWorldPos = Mat(3, 1, &kp_world[3 * (size_t)k]);
        F.mvpMapPoints[k] = mp;
      }
      G.KF.mvuRight = fur; G.KF.mvuRight.resize(nt + 1);
    };
    lld_adapter::TrackingMembers tr;
    tr.mbOnlyTracking = dec[0] != 0;
    {
      Graph G;
      frame_of(G, (unsigned long)ids[0]);
      lld_adapter::FrameOnDevice dev(ctx.get(), G.F);
      dev.SetFrameState(tr, G.F);
      lld_adapter::KeyFrameDecision d;
      d.mThDepth = th_depth; d.mapperStopped = dec[1] != 0; d.bLocalMappingIdle = dec[2] != 0; d.KeyframesInQueue = dec[3]; d.setNotStopOk = dec[4] != 0; d.monocular = dec[5] != 0;
      d.mMaxFrames = dec[6]; d.mMinFrames = dec[7]; d.nKFs = dec[8]; d.nRefMatches = dec[9]; d.mnMatchesInliers = dec[10]; d.rgbd = dec[11] != 0;
      d.mnLastRelocFrameId = (unsigned long)ids[1]; d.mnLastKeyFrameId = (unsigned long)ids[2];
      MapPoint::nNextId() = (unsigned long)first_new_id;
      bool interrupt = false;
      const bool need = dev.NeedNewKeyFrame(tr, d, G.F, &interrupt);
      std::vector<MapPoint*> created(nt, nullptr);
      if (need && dev.KeyFrameMade()) {
        G.KF.mvpMapPoints = G.F.mvpMapPoints;                                 // pKF = new KeyFrame(mCurrentFrame, ..) (:1375)
        dev.CreateNewKeyFrame(tr, G.F, &G.KF, &G.map, nullptr, &created);
      }
      dev.DropOutliers(G.F);
      for (MapPoint* mp : created) if (mp) G.made.push_back(std::unique_ptr<MapPoint>(mp));
      const int32_t hdr[4] = {need, interrupt, dev.KeyFrameMade(), (int32_t)G.map.mspMapPoints.size()};
      wr(out, hdr, 4);
      std::vector<int32_t> fid(nt + 1, -1), kid(nt + 1, -1), ok(nt + 1, -1), order; std::vector<float> world(3 * (size_t)nt + 3, 0.f);
      for (int i = 0; i < nt; i++) {
        if (G.F.mvpMapPoints[i]) fid[i] = (int32_t)G.F.mvpMapPoints[i]->mnId;
        if (i < (int)G.KF.mvpMapPoints.size() && G.KF.mvpMapPoints[i]) kid[i] = (int32_t)G.KF.mvpMapPoints[i]->mnId;
        if (!created[i]) continue;
        const MapPoint* mp = created[i];
        const std::map<KeyFrame*, size_t> o = mp->GetObservations();
        // one observation, in pKF at keypoint i, counted as AddObservation counts it; the reference keyframe and the map are the caller's
        ok[i] = (o.size() == 1 && o.begin()->first == &G.KF && (int)o.begin()->second == i && mp->Observations() == (fur[i] >= 0 ? 2 : 1) && mp->mpRefKF == &G.KF &&
                 mp->mpMap == &G.map && G.map.mspMapPoints.count(created[i])) ? 1 : 0;
        const Mat P = mp->GetWorldPos();
        for (int c = 0; c < 3; c++) world[3 * (size_t)i + c] = P.at<float>(c);
        order.push_back((int32_t)mp->mnId);
      }
      std::sort(order.begin(), order.end());
      wr(out, fid.data(), nt); wr(out, kid.data(), nt); wr(out, ok.data(), nt); wr(out, world.data(), 3 * (size_t)nt); wr(out, order.data(), order.size());
    }
    {
      // UpdateLastFrame on an identical graph: the frame as the LAST frame of the next Track() in localisation mode
      Graph G;
      frame_of(G, (unsigned long)ids[0]);
      lld_adapter::FrameOnDevice dev(ctx.get(), G.F);
      dev.SetFrameState(tr, G.F);                                             // what its own Track() left on the device
      MapPoint::nNextId() = (unsigned long)first_new_id;
      std::vector<MapPoint*> temporal;
      dev.UpdateLastFrame(tr, th_depth, G.F, &G.map, &temporal);
      const int32_t n_tmp = (int32_t)temporal.size();
      wr(out, &n_tmp, 1);
      std::vector<int32_t> fid(nt + 1, -1), tmp_ids; std::vector<float> world(3 * (size_t)nt + 3, 0.f);
      for (int i = 0; i < nt; i++) {
        MapPoint* mp = G.F.mvpMapPoints[i];
        if (!mp) continue;
        fid[i] = (int32_t)mp->mnId;
        if (std::find(temporal.begin(), temporal.end(), mp) == temporal.end()) continue;
        const Mat P = mp->GetWorldPos();
        for (int c = 0; c < 3; c++) world[3 * (size_t)i + c] = P.at<float>(c);
      }
      for (MapPoint* mp : temporal) { tmp_ids.push_back((int32_t)mp->mnId); G.made.push_back(std::unique_ptr<MapPoint>(mp)); }
      wr(out, fid.data(), nt); wr(out, world.data(), 3 * (size_t)nt); wr(out, tmp_ids.data(), tmp_ids.size());
    }
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "frame_finish_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
