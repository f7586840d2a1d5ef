// refkf_harness.cpp — Tracking::TrackReferenceKeyFrame + TrackLocalMap on the device-resident frame, from compiled C++, twice:
//   1. over include/lld_amd.hpp: ORBVocabulary::loadFromTextFile, TrackedFrame::ComputeBoW / TrackReferenceKeyFrame / TrackLocalMap / Download;
//   2. through adapters/lld_tracking_adapter.cc on live Frame / KeyFrame / MapPoint test doubles (FrameOnDevice::TrackReferenceKeyFrame, then
//      FrameOnDevice::TrackLocalMap), writing out what the routines left in the objects.
// usage: refkf_harness <vocabulary.txt> <scene.bin> <out.bin>; the layouts are those of lld_slam_amd/tracking.py write_refkf_scene /
// read_refkf_result (a scene without lines).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

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

void write_record(FILE* f, const lld_amd::TrackRecord& R, int nt) {
  wr(f, R.r.pose_qt, 7); wr(f, &R.r.chi2, 1);
  const int32_t c[14] = {R.r.n_inliers, R.r.lm_iterations, R.r.lm_trials, R.r.n_edges, R.r.n_search_first, R.r.n_search, R.r.used_wide, R.r.n_points,
                         R.r.n_points_map, R.r.n_lines_matched, R.r.n_lines, R.r.n_discarded, R.r.n_point_edges, R.r.n_in_view};
  wr(f, c, 14); wr(f, R.kp_point_id.data(), nt); wr(f, R.kp_outlier.data(), nt);
}

void write_frame_state(FILE* f, const Frame& F) {
  std::vector<int32_t> id(F.N + 1, -1); std::vector<uint8_t> out(F.N + 1, 0);
  for (int k = 0; k < F.N; k++) { if (F.mvpMapPoints[k]) id[k] = (int32_t)F.mvpMapPoints[k]->mnId; out[k] = F.mvbOutlier[k]; }
  wr(f, id.data(), F.N); wr(f, out.data(), F.N);
  float T[16] = {0};
  if (!F.mTcw.empty()) std::memcpy(T, F.mTcw.ptr<float>(), sizeof T);
  wr(f, T, 16);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: refkf_harness <vocabulary.txt> <scene.bin> <out.bin>\n"); return 2; }
  try {
    FILE* in = std::fopen(argv[2], "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(in, 8);
    const int nt = hd[0], nlev = hd[1], nk = hd[2], nn = hd[3], nv = hd[4], nm = hd[5], levelsup = hd[6];
    const std::vector<float> bounds = rd<float>(in, 6), scale = rd<float>(in, nlev), sigma2 = rd<float>(in, nlev), inv_sigma2 = rd<float>(in, nlev);
    const std::vector<double> camg = rd<double>(in, 6);
    const std::vector<uint32_t> fdesc = rd<uint32_t>(in, (size_t)nt * 8);
    const std::vector<float> fxy = rd<float>(in, (size_t)nt * 2); const std::vector<int32_t> foct = rd<int32_t>(in, nt);
    const std::vector<float> fur = rd<float>(in, nt), fang = rd<float>(in, nt);
    lld_frame_view view; { const std::vector<char> b = rd<char>(in, sizeof view); std::memcpy(&view, b.data(), sizeof view); }
    const std::vector<float> Tcw = rd<float>(in, 16);
    const std::vector<uint32_t> kdesc = rd<uint32_t>(in, (size_t)nk * 8); const std::vector<float> kang = rd<float>(in, nk);
    const std::vector<int32_t> kid = rd<int32_t>(in, nk); const std::vector<float> kpos = rd<float>(in, (size_t)nk * 3); const std::vector<uint8_t> kobs = rd<uint8_t>(in, nk);
    const std::vector<int32_t> knode = rd<int32_t>(in, nn), kstart = rd<int32_t>(in, nn + 1), kfeat = rd<int32_t>(in, nv);
    const std::vector<float> mpos = rd<float>(in, (size_t)nm * 3), mnrm = rd<float>(in, (size_t)nm * 3), mmax = rd<float>(in, nm), mmin = rd<float>(in, nm);
    const std::vector<uint32_t> mdesc = rd<uint32_t>(in, (size_t)nm * 8); const std::vector<uint8_t> mobs = rd<uint8_t>(in, nm), mskip = rd<uint8_t>(in, nm);
    const std::vector<int32_t> mid = rd<int32_t>(in, nm);
    std::fclose(in);
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) { std::fprintf(stderr, "cannot open %s\n", argv[3]); return 2; }

    lld_amd::Context ctx(0);
    lld_amd::ORBVocabulary voc(ctx, 2, 4096);
    if (!voc.loadFromTextFile(argv[1])) { std::fprintf(stderr, "vocabulary refused\n"); return 2; }

    // ---------------------------------------------------------------- 1. include/lld_amd.hpp
    {
      lld_orb_search kp; std::memset(&kp, 0, sizeof kp);
      kp.nt = nt; kp.t_desc = fdesc.data(); kp.t_xy = fxy.data(); kp.t_octave = foct.data(); kp.t_uright = fur.data(); kp.t_angle = fang.data();
      kp.grid_min_x = bounds[0]; kp.grid_min_y = bounds[1]; kp.grid_width_inv = bounds[4]; kp.grid_height_inv = bounds[5]; kp.grid_cols = 64; kp.grid_rows = 48;
      kp.n_levels = nlev; kp.level_scale = scale.data(); kp.level_sigma2 = sigma2.data(); kp.level_inv_sigma2 = inv_sigma2.data();
      lld_amd::TrackedFrame tf(ctx, kp, nullptr);
      tf.params.cam = lld_camera{camg[0], camg[1], camg[2], camg[3], camg[4]}; tf.params.pose.gamma = camg[5];
      lld_ref_keyframe kf; std::memset(&kf, 0, sizeof kf);
      kf.n = nk; kf.desc = kdesc.data(); kf.angle = kang.data(); kf.point_id = kid.data(); kf.world_pos = kpos.data(); kf.has_obs = kobs.data();
      kf.n_nodes = nn; kf.node = knode.data(); kf.node_start = kstart.data(); kf.feature = kfeat.data();
      lld_map_points mp; std::memset(&mp, 0, sizeof mp);
      mp.n = nm; mp.world_pos = mpos.data(); mp.normal = mnrm.data(); mp.max_distance = mmax.data(); mp.min_distance = mmin.data(); mp.desc = mdesc.data();
      mp.has_obs = mobs.data(); mp.skip = mskip.data();
      tf.ComputeBoW(voc.get(), levelsup);
      tf.TrackReferenceKeyFrame(view, Tcw.data(), kf);
      tf.TrackLocalMap(mp, mid.data(), nullptr);
      lld_amd::TrackRecord r1, r2;
      tf.Download(&r1, &r2);
      write_record(out, r1, nt); write_record(out, r2, nt);
    }

    // ---------------------------------------------------------------- 2. the adapter on live objects
    {
      std::map<int32_t, std::unique_ptr<MapPoint> > points;                   // one MapPoint per id, shared by the keyframe and the local map
      std::vector<MapPoint*> local(nm, nullptr);
      for (int i = 0; i < nm; i++) {
        std::unique_ptr<MapPoint>& p = points[mid[i]];
        p.reset(new MapPoint());
        p->mnId = (unsigned long)mid[i]; p->mWorldPos = Mat(3, 1, &mpos[3 * (size_t)i]); p->mNormalVector = Mat(3, 1, &mnrm[3 * (size_t)i]);
        p->mfMaxDistance = mmax[i]; p->mfMinDistance = mmin[i]; p->mDescriptor = MatU8(1, 32);
        std::memcpy(p->mDescriptor.ptr<unsigned char>(), &mdesc[8 * (size_t)i], 32);
        p->nObs = mobs[i] ? 2 : 0; p->mbBad = mskip[i] != 0;
        local[i] = p.get();
      }
      KeyFrame KF;
      KF.N = nk; KF.mvKeysUn.resize(nk); KF.mvpMapPoints.assign(nk, nullptr); KF.mDescriptors = MatU8(nk, 32);
      if (nk) std::memcpy(KF.mDescriptors.ptr<unsigned char>(), kdesc.data(), (size_t)nk * 32);
      for (int k = 0; k < nk; k++) {
        KF.mvKeysUn[k].angle = kang[k];
        if (kid[k] < 0) continue;
        std::unique_ptr<MapPoint>& p = points[kid[k]];
        if (!p) { p.reset(new MapPoint()); p->mnId = (unsigned long)kid[k]; p->mWorldPos = Mat(3, 1, &kpos[3 * (size_t)k]); p->nObs = kobs[k] ? 2 : 0; }
        KF.mvpMapPoints[k] = p.get();
      }
      for (int i = 0; i < nn; i++) KF.mFeatVec[(unsigned int)knode[i]].assign(kfeat.begin() + kstart[i], kfeat.begin() + kstart[i + 1]);
      Frame Cur;
      Cur.N = nt; Cur.mnId = 7; Cur.fx = (float)camg[0]; Cur.fy = (float)camg[1]; Cur.cx = (float)camg[2]; Cur.cy = (float)camg[3]; Cur.mbf = (float)camg[4];
      Cur.mb = Cur.mbf / Cur.fx;
      Cur.mvKeysUn.resize(nt);
      for (int k = 0; k < nt; k++) { Cur.mvKeysUn[k].pt.x = fxy[2 * k]; Cur.mvKeysUn[k].pt.y = fxy[2 * k + 1]; Cur.mvKeysUn[k].octave = foct[k]; Cur.mvKeysUn[k].angle = fang[k]; }
      Cur.mvKeys = Cur.mvKeysUn; Cur.mvuRight = fur; Cur.mvInvLevelSigma2 = inv_sigma2; Cur.mvScaleFactors = scale; Cur.mvLevelSigma2 = sigma2;
      Cur.mvpMapPoints.assign(nt, nullptr); Cur.mvbOutlier.assign(nt, false);
      Cur.mDescriptors = MatU8(nt, 32);
      if (nt) std::memcpy(Cur.mDescriptors.ptr<unsigned char>(), fdesc.data(), (size_t)nt * 32);
      Cur.mnMinX = bounds[0]; Cur.mnMinY = bounds[1]; Cur.mnMaxX = bounds[2]; Cur.mnMaxY = bounds[3]; Cur.mfGridElementWidthInv = bounds[4]; Cur.mfGridElementHeightInv = bounds[5];
      Cur.mnScaleLevels = nlev; Cur.mfScaleFactor = nlev > 1 ? scale[1] : 1.f; Cur.mfLogScaleFactor = view.log_scale_factor;
      Frame Last;
      Last.SetPose(Mat(4, 4, Tcw.data()));
      lld_adapter::TrackingMembers tr; tr.gamma = camg[5];
      lld_adapter::FrameOnDevice dev(ctx.get(), Cur);
      const int32_t ok = dev.TrackReferenceKeyFrame(tr, Cur, Last, &KF, voc.get(), levelsup) ? 1 : 0;
      wr(out, &ok, 1);
      write_frame_state(out, Cur);
      std::vector<uint8_t> seen(nk + 1, 0), in_view(nk + 1, 0);
      for (int k = 0; k < nk; k++) if (KF.mvpMapPoints[k]) { seen[k] = KF.mvpMapPoints[k]->mnLastFrameSeen == Cur.mnId; in_view[k] = KF.mvpMapPoints[k]->mbTrackInView; }
      wr(out, seen.data(), nk); wr(out, in_view.data(), nk);
      std::vector<int32_t> fnode, fstart(1, 0), ffeat;                          // mCurrentFrame.mFeatVec as ComputeBoW left it
      for (DBoW2::FeatureVector::const_iterator it = Cur.mFeatVec.begin(); it != Cur.mFeatVec.end(); ++it) {
        fnode.push_back((int32_t)it->first);
        for (size_t j = 0; j < it->second.size(); j++) ffeat.push_back((int32_t)it->second[j]);
        fstart.push_back((int32_t)ffeat.size());
      }
      const int32_t cnt[2] = {(int32_t)fnode.size(), (int32_t)ffeat.size()};
      wr(out, cnt, 2); wr(out, fnode.data(), fnode.size()); wr(out, fstart.data(), fstart.size()); wr(out, ffeat.data(), ffeat.size());
      int32_t inliers = -1;
      if (!Cur.mTcw.empty()) dev.TrackLocalMap(tr, Cur, local, std::vector<MapLine*>(), std::vector<Mat>(), &inliers);
      wr(out, &inliers, 1);
      write_frame_state(out, Cur);
    }
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "refkf_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
