// reloc_harness.cpp — Tracking::Relocalization on the device-resident frame, from compiled C++, twice:
//   1. over include/lld_amd.hpp: TrackedFrame::ComputeBoW / Relocalization / Download;
//   2. through adapters/lld_tracking_adapter.cc on live Frame / KeyFrame / MapPoint test doubles (FrameOnDevice::Relocalization), writing out
//      what the routine left in the objects.
// usage: reloc_harness <vocabulary.txt> <scene.bin> <out.bin>; the layouts are those of lld_slam_amd/tracking.py write_reloc_scene /
// read_reloc_result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct Cand {
  int n, nn, nv, is_bad; uint32_t seed;
  std::vector<uint32_t> desc, pdesc; std::vector<float> ang, pos, maxd, mind; std::vector<int32_t> id, node, start, feat; std::vector<uint8_t> obs;
};

void write_reloc(FILE* f, const lld_reloc_result& r, int K) {
  const int32_t h[6] = {r.matched, r.winner, r.round, r.n_good, r.n_rounds, r.n_kept};
  wr(f, h, 6); wr(f, r.Tcw, 16);
  wr(f, r.n_bow, K); wr(f, r.discarded, K); wr(f, r.rounds, K); wr(f, r.n_good_last, K); wr(f, r.rungs, K); wr(f, r.n_additional1, K); wr(f, r.n_additional2, K);
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
  if (argc != 4) { std::fprintf(stderr, "usage: reloc_harness <vocabulary.txt> <scene.bin> <out.bin>\n"); return 2; }
  try {
    FILE* in = std::fopen(argv[2], "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(in, 4);
    const int nt = hd[0], nlev = hd[1], K = hd[2], levelsup = hd[3];
    const std::vector<float> bounds = rd<float>(in, 6), scale = rd<float>(in, nlev), sigma2 = rd<float>(in, nlev), inv_sigma2 = rd<float>(in, nlev);
    const std::vector<double> camg = rd<double>(in, 6);
    const std::vector<uint32_t> fdesc = rd<uint32_t>(in, (size_t)nt * 8);
    const std::vector<float> fxy = rd<float>(in, (size_t)nt * 2); const std::vector<int32_t> foct = rd<int32_t>(in, nt);
    const std::vector<float> fur = rd<float>(in, nt), fang = rd<float>(in, nt);
    lld_frame_view view; { const std::vector<char> b = rd<char>(in, sizeof view); std::memcpy(&view, b.data(), sizeof view); }
    const std::vector<float> Tcw = rd<float>(in, 16);
    std::vector<Cand> C(K);
    for (int c = 0; c < K; c++) {
      const std::vector<int32_t> h = rd<int32_t>(in, 5);
      Cand& q = C[c];
      q.n = h[0]; q.nn = h[1]; q.nv = h[2]; q.is_bad = h[3]; q.seed = (uint32_t)h[4];
      q.desc = rd<uint32_t>(in, (size_t)q.n * 8); q.pdesc = rd<uint32_t>(in, (size_t)q.n * 8); q.ang = rd<float>(in, q.n); q.id = rd<int32_t>(in, q.n);
      q.pos = rd<float>(in, (size_t)q.n * 3); q.obs = rd<uint8_t>(in, q.n); q.maxd = rd<float>(in, q.n); q.mind = rd<float>(in, q.n);
      q.node = rd<int32_t>(in, q.nn); q.start = rd<int32_t>(in, q.nn + 1); q.feat = rd<int32_t>(in, q.nv);
    }
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
      std::vector<lld_ref_keyframe> kfs(K); std::vector<lld_reloc_candidate> ex(K);
      for (int c = 0; c < K; c++) {
        const Cand& q = C[c];
        std::memset(&kfs[c], 0, sizeof kfs[c]); std::memset(&ex[c], 0, sizeof ex[c]);
        kfs[c].n = q.n; kfs[c].desc = q.desc.data(); kfs[c].angle = q.ang.data(); kfs[c].point_id = q.id.data(); kfs[c].world_pos = q.pos.data(); kfs[c].has_obs = q.obs.data();
        kfs[c].n_nodes = q.nn; kfs[c].node = q.node.data(); kfs[c].node_start = q.start.data(); kfs[c].feature = q.feat.data();
        ex[c].max_distance = q.maxd.data(); ex[c].min_distance = q.mind.data(); ex[c].point_desc = q.pdesc.data(); ex[c].is_bad = q.is_bad; ex[c].seed = q.seed;
      }
      tf.ComputeBoW(voc.get(), levelsup);
      lld_amd::TrackedFrame::RelocRecord rec;
      const int32_t ok = tf.Relocalization(view, Tcw.data(), kfs, ex, &rec) ? 1 : 0;
      wr(out, &ok, 1);
      write_reloc(out, rec.r, K);
      lld_amd::TrackRecord r1;
      tf.Download(&r1, nullptr);
      wr(out, r1.kp_point_id.data(), nt); wr(out, r1.kp_outlier.data(), nt);
    }

    // ---------------------------------------------------------------- 2. the adapter on live objects
    {
      std::vector<std::unique_ptr<MapPoint> > points;
      std::vector<std::unique_ptr<KeyFrame> > keyframes;
      std::vector<KeyFrame*> vpCandidateKFs;
      std::vector<uint32_t> seeds;
      for (int c = 0; c < K; c++) {
        const Cand& q = C[c];
        keyframes.emplace_back(new KeyFrame());
        KeyFrame& KF = *keyframes.back();
        KF.N = q.n; KF.mvKeysUn.resize(q.n); KF.mvpMapPoints.assign(q.n, nullptr); KF.mDescriptors = MatU8(q.n, 32); KF.mbBad = q.is_bad != 0;
        if (q.n) std::memcpy(KF.mDescriptors.ptr<unsigned char>(), q.desc.data(), (size_t)q.n * 32);
        for (int k = 0; k < q.n; k++) {
          KF.mvKeysUn[k].angle = q.ang[k];
          if (q.id[k] < 0) continue;
          points.emplace_back(new MapPoint());
          MapPoint* p = points.back().get();
          p->mnId = (unsigned long)q.id[k]; p->mWorldPos = Mat(3, 1, &q.pos[3 * (size_t)k]); p->nObs = q.obs[k] ? 2 : 0;
          p->mfMaxDistance = q.maxd[k]; p->mfMinDistance = q.mind[k]; p->mDescriptor = MatU8(1, 32);
          std::memcpy(p->mDescriptor.ptr<unsigned char>(), &q.pdesc[8 * (size_t)k], 32);
          KF.mvpMapPoints[k] = p;
        }
        for (int i = 0; i < q.nn; i++) KF.mFeatVec[(unsigned int)q.node[i]].assign(q.feat.begin() + q.start[i], q.feat.begin() + q.start[i + 1]);
        vpCandidateKFs.push_back(&KF); seeds.push_back(q.seed);
      }
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
      Cur.SetPose(Mat(4, 4, Tcw.data()));                                       // the pose the lost frame carries into the routine
      lld_adapter::TrackingMembers tr; tr.gamma = camg[5];
      lld_adapter::FrameOnDevice dev(ctx.get(), Cur);
      dev.ComputeBoW(Cur, voc.get(), levelsup);                                // the caller needs the frame's vectors for DetectRelocalizationCandidates (:1844)
      const int32_t ok = dev.Relocalization(tr, Cur, vpCandidateKFs, nullptr, levelsup, &seeds) ? 1 : 0;   // ... so the routine does not transform again
      wr(out, &ok, 1);
      write_frame_state(out, Cur);
    }
    std::fclose(out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "reloc_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
