// lld_frame_reloc.hip — Tracking::Relocalization (src/Tracking.cc:1837-1998) as a stage of the device-resident frame chain
// (lld_frame_relocalize, include/lld_amd.h).
//
// The reference walks its candidates one after the other inside every round of its while loop.  Each PnPsolver owns its rand() stream and a
// candidate's ladder touches only what it wrote into the frame itself, so a round is evaluated here for every live candidate SIDE BY SIDE, each
// on its own copy ("slot") of mvpMapPoints / mvbOutlier / mTcw, and the first slot in candidate order that ends with nGood >= 50 is the
// reference's winner.  Per call: one upload of the candidates, one download of the K SearchByBoW counts (SetRansacParameters is the host's
// fp64 expression), then per round ONE status word.  Kernels of this file (the searches, PnP and PoseOptimization are the library's own
// kernels, run batched over the slots and predicated on the flags these write):
//
//   reloc_bow_match_kernel     SearchByBoW(pKF, F) for all candidates: one wavefront per (candidate, keyframe node) (lld_bow_merge.h)
//   reloc_bow_finish_kernel    one workgroup per candidate: rotation histogram, vvpMapPointMatches[i] and its count
//   reloc_pnp_assemble_kernel  the PnPsolver constructor (src/PnPsolver.cc:66-110) per kept candidate: its matches in ascending keypoint order
//   reloc_gate_kernel          after iterate(5): bNoMore -> the candidate leaves (:1910-1914); a pose -> the slot takes mTcw and the inliers
//                              (:1919-1934) and sFound becomes the candidate's skip bytes
//   reloc_after_pose_kernel    after each PoseOptimization: SetPose, nGood, the discards of :1941-1943 / :1969-1971, the decisions
//                              nGood < 10, nGood < 50, 30 < nGood < 50 and the rebuilt sFound of :1958-1961
//   reloc_between_kernel       nadditional + nGood >= 50 (:1950, :1965)
//   reloc_pick_kernel          the first slot in candidate order with nGood >= 50 becomes the frame; records; the status word
#include "lld_common.h"
#include "lld_bow_merge.h"
#include "lld_device_math.h"
#include "lld_frame_track_state.h"
#include "lld_pnp_internal.h"
#include "lld_track_internal.h"
#include "lld_wave.h"

namespace {

using namespace lld_track;
using namespace lld_bow_merge;

constexpr int kSlotThreads = 256;
constexpr int kAsmThreads = 1024;
constexpr int kFoundSlots = 2 * LLD_ORB_MAX_KEYPOINTS;         // sFound as an open-addressing set in LDS: at most nt ids, half full
constexpr int kMinBow = 15;                                    // if(nmatches<15) (:1874)
constexpr int kMaxRoundsSlack = 2;
enum { RUN_PO1 = 0, RUN_S1, RUN_PO2, RUN_S2, RUN_PO3, N_RUN };
enum { CUR_GOOD = 0, CUR_MASK, CUR_ITERATED, CUR_NO_MORE };    // of the running round, per slot
enum { REC_ROUNDS = 0, REC_GOOD, REC_MASK, REC_ADD1, REC_ADD2, REC_NO_MORE, REC_INTS = 8 };   // what the reference has done to a candidate so far
enum { ST_MATCHED = 0, ST_WINNER, ST_ROUND, ST_GOOD, ST_LIVE, ST_ROUNDS, ST_WORD = 7, ST_INTS = 8 };

struct CandDev { int32_t n, pad; const int32_t* point_id; uint8_t* skip; };   // a candidate's MapPoints and their "bad or already found" bytes

struct RelocDev {
  int K, nt;
  const CandDev* cand;
  // vvpMapPointMatches [K][nt] and SearchByBoW's counts [K][4]
  uint8_t* m_has; int32_t* m_id; uint8_t* m_obs; float* m_world; int32_t* m_cnt;
  // the slots: [K][nt] copies of mvpMapPoints (has, id, world, Observations() > 0) and mvbOutlier, mTcw as SE3Quat / result / float view
  uint8_t* s_has; int32_t* s_id; uint8_t* s_obs; float* s_world; uint8_t* s_out;
  double* s_pose_qt; double* s_pose_out; lld_frame_view* s_view;
  int32_t* run;                          // [N_RUN][K] the rungs' predicates
  int32_t* cnt1; int32_t* cnt2;          // [K][4] ap_counts of the two projected searches ([1] = nadditional)
  uint8_t* live;                         // [K] !vbDiscarded
  int32_t* cur; int32_t* rec; int32_t* status;
  const lld_pnp::PnpRes* pnp_res; const uint8_t* pnp_flags;   // vbInliers [K][nt]
};

__global__ __launch_bounds__(kMatchWaves * 64) void reloc_bow_match_kernel(const BowSearchDev* __restrict__ bows) {
  const BowSearchDev B = bows[blockIdx.y];
  const int w = blockIdx.x * kMatchWaves + (threadIdx.x >> 6);
  if (w >= B.n_kf_nodes) return;                 // whole wavefronts leave
  bow_match_node(B, w, threadIdx.x & 63);
}

__global__ __launch_bounds__(kFinishThreads) void reloc_bow_finish_kernel(const BowSearchDev* __restrict__ bows, const ApplyDev* __restrict__ aps) {
  __shared__ int hist[kHisto];
  __shared__ int ctl[4];
  const BowSearchDev B = bows[blockIdx.x];
  const ApplyDev A = aps[blockIdx.x];
  bow_finish_block(B, A, hist, ctl);
}

struct LevelTable { float v[LLD_ORB_MAX_LEVELS]; };

// PnPsolver(F, vpMapPointMatches) (:66-110): for(i < vpMapPointMatches.size()) if(pMP && !pMP->isBad()) push_back in keypoint order.  A match
// table holds good MapPoints only (SearchByBoW skips the others, ORBmatcher.cc:193-197), so N is SearchByBoW's count.
__global__ __launch_bounds__(kAsmThreads) void reloc_pnp_assemble_kernel(RelocDev R, const int32_t* __restrict__ off, const uint8_t* __restrict__ keep, lld_pnp::SlabDev slab,
                                                                         const float* __restrict__ t_xy, const int32_t* __restrict__ t_octave, LevelTable sigma2, float th2) {
  __shared__ int wsum[kAsmThreads / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  if (!keep[c]) return;                            // uniform over the workgroup
  const uint8_t* has = R.m_has + (size_t)c * R.nt;
  const float* world = R.m_world + 3 * (size_t)c * R.nt;
  const int per = (R.nt + kAsmThreads - 1) / kAsmThreads, k0 = min(tid * per, R.nt), k1 = min(k0 + per, R.nt);
  int cnt = 0;
  for (int k = k0; k < k1; k++) cnt += has[k] ? 1 : 0;
  int n_has;
  int e = off[c] + lld_wave::block_excl_scan<kAsmThreads>(cnt, wsum, n_has);
  const int end = off[c] + R.m_cnt[4 * c];         // (the count the host sized the slab by)
  for (int k = k0; k < k1; k++) {
    if (!has[k] || e >= end) continue;
    slab.pt[e] = make_float4(world[3 * k], world[3 * k + 1], world[3 * k + 2], __fmul_rn(sigma2.v[t_octave[k]], th2));   // mvMaxError (float)
    slab.uv[e] = make_float2(t_xy[2 * k], t_xy[2 * k + 1]);
    slab.kp[e] = k;
    e++;
  }
}

// sFound of slot c as the skip bytes of its candidate's MapPoints: bad, or its id among the ids the slot holds.
__device__ void mark_found(const RelocDev& R, int c, int32_t* tab) {
  const int tid = threadIdx.x;
  for (int i = tid; i < kFoundSlots; i += kSlotThreads) tab[i] = -1;
  __syncthreads();
  const uint8_t* has = R.s_has + (size_t)c * R.nt; const int32_t* id = R.s_id + (size_t)c * R.nt;
  for (int k = tid; k < R.nt; k += kSlotThreads) if (has[k]) seen_insert(tab, kFoundSlots - 1, id[k]);
  __syncthreads();
  const CandDev cd = R.cand[c];
  for (int q = tid; q < cd.n; q += kSlotThreads) {
    const int32_t pid = cd.point_id[q];
    cd.skip[q] = (pid < 0 || seen_lookup(tab, kFoundSlots - 1, pid)) ? 1 : 0;
  }
}

__global__ __launch_bounds__(kSlotThreads) void reloc_gate_kernel(RelocDev R, ViewConsts C) {
  __shared__ int32_t tab[kFoundSlots];
  const int c = blockIdx.x, tid = threadIdx.x;
  const bool live = R.live[c] != 0;
  const lld_pnp::PnpRes res = R.pnp_res[c];
  const bool pose = live && res.has_pose != 0;
  __syncthreads();                                 // every lane has read `live` before lane 0 clears it
  if (tid == 0) {
    for (int r = 0; r < N_RUN; r++) R.run[r * R.K + c] = (r == RUN_PO1 && pose) ? 1 : 0;
    R.cur[4 * c + CUR_GOOD] = -1; R.cur[4 * c + CUR_MASK] = 0; R.cur[4 * c + CUR_ITERATED] = live; R.cur[4 * c + CUR_NO_MORE] = live && res.no_more != 0;
    for (int q = 0; q < 4; q++) { R.cnt1[4 * c + q] = 0; R.cnt2[4 * c + q] = 0; }
    if (live && res.no_more != 0) R.live[c] = 0;   // vbDiscarded[i]=true; nCandidates--;  (:1910-1914)
  }
  if (!pose) return;
  // Tcw.copyTo(mCurrentFrame.mTcw); mvpMapPoints[j] = vbInliers[j] ? vvpMapPointMatches[i][j] : NULL over all nt entries (:1919-1934)
  const size_t o = (size_t)c * R.nt;
  const uint8_t* inl = R.pnp_flags + o;
  for (int k = tid; k < R.nt; k += kSlotThreads) {
    const bool has = inl[k] != 0 && R.m_has[o + k] != 0;
    R.s_has[o + k] = has; R.s_id[o + k] = has ? R.m_id[o + k] : -1; R.s_obs[o + k] = has ? R.m_obs[o + k] : 0; R.s_out[o + k] = 0;
    for (int q = 0; q < 3; q++) R.s_world[3 * (o + k) + q] = has ? R.m_world[3 * (o + k) + q] : 0.f;
  }
  if (tid == 64) {
    float Rf[9], tf[3];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) Rf[3 * i + j] = res.tcw[4 * i + j]; tf[i] = res.tcw[4 * i + 3]; }
    view_from_matrix(Rf, tf, C, &R.s_view[c], R.s_pose_qt + 7 * c);
  }
  __syncthreads();
  mark_found(R, c, tab);                           // sFound.insert(vvpMapPointMatches[i][j]) of the inliers (:1930)
}

__global__ __launch_bounds__(kSlotThreads) void reloc_after_pose_kernel(RelocDev R, ViewConsts C, int stage) {
  __shared__ int32_t tab[kFoundSlots];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int ri = stage == 1 ? RUN_PO1 : (stage == 2 ? RUN_PO2 : RUN_PO3);
  if (!R.run[ri * R.K + c]) return;                // uniform over the workgroup
  const int* pi = reinterpret_cast<const int*>(R.s_pose_out + 12 * (size_t)c + 8);
  const int nGood = pi[0], n_pt = pi[4];
  // pFrame->SetPose(pose) - unless PoseOptimization returned before it optimised (fewer than three points, Optimizer.cc:809-810)
  if (tid == 0 && n_pt >= 3) view_from_pose(R.s_pose_out + 12 * (size_t)c, C, &R.s_view[c], nullptr, R.s_pose_qt + 7 * c);
  const bool coarse = stage == 1 && nGood >= 10 && nGood < 50;       // if(nGood<10) continue; ... if(nGood<50)  (:1938, :1946)
  const bool narrow = stage == 2 && nGood > 30 && nGood < 50;        // if(nGood>30 && nGood<50)                  (:1956)
  if ((stage == 1 && nGood >= 10) || stage == 3) {                   // the outliers leave, their flags stay (:1941-1943, :1969-1971)
    const size_t o = (size_t)c * R.nt;
    for (int k = tid; k < R.nt; k += kSlotThreads)
      if (R.s_has[o + k] && R.s_out[o + k]) { R.s_has[o + k] = 0; R.s_id[o + k] = -1; }
  }
  if (tid == 0) {
    R.cur[4 * c + CUR_GOOD] = nGood;
    int m = R.cur[4 * c + CUR_MASK] | (stage == 1 ? LLD_RELOC_RUNG_POSE1 : (stage == 2 ? LLD_RELOC_RUNG_POSE2 : LLD_RELOC_RUNG_POSE3));
    if (coarse) { m |= LLD_RELOC_RUNG_SEARCH1; R.run[RUN_S1 * R.K + c] = 1; }
    if (narrow) { m |= LLD_RELOC_RUNG_SEARCH2; R.run[RUN_S2 * R.K + c] = 1; }
    R.cur[4 * c + CUR_MASK] = m;
  }
  if (narrow) {                                    // sFound.clear(); insert every mvpMapPoints[ip] (:1958-1961), flagged ones included
    __syncthreads();
    mark_found(R, c, tab);
  }
}

__global__ void reloc_between_kernel(RelocDev R, int which) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= R.K) return;
  if (which == 1) { if (R.run[RUN_S1 * R.K + c]) R.run[RUN_PO2 * R.K + c] = (R.cnt1[4 * c + 1] + R.cur[4 * c + CUR_GOOD] >= 50) ? 1 : 0; }   // :1950
  else            { if (R.run[RUN_S2 * R.K + c]) R.run[RUN_PO3 * R.K + c] = (R.cur[4 * c + CUR_GOOD] + R.cnt2[4 * c + 1] >= 50) ? 1 : 0; }   // :1965
}

// The reference stops at the first candidate, in order, whose attempt ends with nGood >= 50 (:1979-1983) and never reaches the ones behind it
// in that round: only the candidates up to the winner take this round into their records.
__global__ __launch_bounds__(kSlotThreads) void reloc_pick_kernel(RelocDev R, TrackDev D, ViewConsts C, int round) {
  __shared__ int win_sh, cnt_sh[2];
  const int tid = threadIdx.x;
  if (tid == 0) {
    int winner = -1;
    for (int c = 0; c < R.K && winner < 0; c++)
      if (R.run[RUN_PO1 * R.K + c] && R.cur[4 * c + CUR_GOOD] >= 50) winner = c;
    int n_live = 0;
    for (int c = 0; c < R.K; c++) {
      n_live += R.live[c] ? 1 : 0;
      if (!R.cur[4 * c + CUR_ITERATED] || (winner >= 0 && c > winner)) continue;
      int32_t* rec = R.rec + REC_INTS * c;
      rec[REC_ROUNDS]++;
      if (R.cur[4 * c + CUR_NO_MORE]) rec[REC_NO_MORE] = 1;
      if (R.run[RUN_PO1 * R.K + c]) {
        const int m = R.cur[4 * c + CUR_MASK];
        rec[REC_GOOD] = R.cur[4 * c + CUR_GOOD]; rec[REC_MASK] = m;
        rec[REC_ADD1] = (m & LLD_RELOC_RUNG_SEARCH1) ? R.cnt1[4 * c + 1] : 0;
        rec[REC_ADD2] = (m & LLD_RELOC_RUNG_SEARCH2) ? R.cnt2[4 * c + 1] : 0;
      }
    }
    R.status[ST_MATCHED] = winner >= 0; R.status[ST_WINNER] = winner; R.status[ST_ROUND] = winner >= 0 ? round : 0;
    R.status[ST_GOOD] = winner >= 0 ? R.cur[4 * winner + CUR_GOOD] : 0; R.status[ST_LIVE] = n_live; R.status[ST_ROUNDS] = round;
    R.status[ST_WORD] = winner >= 0 ? (int32_t)(0x80000000u | (unsigned)winner) : n_live;
    win_sh = winner; cnt_sh[0] = 0; cnt_sh[1] = 0;
  }
  __syncthreads();
  const int w = win_sh;
  if (w < 0) return;
  // the winner's slot is the frame: mvpMapPoints, mvbOutlier of the held ones, and the stage-1 record of the chain
  const size_t o = (size_t)w * R.nt;
  int n_pts = 0, n_map = 0;
  for (int k = tid; k < R.nt; k += kSlotThreads) {
    const bool has = R.s_has[o + k] != 0;
    const uint8_t bad = has ? R.s_out[o + k] : 0;
    D.kp_has[k] = has; D.kp_id[k] = has ? R.s_id[o + k] : -1; D.kp_obs[k] = has ? R.s_obs[o + k] : 0; D.kp_outlier[k] = bad;
    for (int q = 0; q < 3; q++) D.kp_world[3 * k + q] = has ? R.s_world[3 * (o + k) + q] : 0.f;
    D.rec_kp_id[0][k] = has ? R.s_id[o + k] : -1; D.rec_kp_out[0][k] = bad;
    if (has) { n_pts++; if (R.s_obs[o + k]) n_map++; }
  }
  lld_wave::sum_each(n_pts, n_map);
  if ((tid & 63) == 0) { atomicAdd(&cnt_sh[0], n_pts); atomicAdd(&cnt_sh[1], n_map); }
  __syncthreads();
  if (tid == 0) {
    for (int i = 0; i < 7; i++) D.pose_qt[i] = R.s_pose_qt[7 * w + i];
    *D.view = R.s_view[w];
    line_camera_from_view(C, *D.view, D.line_params);
    RecHeader& H = *D.rec_h[0];
    rec_header_from_pose(H, R.s_pose_out + 12 * (size_t)w);
    H.i[RI_SEARCH1] = R.m_cnt[4 * w]; H.i[RI_SEARCH] = R.m_cnt[4 * w];
    H.i[RI_POINTS] = cnt_sh[0]; H.i[RI_POINTS_MAP] = cnt_sh[1];
  }
}

// the stage-1 record of a frame that holds nothing (track_reset_launch zeroes the headers)
__global__ void reloc_record_clear_kernel(TrackDev D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < D.nt) { D.rec_kp_id[0][i] = -1; D.rec_kp_out[0][i] = 0; }
  if (i < D.nl) { D.rec_ln_id[0][i] = -1; D.rec_ln_out[0][i] = 0; }
}

}  // namespace

extern "C" int lld_frame_relocalize(lld_frame* f, const lld_track_params* P, const lld_frame_view* view, const double* pose_qt, int32_t K,
                                    const lld_ref_keyframe* cands, const lld_reloc_candidate* extra, const lld_pnp_params* pnp, lld_reloc_result* out) {
  if (!f || !P || !view || !pose_qt || !cands || !extra || !pnp || !out) return LLD_ERR_INVALID;
  if (!f->has_bow) return LLD_ERR_INVALID;                                   // mCurrentFrame.ComputeBoW() comes first (:1840)
  if (K < 1 || K > LLD_PNP_MAX_SOLVERS) return LLD_ERR_INVALID;
  const int nt = f->nt;
  if (nt > 0 && !f->has_angle) return LLD_ERR_INVALID;                       // ORBmatcher(0.75, true) / (0.9, true): mbCheckOrientation
  if (view->n_levels != f->consts.n_levels) return LLD_ERR_INVALID;
  if (!(P->cam.fx > 0) || !(P->cam.fy > 0) || !f->has_inv_sigma2) return LLD_ERR_INVALID;
  if (pnp->min_set != 4) return LLD_ERR_UNSUPPORTED;
  if (pnp->max_iterations < 1 || pnp->max_iterations > LLD_PNP_MAX_ITERATIONS || !(pnp->probability > 0.0 && pnp->probability < 1.0) ||
      !(pnp->epsilon > 0.0f && pnp->epsilon <= 1.0f) || !(pnp->th2 > 0.0f)) return LLD_ERR_INVALID;
  std::vector<int> nv(K, 0);
  int n_max = 0, nn_max = 0;
  for (int c = 0; c < K; c++) {
    int s = ref_keyframe_check(&cands[c], &nv[c]); if (s) return s;
    if (cands[c].n > 0 && (!extra[c].max_distance || !extra[c].min_distance)) return LLD_ERR_INVALID;
    n_max = std::max(n_max, cands[c].n); nn_max = std::max(nn_max, cands[c].n_nodes);
  }
  lld_ctx* ctx = f->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  int s = ensure_state(f); if (s) return s;
  lld_frame_track_state* S = f->track;
  fill_consts(S, P, view);
  const ViewConsts C = S->consts;

  // ---- layout: the uploaded block, then device-only state
  UploadBlock B; StageHeader H; H.reserve(B);
  const auto bows = B.take<BowSearchDev>(K); const auto aps = B.take<ApplyDev>(K); const auto cand = B.take<CandDev>(K);
  const Span<RelocProjSlot> proj[2] = {B.take<RelocProjSlot>(K), B.take<RelocProjSlot>(K)};
  const size_t pstride = orbs_problem_bytes(); const auto prob = B.take<char>(pstride * 2 * K);
  std::vector<RefKeyframeUp> U(K);
  for (int c = 0; c < K; c++) U[c].reserve(B, cands[c], nv[c], &extra[c]);
  B.end_upload();
  const size_t kn = (size_t)K * nt;
  // zeroed at the start of the call: match tables, counts, slots' flags and records
  const size_t o_zero = B.size;
  const auto mhas = B.take<uint8_t>(kn); const auto mid = B.take<int32_t>(kn); const auto mobs = B.take<uint8_t>(kn); const auto mworld = B.take<float>(kn, 3);
  const auto mcnt = B.take<int32_t>(K, 4), run = B.take<int32_t>(K, N_RUN), cnt1 = B.take<int32_t>(K, 4), cnt2 = B.take<int32_t>(K, 4), cur = B.take<int32_t>(K, 4);
  const auto rec = B.take<int32_t>(K, REC_INTS), status = B.take<int32_t>(ST_INTS);
  const size_t zero_bytes = B.size - o_zero;
  const auto taken = B.take<int32_t>(kn);
  const auto shas = B.take<uint8_t>(kn); const auto sid = B.take<int32_t>(kn); const auto sobs = B.take<uint8_t>(kn); const auto sworld = B.take<float>(kn, 3);
  const auto sout = B.take<uint8_t>(kn); const auto sqt = B.take<double>(K, 7); const auto spo = B.take<double>(K, 12); const auto sview = B.take<lld_frame_view>(K);
  const auto live = B.take<uint8_t>(K), keep = B.take<uint8_t>(K); const auto off_d = B.take<int32_t>(K);
  struct SlotScratch { Span<uint8_t> skip; SearchScratch search; };          // sFound as skip bytes and the projected searches' scratch, per candidate
  std::vector<SlotScratch> W(K);
  for (int c = 0; c < K; c++) { W[c].skip = B.take<uint8_t>(cands[c].n); W[c].search.reserve(B, cands[c].n, nt); }
  const auto pwork = B.take<char>(pose_slots_work_bytes(K, nt));
  s = stage_begin(S, ctx, 0, B); if (s) return s;
  // the second pinned region: the small uploads after the counts are known, the status word, the final records
  UploadBlock B2; const auto h2_keep = B2.take<uint8_t>(K);
  const auto h2_off = B2.take<int32_t>(K), h2_status = B2.take<int32_t>(ST_INTS), h2_cnt = B2.take<int32_t>(K), h2_rec = B2.take<int32_t>(K, REC_INTS); const auto h2_view = B2.take<lld_frame_view>(1);
  s = ensure_stage(S, 1, B2.size); if (s) return s;
  B2.bind(S->h_stage[1], nullptr);

  // ---- the device's view of everything
  RelocDev R{};
  R.K = K; R.nt = nt; R.cand = B.dev(cand);
  R.m_has = B.dev(mhas); R.m_id = B.dev(mid); R.m_obs = B.dev(mobs); R.m_world = B.dev(mworld); R.m_cnt = B.dev(mcnt);
  R.s_has = B.dev(shas); R.s_id = B.dev(sid); R.s_obs = B.dev(sobs); R.s_world = B.dev(sworld); R.s_out = B.dev(sout);
  R.s_pose_qt = B.dev(sqt); R.s_pose_out = B.dev(spo); R.s_view = B.dev(sview);
  R.run = B.dev(run); R.cnt1 = B.dev(cnt1); R.cnt2 = B.dev(cnt2); R.live = B.dev(live); R.cur = B.dev(cur); R.rec = B.dev(rec); R.status = B.dev(status);

  // ---- pack
  H.stage(B, C, view, pose_qt);
  for (int c = 0; c < K; c++) {
    const int n = cands[c].n;
    U[c].stage(B, cands[c], &extra[c]);
    BowSearchDev& Bs = B.host(bows)[c];
    std::memset(&Bs, 0, sizeof(Bs));
    bow_frame_side(f, Bs);
    Bs.n_kf_nodes = extra[c].is_bad ? 0 : cands[c].n_nodes;                  // if(pKF->isBad()) vbDiscarded[i] = true: no search (:1869-1870)
    const RefKeyframeUp::Query q = U[c].dev(B, Bs);
    Bs.nnratio = 0.75f; Bs.check_orientation = 1;                            // ORBmatcher matcher(0.75,true) (:1853)
    Bs.taken = B.dev(taken) + (size_t)c * nt;
    const size_t ck = (size_t)c * nt;
    B.host(aps)[c] = ApplyDev{R.m_has + ck, R.m_world + 3 * ck, R.m_id + ck, R.m_obs + ck, q.pos, q.id, q.obs, R.m_cnt + 4 * c, 0, 0};
    B.host(cand)[c] = CandDev{n, 0, q.id, B.dev(W[c].skip)};
    // the two projected searches of the slot: matcher2(0.9,true).SearchByProjection(F, pKF, sFound, 10, 100) and (.., 3, 64)
    const SearchScratch& ss = W[c].search;
    for (int k = 0; k < 2; k++) {
      const int32_t* run_k = R.run + (k == 0 ? RUN_S1 : RUN_S2) * K + c;
      B.host(proj[k])[c] = RelocProjSlot{n, 0, q.pos, B.dev(U[c].maxd), B.dev(U[c].mind), B.dev(W[c].skip), B.dev(U[c].ang), B.dev(ss.qrec), R.s_view + c, run_k};
      const ApplyDev ap{R.s_has + ck, R.s_world + 3 * ck, R.s_id + ck, R.s_obs + ck, q.pos, q.id, q.obs, (k == 0 ? R.cnt1 : R.cnt2) + 4 * c, 0, 0};
      orbs_fill_problem_reloc(f, n, R.s_has + ck, B.dev(ss.qrec), B.dev(U[c].pdesc), ss.out(B), B.dev(ss.cache), k == 0 ? 100 : 64,
                              RunIf{run_k, 1, 0}, ap, B.host(prob) + pstride * (size_t)(k * K + c));
    }
  }
  hipStream_t st = ctx->stream;
  s = stage_submit(S, st, 0, B); if (s) return s;

  // ---- the frame enters the routine holding nothing; SearchByBoW against every candidate
  s = track_reset_launch(st, S, B, H); if (s) return s;
  { const int nmax = std::max(std::max(nt, S->nl), 1); hipLaunchKernelGGL(reloc_record_clear_kernel, dim3((nmax + 255) / 256), dim3(256), 0, st, S->D); }
  S->stage1_queued = true; S->local_map_of = nullptr; S->n_in_view = 0; S->finish_ready = false; S->stage2_queued = false;
  LLD_HIP_TRY(hipMemsetAsync(B.d + o_zero, 0, zero_bytes, st));
  if (kn) LLD_HIP_TRY(hipMemsetAsync(B.dev(taken), 0xff, kn * 4, st));
  if (nt > 0 && nn_max > 0)
    hipLaunchKernelGGL(reloc_bow_match_kernel, dim3((nn_max + kMatchWaves - 1) / kMatchWaves, K), dim3(kMatchWaves * 64), 0, st, B.dev(bows));
  hipLaunchKernelGGL(reloc_bow_finish_kernel, dim3(K), dim3(kFinishThreads), 0, st, B.dev(bows), B.dev(aps));
  LLD_HIP_TRY(hipGetLastError());
  // ---- the counts (4 K bytes: word 0 of every candidate's ap_counts): the only transfer before the rounds
  int32_t* h_cnt = B2.host(h2_cnt);
  LLD_HIP_TRY(hipMemcpy2DAsync(h_cnt, 4, R.m_cnt, 16, 4, K, hipMemcpyDeviceToHost, st));
  LLD_HIP_TRY(hipStreamSynchronize(st));
  S->upload_pending[0] = false;
  std::vector<int32_t> n_corr(K, 0), off(K, 0);
  std::vector<uint32_t> seeds(K, 0);
  uint8_t* h_keep = B2.host(h2_keep);
  int n_kept = 0;
  for (int c = 0; c < K; c++) {
    const int nb = h_cnt[c];
    h_keep[c] = (!extra[c].is_bad && nb >= kMinBow) ? 1 : 0;
    n_corr[c] = h_keep[c] ? nb : 0; seeds[c] = extra[c].seed; n_kept += h_keep[c];
  }
  auto fill_out = [&](const int32_t* status, const int32_t* rec, const lld_frame_view* fv) {
    out->matched = status ? status[ST_MATCHED] : 0; out->winner = status && status[ST_MATCHED] ? status[ST_WINNER] : -1;
    out->round = status ? status[ST_ROUND] : 0; out->n_good = status ? status[ST_GOOD] : 0; out->n_rounds = status ? status[ST_ROUNDS] : 0; out->n_kept = n_kept;
    const lld_frame_view& V = out->matched ? *fv : *view;
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) out->Tcw[4 * i + j] = V.Rcw[3 * i + j]; out->Tcw[4 * i + 3] = V.tcw[i]; }
    out->Tcw[12] = 0.f; out->Tcw[13] = 0.f; out->Tcw[14] = 0.f; out->Tcw[15] = 1.f;
    for (int c = 0; c < K; c++) {
      const int32_t* r = rec ? rec + REC_INTS * c : nullptr;
      const bool attempted = r && r[REC_MASK] != 0;
      if (out->n_bow) out->n_bow[c] = h_cnt[c];
      if (out->discarded) out->discarded[c] = (!h_keep[c] || (r && r[REC_NO_MORE])) ? 1 : 0;
      if (out->rounds) out->rounds[c] = r ? r[REC_ROUNDS] : 0;
      if (out->n_good_last) out->n_good_last[c] = attempted ? r[REC_GOOD] : -1;
      if (out->rungs) out->rungs[c] = r ? r[REC_MASK] : 0;
      if (out->n_additional1) out->n_additional1[c] = r ? r[REC_ADD1] : 0;
      if (out->n_additional2) out->n_additional2[c] = r ? r[REC_ADD2] : 0;
    }
  };
  if (n_kept == 0) { fill_out(nullptr, nullptr, nullptr); return LLD_OK; }   // nCandidates == 0: the while loop is not entered (:1894)

  // ---- one PnPsolver per candidate (a discarded one has no correspondences and is never live), its slab filled by a kernel
  lld_pnp_batch* batch = nullptr;
  lld_pnp::SlabDev slab{};
  s = lld_pnp::batch_create_dev(ctx, K, n_corr.data(), nt, (float)P->cam.fx, (float)P->cam.fy, (float)P->cam.cx, (float)P->cam.cy, seeds.data(), pnp, &batch, &slab, off.data());
  if (s) return s;
  auto fail = [&](int status) { (void)hipStreamSynchronize(st); lld_pnp_batch_destroy(batch); return status; };
  R.pnp_res = lld_pnp::batch_results_dev(batch); R.pnp_flags = lld_pnp::batch_flags_dev(batch, 0);
  B2.stage(h2_off, off.data());
  if (hipMemcpyAsync(B.dev(keep), h_keep, K, hipMemcpyHostToDevice, st) != hipSuccess || hipMemcpyAsync(R.live, h_keep, K, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(B.dev(off_d), B2.host(h2_off), (size_t)K * 4, hipMemcpyHostToDevice, st) != hipSuccess) return fail(LLD_ERR_HIP);
  LevelTable sig2;
  for (int l = 0; l < LLD_ORB_MAX_LEVELS; l++) sig2.v[l] = f->sigma2[l];
  const KeypointsDev kp = resident_keypoints(f, false);
  hipLaunchKernelGGL(reloc_pnp_assemble_kernel, dim3(K), dim3(kAsmThreads), 0, st, R, B.dev(off_d), B.dev(keep), slab, kp.xy, kp.octave, sig2, pnp->th2);

  // ---- the rounds: iterate(5) on the live solvers, the gate, the ladder over the slots, the pick; one status word back
  PoseSlotsDev ps{};
  ps.n_slots = K; ps.nt = nt;
  ps.t_xy = kp.xy; ps.t_uright = kp.uright; ps.t_octave = kp.octave;
  ps.kp_has = R.s_has; ps.kp_world = R.s_world; ps.pose_qt = R.s_pose_qt; ps.cam = P->cam;
  for (int l = 0; l < LLD_ORB_MAX_LEVELS; l++) ps.inv_sigma2[l] = f->inv_sigma2[l];
  ps.kp_outlier = R.s_out; ps.pose_out = R.s_pose_out;
  auto pose_rung = [&](int run_index, int stage) {
    PoseSlotsDev q = ps; q.run = R.run + run_index * K;
    int r = pose_slots_launch(ctx, st, q, P->pose, B.dev(pwork)); if (r) return r;
    hipLaunchKernelGGL(reloc_after_pose_kernel, dim3(K), dim3(kSlotThreads), 0, st, R, C, stage);
    return LLD_OK;
  };
  auto search_rung = [&](int k, float th) {
    int r = orbs_project_reloc_slots(st, f, K, n_max, B.dev(proj[k]), th); if (r) return r;
    r = orbs_launch_n(ctx, st, f, B.dev(prob) + pstride * (size_t)(k * K), K); if (r) return r;
    hipLaunchKernelGGL(reloc_between_kernel, dim3((K + 63) / 64), dim3(64), 0, st, R, k + 1);
    return LLD_OK;
  };
  volatile int32_t* h_word = B2.host(h2_status);
  // every round a live solver either ends (bNoMore) or returned a pose after at least 5 more iterations; a stream of poses that never reach 50
  // inliers has no end in the reference either: the loop stops after max_iterations rounds
  const int max_rounds = pnp->max_iterations + kMaxRoundsSlack;
  for (int round = 1; round <= max_rounds; round++) {
    s = lld_pnp::batch_iterate_live(batch, 5, R.live); if (s) return fail(s);
    hipLaunchKernelGGL(reloc_gate_kernel, dim3(K), dim3(kSlotThreads), 0, st, R, C);
    if ((s = pose_rung(RUN_PO1, 1)) || (s = search_rung(0, 10.f)) || (s = pose_rung(RUN_PO2, 2)) || (s = search_rung(1, 3.f)) || (s = pose_rung(RUN_PO3, 3))) return fail(s);
    hipLaunchKernelGGL(reloc_pick_kernel, dim3(1), dim3(kSlotThreads), 0, st, R, S->D, C, round);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(const_cast<int32_t*>(h_word), R.status + ST_WORD, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return fail(LLD_ERR_HIP);
    const int32_t word = *h_word;
    if (word < 0 || word == 0) break;                                        // bMatch, or nCandidates == 0
  }
  // ---- `out`
  if (hipMemcpyAsync(B2.host(h2_status), R.status, ST_INTS * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(B2.host(h2_rec), R.rec, (size_t)K * REC_INTS * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(B2.host(h2_view), S->D.view, sizeof(lld_frame_view), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(LLD_ERR_HIP);
  fill_out(B2.host(h2_status), B2.host(h2_rec), B2.host(h2_view));
  lld_pnp_batch_destroy(batch);
  return LLD_OK;
}
