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
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!keep[c]) return;
  const uint8_t* has = R.m_has + (size_t)c * R.nt;
  const float* world = R.m_world + 3 * (size_t)c * R.nt;
  const int per = (R.nt + kAsmThreads - 1) / kAsmThreads, k0 = min(tid * per, R.nt), k1 = min(k0 + per, R.nt);
  int cnt = 0;
  for (int k = k0; k < k1; k++) cnt += has[k] ? 1 : 0;
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; w++) base += wsum[w];
  int e = off[c] + base + incl - cnt;
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
  for (int off = 32; off > 0; off >>= 1) { n_pts += __shfl_xor(n_pts, off); n_map += __shfl_xor(n_map, off); }
  if ((tid & 63) == 0) { atomicAdd(&cnt_sh[0], n_pts); atomicAdd(&cnt_sh[1], n_map); }
  __syncthreads();
  if (tid == 0) {
    for (int i = 0; i < 7; i++) D.pose_qt[i] = R.s_pose_qt[7 * w + i];
    *D.view = R.s_view[w];
    line_camera_from_view(C, *D.view, D.line_params);
    const double* po = R.s_pose_out + 12 * (size_t)w;
    const int* pi = reinterpret_cast<const int*>(po + 8);
    RecHeader& H = *D.rec_h[0];
    for (int i = 0; i < 7; i++) H.pose_qt[i] = po[i];
    H.chi2 = po[7];
    H.i[RI_INL] = pi[0]; H.i[RI_ITS] = pi[1]; H.i[RI_TRIALS] = pi[2]; H.i[RI_EDGES] = pi[3]; H.i[RI_POINT_EDGES] = pi[4];
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
  fill_consts(S, f, P, view);
  const ViewConsts C = S->consts;

  // ---- layout: the uploaded block, then device-only state
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += al(bytes); return at; };
  const size_t o_pose = take(7 * 8), o_lp = take(sizeof(LineTrackDevParams)), o_view = take(sizeof(lld_frame_view));
  const size_t o_bows = take(sizeof(BowSearchDev) * K), o_aps = take(sizeof(ApplyDev) * K), o_cand = take(sizeof(CandDev) * K);
  const size_t o_proj1 = take(sizeof(RelocProjSlot) * K), o_proj2 = take(sizeof(RelocProjSlot) * K);
  const size_t pstride = orbs_problem_bytes();
  const size_t o_prob = take(pstride * 2 * K);
  struct CandUp { size_t desc, ang, id, pos, obs, node, start, feat, maxd, mind, pdesc; };
  std::vector<CandUp> U(K);
  for (int c = 0; c < K; c++) {
    const int n = cands[c].n, nn = cands[c].n_nodes;
    U[c].desc = take((size_t)n * 32); U[c].ang = take((size_t)n * 4); U[c].id = take((size_t)n * 4); U[c].pos = take((size_t)n * 12); U[c].obs = take(n);
    U[c].node = take((size_t)nn * 4); U[c].start = take((size_t)(nn + 1) * 4); U[c].feat = take((size_t)nv[c] * 4);
    U[c].maxd = take((size_t)n * 4); U[c].mind = take((size_t)n * 4);
    U[c].pdesc = extra[c].point_desc ? take((size_t)n * 32) : U[c].desc;
  }
  const size_t up_bytes = o;
  const size_t kn = (size_t)K * nt;
  // zeroed at the start of the call: match tables, counts, slots' flags and records
  const size_t o_zero = o;
  const size_t o_mhas = take(kn), o_mid = take(kn * 4), o_mobs = take(kn), o_mworld = take(kn * 12), o_mcnt = take((size_t)K * 16);
  const size_t o_run = take((size_t)N_RUN * K * 4), o_cnt1 = take((size_t)K * 16), o_cnt2 = take((size_t)K * 16), o_cur = take((size_t)K * 16);
  const size_t o_rec = take((size_t)K * REC_INTS * 4), o_status = take(ST_INTS * 4);
  const size_t zero_bytes = o - o_zero;
  const size_t o_taken = take(kn * 4);
  const size_t o_shas = take(kn), o_sid = take(kn * 4), o_sobs = take(kn), o_sworld = take(kn * 12), o_sout = take(kn);
  const size_t o_sqt = take((size_t)K * 7 * 8), o_spo = take((size_t)K * 12 * 8), o_sview = take(sizeof(lld_frame_view) * K);
  const size_t o_live = take(K), o_keep = take(K), o_off = take((size_t)K * 4);
  std::vector<size_t> o_skip(K), o_qrec(K), o_cache(K), o_so0(K), o_so1(K), o_so2(K), o_so3(K), o_so4(K), o_so5(K);
  for (int c = 0; c < K; c++) {
    const int n = cands[c].n;
    o_skip[c] = take(n); o_qrec[c] = take(orbs_qrec_bytes(n)); o_cache[c] = take(orbs_cache_bytes(n));
    o_so0[c] = take((size_t)n * 4); o_so1[c] = take((size_t)n * 4); o_so2[c] = take((size_t)n * 4); o_so3[c] = take(n); o_so4[c] = take((size_t)nt * 4); o_so5[c] = take(16);
  }
  const size_t o_pwork = take(pose_slots_work_bytes(K, nt));
  s = ensure_work(S, ctx, o); if (s) return s;
  s = ensure_stage(S, 0, up_bytes); if (s) return s;
  // the second pinned region: the small uploads after the counts are known, the status word, the final records
  const size_t h2_keep = 0, h2_off = al(K), h2_status = h2_off + al((size_t)K * 4), h2_cnt = h2_status + al(ST_INTS * 4), h2_rec = h2_cnt + al((size_t)K * 4),
               h2_view = h2_rec + al((size_t)K * REC_INTS * 4), h2_bytes = h2_view + al(sizeof(lld_frame_view));
  s = ensure_stage(S, 1, h2_bytes); if (s) return s;
  char* h = S->h_stage[0]; char* h2 = S->h_stage[1]; char* d = S->d_work;

  // ---- the device's view of everything
  RelocDev R{};
  R.K = K; R.nt = nt; R.cand = reinterpret_cast<const CandDev*>(d + o_cand);
  R.m_has = reinterpret_cast<uint8_t*>(d + o_mhas); R.m_id = reinterpret_cast<int32_t*>(d + o_mid); R.m_obs = reinterpret_cast<uint8_t*>(d + o_mobs);
  R.m_world = reinterpret_cast<float*>(d + o_mworld); R.m_cnt = reinterpret_cast<int32_t*>(d + o_mcnt);
  R.s_has = reinterpret_cast<uint8_t*>(d + o_shas); R.s_id = reinterpret_cast<int32_t*>(d + o_sid); R.s_obs = reinterpret_cast<uint8_t*>(d + o_sobs);
  R.s_world = reinterpret_cast<float*>(d + o_sworld); R.s_out = reinterpret_cast<uint8_t*>(d + o_sout);
  R.s_pose_qt = reinterpret_cast<double*>(d + o_sqt); R.s_pose_out = reinterpret_cast<double*>(d + o_spo); R.s_view = reinterpret_cast<lld_frame_view*>(d + o_sview);
  R.run = reinterpret_cast<int32_t*>(d + o_run); R.cnt1 = reinterpret_cast<int32_t*>(d + o_cnt1); R.cnt2 = reinterpret_cast<int32_t*>(d + o_cnt2);
  R.live = reinterpret_cast<uint8_t*>(d + o_live); R.cur = reinterpret_cast<int32_t*>(d + o_cur); R.rec = reinterpret_cast<int32_t*>(d + o_rec);
  R.status = reinterpret_cast<int32_t*>(d + o_status);

  // ---- pack
  std::memcpy(h + o_pose, pose_qt, 7 * 8);
  line_params_from_view(C, *view, reinterpret_cast<LineTrackDevParams*>(h + o_lp));
  std::memcpy(h + o_view, view, sizeof(lld_frame_view));
  const uint32_t* f_desc = reinterpret_cast<const uint32_t*>(f->d + f->o_td);
  const float* f_angle = reinterpret_cast<const float*>(f->d + f->o_tang);
  for (int c = 0; c < K; c++) {
    const lld_ref_keyframe& kf = cands[c];
    const int n = kf.n, nn = kf.n_nodes;
    if (n) {
      std::memcpy(h + U[c].desc, kf.desc, (size_t)n * 32); std::memcpy(h + U[c].ang, kf.angle, (size_t)n * 4); std::memcpy(h + U[c].id, kf.point_id, (size_t)n * 4);
      std::memcpy(h + U[c].pos, kf.world_pos, (size_t)n * 12);
      if (kf.has_obs) std::memcpy(h + U[c].obs, kf.has_obs, n); else std::memset(h + U[c].obs, 1, n);
      std::memcpy(h + U[c].maxd, extra[c].max_distance, (size_t)n * 4); std::memcpy(h + U[c].mind, extra[c].min_distance, (size_t)n * 4);
      if (extra[c].point_desc) std::memcpy(h + U[c].pdesc, extra[c].point_desc, (size_t)n * 32);
    }
    if (nn) { std::memcpy(h + U[c].node, kf.node, (size_t)nn * 4); std::memcpy(h + U[c].start, kf.node_start, (size_t)(nn + 1) * 4); }
    else std::memset(h + U[c].start, 0, 4);
    if (nv[c]) std::memcpy(h + U[c].feat, kf.feature, (size_t)nv[c] * 4);
    const int32_t* d_id = reinterpret_cast<const int32_t*>(d + U[c].id);
    const float* d_pos = reinterpret_cast<const float*>(d + U[c].pos);
    const uint8_t* d_obs = reinterpret_cast<const uint8_t*>(d + U[c].obs);
    BowSearchDev& B = reinterpret_cast<BowSearchDev*>(h + o_bows)[c];
    std::memset(&B, 0, sizeof(B));
    B.nt = nt; B.n_kf_nodes = extra[c].is_bad ? 0 : nn;                      // if(pKF->isBad()) vbDiscarded[i] = true: no search (:1869-1870)
    B.f_desc = f_desc; B.f_angle = f_angle;
    B.f_n_nodes = f->bow_n_nodes(); B.f_node = f->bow_node(); B.f_node_start = f->bow_node_start(); B.f_feature = f->bow_feature();
    B.kf_desc = reinterpret_cast<const uint32_t*>(d + U[c].desc); B.kf_angle = reinterpret_cast<const float*>(d + U[c].ang); B.kf_point_id = d_id;
    B.kf_node = reinterpret_cast<const int32_t*>(d + U[c].node); B.kf_node_start = reinterpret_cast<const int32_t*>(d + U[c].start);
    B.kf_feature = reinterpret_cast<const int32_t*>(d + U[c].feat);
    B.nnratio = 0.75f; B.check_orientation = 1;                              // ORBmatcher matcher(0.75,true) (:1853)
    B.taken = reinterpret_cast<int32_t*>(d + o_taken) + (size_t)c * nt;
    const size_t ck = (size_t)c * nt;
    reinterpret_cast<ApplyDev*>(h + o_aps)[c] = ApplyDev{R.m_has + ck, R.m_world + 3 * ck, R.m_id + ck, R.m_obs + ck, d_pos, d_id, d_obs, R.m_cnt + 4 * c, 0, 0};
    reinterpret_cast<CandDev*>(h + o_cand)[c] = CandDev{n, 0, d_id, reinterpret_cast<uint8_t*>(d + o_skip[c])};
    // the two projected searches of the slot: matcher2(0.9,true).SearchByProjection(F, pKF, sFound, 10, 100) and (.., 3, 64)
    const SearchOut so{reinterpret_cast<int32_t*>(d + o_so0[c]), reinterpret_cast<int32_t*>(d + o_so1[c]), reinterpret_cast<int32_t*>(d + o_so2[c]),
                       reinterpret_cast<uint8_t*>(d + o_so3[c]), reinterpret_cast<int32_t*>(d + o_so4[c]), reinterpret_cast<int32_t*>(d + o_so5[c])};
    for (int k = 0; k < 2; k++) {
      const int32_t* run = R.run + (k == 0 ? RUN_S1 : RUN_S2) * K + c;
      RelocProjSlot& ps = reinterpret_cast<RelocProjSlot*>(h + (k == 0 ? o_proj1 : o_proj2))[c];
      ps = RelocProjSlot{n, 0, d_pos, reinterpret_cast<const float*>(d + U[c].maxd), reinterpret_cast<const float*>(d + U[c].mind), reinterpret_cast<const uint8_t*>(d + o_skip[c]),
                         reinterpret_cast<const float*>(d + U[c].ang), d + o_qrec[c], R.s_view + c, run};
      const ApplyDev ap{R.s_has + ck, R.s_world + 3 * ck, R.s_id + ck, R.s_obs + ck, d_pos, d_id, d_obs, (k == 0 ? R.cnt1 : R.cnt2) + 4 * c, 0, 0};
      orbs_fill_problem_reloc(f, n, R.s_has + ck, d + o_qrec[c], reinterpret_cast<const uint32_t*>(d + U[c].pdesc), so, d + o_cache[c], k == 0 ? 100 : 64,
                              RunIf{run, 1, 0}, ap, h + o_prob + pstride * (size_t)(k * K + c));
    }
  }
  hipStream_t st = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, st));
  LLD_HIP_TRY(hipEventRecord(S->uploaded[0], st)); S->upload_pending[0] = true;

  // ---- the frame enters the routine holding nothing; SearchByBoW against every candidate
  s = track_reset_launch(st, S, reinterpret_cast<const double*>(d + o_pose), reinterpret_cast<const lld_frame_view*>(d + o_view),
                         reinterpret_cast<const LineTrackDevParams*>(d + o_lp)); if (s) return s;
  { const int nmax = std::max(std::max(nt, S->nl), 1); hipLaunchKernelGGL(reloc_record_clear_kernel, dim3((nmax + 255) / 256), dim3(256), 0, st, S->D); }
  S->stage1_queued = true; S->n_in_view = 0;
  LLD_HIP_TRY(hipMemsetAsync(d + o_zero, 0, zero_bytes, st));
  if (kn) LLD_HIP_TRY(hipMemsetAsync(d + o_taken, 0xff, kn * 4, st));
  if (nt > 0 && nn_max > 0)
    hipLaunchKernelGGL(reloc_bow_match_kernel, dim3((nn_max + kMatchWaves - 1) / kMatchWaves, K), dim3(kMatchWaves * 64), 0, st, reinterpret_cast<const BowSearchDev*>(d + o_bows));
  hipLaunchKernelGGL(reloc_bow_finish_kernel, dim3(K), dim3(kFinishThreads), 0, st, reinterpret_cast<const BowSearchDev*>(d + o_bows), reinterpret_cast<const ApplyDev*>(d + o_aps));
  LLD_HIP_TRY(hipGetLastError());
  // ---- the counts (4 K bytes: word 0 of every candidate's ap_counts): the only transfer before the rounds
  int32_t* h_cnt = reinterpret_cast<int32_t*>(h2 + h2_cnt);
  LLD_HIP_TRY(hipMemcpy2DAsync(h_cnt, 4, d + o_mcnt, 16, 4, K, hipMemcpyDeviceToHost, st));
  LLD_HIP_TRY(hipStreamSynchronize(st));
  S->upload_pending[0] = false;
  std::vector<int32_t> n_corr(K, 0), off(K, 0);
  std::vector<uint32_t> seeds(K, 0);
  uint8_t* h_keep = reinterpret_cast<uint8_t*>(h2 + h2_keep);
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
  std::memcpy(h2 + h2_off, off.data(), (size_t)K * 4);
  if (hipMemcpyAsync(d + o_keep, h2 + h2_keep, K, hipMemcpyHostToDevice, st) != hipSuccess || hipMemcpyAsync(d + o_live, h2 + h2_keep, K, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d + o_off, h2 + h2_off, (size_t)K * 4, hipMemcpyHostToDevice, st) != hipSuccess) return fail(LLD_ERR_HIP);
  LevelTable sig2;
  for (int l = 0; l < LLD_ORB_MAX_LEVELS; l++) sig2.v[l] = f->sigma2[l];
  hipLaunchKernelGGL(reloc_pnp_assemble_kernel, dim3(K), dim3(kAsmThreads), 0, st, R, reinterpret_cast<const int32_t*>(d + o_off), reinterpret_cast<const uint8_t*>(d + o_keep), slab,
                     reinterpret_cast<const float*>(f->d + f->o_txy), reinterpret_cast<const int32_t*>(f->d + f->o_toct), sig2, pnp->th2);

  // ---- the rounds: iterate(5) on the live solvers, the gate, the ladder over the slots, the pick; one status word back
  PoseSlotsDev ps{};
  ps.n_slots = K; ps.nt = nt;
  ps.t_xy = reinterpret_cast<const float*>(f->d + f->o_txy); ps.t_uright = f->has_uright ? reinterpret_cast<const float*>(f->d + f->o_tur) : nullptr;
  ps.t_octave = reinterpret_cast<const int32_t*>(f->d + f->o_toct);
  ps.kp_has = R.s_has; ps.kp_world = R.s_world; ps.pose_qt = R.s_pose_qt; ps.cam = P->cam;
  for (int l = 0; l < LLD_ORB_MAX_LEVELS; l++) ps.inv_sigma2[l] = f->inv_sigma2[l];
  ps.kp_outlier = R.s_out; ps.pose_out = R.s_pose_out;
  auto pose_rung = [&](int run_index, int stage) {
    PoseSlotsDev q = ps; q.run = R.run + run_index * K;
    int r = pose_slots_launch(ctx, st, q, P->pose, d + o_pwork); if (r) return r;
    hipLaunchKernelGGL(reloc_after_pose_kernel, dim3(K), dim3(kSlotThreads), 0, st, R, C, stage);
    return LLD_OK;
  };
  auto search_rung = [&](int k, float th) {
    int r = orbs_project_reloc_slots(st, f, K, n_max, reinterpret_cast<const RelocProjSlot*>(d + (k == 0 ? o_proj1 : o_proj2)), th); if (r) return r;
    r = orbs_launch_n(ctx, st, f, d + o_prob + pstride * (size_t)(k * K), K); if (r) return r;
    hipLaunchKernelGGL(reloc_between_kernel, dim3((K + 63) / 64), dim3(64), 0, st, R, k + 1);
    return LLD_OK;
  };
  volatile int32_t* h_word = reinterpret_cast<volatile int32_t*>(h2 + h2_status);
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
  if (hipMemcpyAsync(h2 + h2_status, R.status, ST_INTS * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(h2 + h2_rec, R.rec, (size_t)K * REC_INTS * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(h2 + h2_view, S->D.view, sizeof(lld_frame_view), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(LLD_ERR_HIP);
  fill_out(reinterpret_cast<const int32_t*>(h2 + h2_status), reinterpret_cast<const int32_t*>(h2 + h2_rec), reinterpret_cast<const lld_frame_view*>(h2 + h2_view));
  lld_pnp_batch_destroy(batch);
  return LLD_OK;
}
