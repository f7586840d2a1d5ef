// lld_frame_track.hip — the Tracking thread's per-frame chain as ONE device-resident sequence (round 6, lld_frame_track_*).
//
// The reference runs on one Frame (stereo): TrackWithMotionModel = SearchByProjection(Current, Last) [twice if < 20 matches]
// (src/Tracking.cc:904-911) -> AddLinesFrom(mLastFrame.mvpMapLines) (:924) -> Optimizer::PoseOptimization (:937) -> discard of the outliers
// (:940-975); TrackLocalMap = SearchLocalPoints (:1133, :1613-1664) -> AddLinesFrom(local_lines) (:1140) -> PoseOptimization (:1152) ->
// statistics / discard (:1155-1187).  Between those calls the Frame carries mvpMapPoints, mvbOutlier, mvpMapLines, mvbOutlierLines and mTcw.
// Here they are device arrays of the resident lld_frame (lld_track_internal.h): every stage reads what the stage before it left in HBM
// and NOTHING travels to the host between the stages; the host uploads a stage's map-side inputs once, queues its kernels and returns.
// lld_frame_track_download fetches the per-stage records (one copy, one synchronisation).
//
//   keypoint k   kp_has[k] (mvpMapPoints[k] != NULL), kp_world[k] (its GetWorldPos), kp_id[k] (the caller's MapPoint id), kp_obs[k]
//                (Observations() > 0), kp_outlier[k] (mvbOutlier)
//   line i       ln_has[i], ln_x0 / ln_dir[i] (MapLine::GetMinimalPos), ln_id[i], ln_outlier[i]
//   per frame    pose_qt (double; what Converter::toSE3Quat(mTcw) hands PoseOptimization), the float view (Frame::UpdatePoseMatrices), the
//                ids of the MapPoints the outlier discard marked (mnLastFrameSeen = mnId, :949) and of the MapLines this frame already
//                tracked (tracked_last_id = mnId, :1117): SearchLocalPoints / AddLinesFrom skip them by id.
//
// Kernels of this file: the bookkeeping between the library's search / line / pose kernels (lld_orb_search.hip, lld_line_match.hip, lld_pose.hip),
// i.e. what the reference does in the few lines of C++ between its calls.  Host half of a stage: one UploadBlock (lld_upload_block.h) declares the
// uploaded arrays and the scratch behind them once, region structs (here and in lld_frame_track_state.h) lay out, pack and bind each group of
// arrays, stage_begin / stage_submit size the buffers and queue the one copy.
#include "lld_common.h"
#include "lld_device_math.h"
#include "lld_frame_track_state.h"
#include "lld_map_internal.h"
#include "lld_track_internal.h"
#include "lld_wave.h"

namespace {

using namespace lld_track;

// A new frame enters TrackWithMotionModel: no MapPoints (fill(..., NULL), :897), no outlier flags, nothing discarded or tracked yet.
__global__ void track_reset_kernel(TrackDev D, const double* pose_guess, const lld_frame_view* view_up, const LineTrackDevParams* lp_up) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { *D.view = *view_up; *D.line_params = *lp_up; }                 // the caller's view of the predicted pose (kept if PoseOptimization does not run)
  if (i < D.nt) { D.kp_has[i] = 0; D.kp_id[i] = -1; D.kp_obs[i] = 0; D.kp_outlier[i] = 0; }
  if (i < D.nl) { D.ln_has[i] = 0; D.ln_id[i] = -1; D.ln_outlier[i] = 0; }
  if (i < 7) D.pose_qt[i] = pose_guess[i];
  if (i == 0) { *D.n_discard = 0; *D.n_tracked = 0; }
  rec_headers_zero(D, i);
}

// The frame enters TrackLocalMap from a stage 1 that ran elsewhere (lld_frame_track_set_state): what that routine left in the frame.
struct HeldDev { const int32_t* kp_id; const float* kp_world; const uint8_t* kp_obs; const uint8_t* kp_out; const int32_t* seen; int n_seen;
                const int32_t* ln_id; const double* ln_x0; const double* ln_dir; const uint8_t* ln_out; const int32_t* tracked; int n_tracked; };
__global__ void track_load_kernel(TrackDev D, HeldDev U, const double* pose_qt, const lld_frame_view* view_up, const LineTrackDevParams* lp_up) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { *D.view = *view_up; *D.line_params = *lp_up; *D.n_discard = U.n_seen; }
  if (i < D.nt) {
    const int32_t id = U.kp_id[i];
    const bool has = id >= 0;
    D.kp_has[i] = has; D.kp_id[i] = has ? id : -1; D.kp_obs[i] = has ? U.kp_obs[i] : 0; D.kp_outlier[i] = U.kp_out[i];
    for (int c = 0; c < 3; c++) D.kp_world[3 * i + c] = has ? U.kp_world[3 * i + c] : 0.f;
  }
  if (i < U.n_seen) D.discard[i] = U.seen[i];
  if (i < D.nl) {
    const int32_t id = U.ln_id[i];
    const bool has = id >= 0;
    D.ln_has[i] = has; D.ln_id[i] = has ? id : -1; D.ln_outlier[i] = U.ln_out[i];
    for (int c = 0; c < 3; c++) { D.ln_x0[3 * i + c] = has ? U.ln_x0[3 * i + c] : 0.0; D.ln_dir[3 * i + c] = has ? U.ln_dir[3 * i + c] : 0.0; }
  }
  if (i < U.n_tracked) D.tracked[i] = U.tracked[i];
  if (i == 0) *D.n_tracked = U.n_tracked;
  if (i < 7) D.pose_qt[i] = pose_qt[i];
  rec_headers_zero(D, i);
  if (i < D.nt) { D.rec_kp_id[0][i] = -1; D.rec_kp_out[0][i] = 0; }
  if (i < D.nl) { D.rec_ln_id[0][i] = -1; D.rec_ln_out[0][i] = 0; }
}

// What follows PoseOptimization.  stage 0 = TrackWithMotionModel (src/Tracking.cc:940-975): an outlier point leaves the frame, its flag is
// cleared, its MapPoint is marked seen (-> the discard list); an outlier line leaves, its flag STAYS (the reference does not clear
// mvbOutlierLines).  stage 1 = TrackLocalMap (:1155-1187): outlier points leave (STEREO) with their flag kept, outlier lines leave.
// Before any of it the stage's record is written: ids as matched, flags as PoseOptimization left them.  One workgroup.
__global__ __launch_bounds__(1024) void track_after_pose_kernel(TrackDev D, ViewConsts C, int stage) {
  __shared__ int cnt[8];
  const int tid = threadIdx.x;
  if (tid < 8) cnt[tid] = 0;
  __syncthreads();
  // the last wavefront's first lane turns the optimised pose into the frame's float view while the other fifteen walk the keypoints and lines
  // (a chain of ~500 dependent fp64 instructions behind one global load: it would otherwise follow the walk's own chain of loads)
  constexpr int kWalk = 960;
  if (tid == kWalk) {
    const int* pi = reinterpret_cast<const int*>(D.pose_out + 8);
    rec_header_from_pose(*D.rec_h[stage], D.pose_out);
    // pFrame->SetPose(pose) - unless PoseOptimization returned before it optimised (fewer than three points, Optimizer.cc:809-810)
    if (pi[4] >= 3) view_from_pose(D.pose_out, C, D.view, D.line_params, D.pose_qt);
  }
  int n_pts = 0, n_map = 0, n_disc = 0, n_lm = 0, n_ln = 0;
  for (int k0 = 0; k0 < D.nt && tid < kWalk; k0 += 2 * kWalk) {
    // two keypoints per lane, every load issued before the first use
    const int ka = k0 + tid, kb = ka + kWalk;
    const bool ina = ka < D.nt, inb = kb < D.nt;
    const int kca = ina ? ka : 0, kcb = inb ? kb : 0;
    const uint8_t ha = D.kp_has[kca], hb = D.kp_has[kcb], oa = D.kp_outlier[kca], ob = D.kp_outlier[kcb], va = D.kp_obs[kca], vb = D.kp_obs[kcb];
    const int32_t ia = D.kp_id[kca], ib = D.kp_id[kcb];
    auto one = [&](int k, bool in, uint8_t has_, uint8_t out_, uint8_t obs_, int32_t id_) {
      if (!in) return;
      const bool has = has_ != 0;
      const uint8_t bad = has ? out_ : 0;
      D.rec_kp_id[stage][k] = has ? id_ : -1;
      D.rec_kp_out[stage][k] = bad;
      if (!has) return;
      if (bad) {
        if (stage == 0) { const int at = atomicAdd(D.n_discard, 1); D.discard[at] = id_; D.kp_outlier[k] = 0; }
        D.kp_has[k] = 0; D.kp_id[k] = -1;
        n_disc++;
      } else { n_pts++; if (obs_) n_map++; }
    };
    one(ka, ina, ha, oa, va, ia); one(kb, inb, hb, ob, vb, ib);
  }
  for (int i = tid; i < D.nl && tid < kWalk; i += kWalk) {
    const uint8_t has_ = D.ln_has[i], out_ = D.ln_outlier[i]; const int32_t id_ = D.ln_id[i];
    const bool has = has_ != 0;
    D.rec_ln_id[stage][i] = has ? id_ : -1;
    D.rec_ln_out[stage][i] = has ? out_ : 0;
    if (!has) continue;
    n_lm++;
    if (out_) { D.ln_has[i] = 0; D.ln_id[i] = -1; } else n_ln++;
  }
  // wavefront sums first: five LDS atomics per wavefront instead of per lane
  lld_wave::sum_each(n_pts, n_map, n_disc, n_lm, n_ln);
  if ((tid & 63) == 0) { atomicAdd(&cnt[0], n_pts); atomicAdd(&cnt[1], n_map); atomicAdd(&cnt[2], n_disc); atomicAdd(&cnt[3], n_lm); atomicAdd(&cnt[4], n_ln); }
  __syncthreads();
  if (tid == 0) {
    RecHeader& H = *D.rec_h[stage];
    H.i[RI_POINTS] = cnt[0]; H.i[RI_POINTS_MAP] = cnt[1]; H.i[RI_DISCARDED] = cnt[2]; H.i[RI_LINES_MATCHED] = cnt[3]; H.i[RI_LINES] = cnt[4];
  }
}

// SearchLocalPoints' "already seen in this frame" (src/Tracking.cc:1616-1643): pMP->mnLastFrameSeen == mCurrentFrame.mnId holds for the
// MapPoints the frame holds (:1629) and for those the outlier discard marked (:949).  Ids are the caller's (>= 0).  Lines: tracked_last_id ==
// mnId (:1023) against the list of lines assigned so far.
constexpr int kSeenThreads = 1024;
// One workgroup: the ids the frame holds or discarded (and the lines it tracked) go into two open-addressing hash sets in LDS (at most half
// full: ids >= 0, -1 = empty), then every local MapPoint / MapLine probes its id.
__global__ __launch_bounds__(kSeenThreads) void track_mark_seen_kernel(TrackDev D, int n_mp, const int32_t* mp_id, const uint8_t* mp_skip, uint8_t* mp_skip_out,
                                                                      int n_ml, const int32_t* ml_id, const uint8_t* ml_skip, uint8_t* ml_skip_out, unsigned pmask, unsigned lmask) {
  extern __shared__ int32_t seen_tab[];              // [pmask + 1] point ids, then [lmask + 1] line ids
  int32_t* ptab = seen_tab; int32_t* ltab = seen_tab + pmask + 1;
  const int tid = threadIdx.x;
  for (unsigned k = tid; k < pmask + 1 + lmask + 1; k += kSeenThreads) seen_tab[k] = -1;
  const int nd = *D.n_discard, ntr = min(*D.n_tracked, D.tracked_cap);
  __syncthreads();
  for (int k = tid; k < D.nt; k += kSeenThreads) if (D.kp_has[k]) seen_insert(ptab, pmask, D.kp_id[k]);
  for (int k = tid; k < nd; k += kSeenThreads) seen_insert(ptab, pmask, D.discard[k]);
  for (int k = tid; k < ntr; k += kSeenThreads) seen_insert(ltab, lmask, D.tracked[k]);
  __syncthreads();
  for (int q = tid; q < n_mp; q += kSeenThreads) mp_skip_out[q] = ((mp_skip && mp_skip[q]) || seen_lookup(ptab, pmask, mp_id[q])) ? 1 : 0;
  for (int j = tid; j < n_ml; j += kSeenThreads) ml_skip_out[j] = ((ml_skip && ml_skip[j]) || seen_lookup(ltab, lmask, ml_id[j])) ? 1 : 0;
}

// LDS of track_mark_seen_kernel for a frame: the point table holds the ids the frame holds or discarded (<= 2 nt), the line table the tracked
// list (<= tracked_cap = 2 nl + 16), each at most half full.  Fixed per frame: sized once by state_build.
constexpr size_t kSeenLdsMax = 150 * 1024;
unsigned seen_pow2(unsigned n) { unsigned p = 64; while (p < n) p <<= 1; return p; }
unsigned seen_point_slots(int nt) { return seen_pow2(4u * (unsigned)std::max(nt, 1)); }
unsigned seen_line_slots(int nl) { return seen_pow2(2u * (unsigned)(2 * nl + 16)); }
// The most frame lines the chain takes next to nt keypoints: the LDS above, and pose_track_launch's 16384 (its line scan keeps the edge flags in LDS).
int track_max_lines(int nt) {
  const size_t left = kSeenLdsMax / 4 - seen_point_slots(nt);
  size_t lsize = 64;
  while (2 * lsize <= left) lsize <<= 1;
  return std::min((int)(lsize / 4) - 8, 16 * 1024);                       // seen_line_slots(nl) <= lsize  <=>  4 nl + 32 <= lsize
}

}  // namespace

namespace lld_track {
void state_free(lld_frame* f) {
  lld_frame_track_state* S = f->track;
  if (!S) return;
  if (S->d_state) (void)hipFree(S->d_state);
  if (S->d_work) (void)hipFree(S->d_work);
  for (int s = 0; s < 2; s++) { if (S->h_stage[s]) (void)hipHostFree(S->h_stage[s]); if (S->uploaded[s]) (void)hipEventDestroy(S->uploaded[s]); }
  if (S->h_rec) (void)hipHostFree(S->h_rec);
  delete S;
  f->track = nullptr;
}

int ensure_stage(lld_frame_track_state* S, int s, size_t bytes) {
  if (S->upload_pending[s]) { LLD_HIP_TRY(hipEventSynchronize(S->uploaded[s])); S->upload_pending[s] = false; }   // (long complete: the previous frame's copy)
  if (bytes <= S->h_stage_bytes[s]) return LLD_OK;
  if (S->h_stage[s]) LLD_HIP_TRY(hipHostFree(S->h_stage[s]));
  S->h_stage[s] = nullptr; S->h_stage_bytes[s] = 0;
  const size_t want = bytes + (bytes >> 2) + 4096;
  LLD_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S->h_stage[s]), want, hipHostMallocDefault));
  S->h_stage_bytes[s] = want;
  return LLD_OK;
}

int stage_begin(lld_frame_track_state* S, lld_ctx* ctx, int s, UploadBlock& B) {
  if (B.size > S->work_bytes) {                                  // grow-only d_work
    LLD_HIP_TRY(hipStreamSynchronize(ctx->stream));                // kernels of an earlier stage may still read the old block
    if (S->d_work) LLD_HIP_TRY(hipFree(S->d_work));
    S->d_work = nullptr; S->work_bytes = 0;
    const size_t want = B.size + (B.size >> 2) + 4096;
    if (hipMalloc(reinterpret_cast<void**>(&S->d_work), want) != hipSuccess) return LLD_ERR_ALLOC;
    S->work_bytes = want;
  }
  const int st = ensure_stage(S, s, B.up_bytes); if (st) return st;
  B.bind(S->h_stage[s], S->d_work);
  return LLD_OK;
}
int stage_submit(lld_frame_track_state* S, hipStream_t st, int s, const UploadBlock& B) {
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, st));
  LLD_HIP_TRY(hipEventRecord(S->uploaded[s], st)); S->upload_pending[s] = true;
  return LLD_OK;
}

void fill_consts(lld_frame_track_state* S, const lld_track_params* P, const lld_frame_view* view) {
  ViewConsts& C = S->consts;
  C.fx = view->fx; C.fy = view->fy; C.cx = view->cx; C.cy = view->cy; C.bf = view->bf;
  C.min_x = view->min_x; C.max_x = view->max_x; C.min_y = view->min_y; C.max_y = view->max_y; C.log_scale_factor = view->log_scale_factor; C.n_levels = view->n_levels;
  C.b = (double)(view->bf / view->fx);                                      // mb = mbf / fx, floats (src/Frame.cc:97)
  C.thr_base = P->line_thr_reproj_base; C.sx = S->sx; C.sy = S->sy; C.monocular = P->monocular; C.use_grid = P->line_use_grid;
}

}  // namespace lld_track

namespace {

// lld_frame_build_lines with no right lines: every left line is unmatched (-1, "no distance").
__global__ void lines_unmatched_kernel(int n, int32_t* __restrict__ match, double* __restrict__ dist) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { match[i] = -1; dist[i] = 1.7976931348623157e308; }
}

// The fresh state f->track points at: keypoint-side arrays, the frame's lines (copied from `L`, may be null: a frame without lines), the records.
// Synchronous (it is part of uploading a new frame, like lld_frame_create).  An error return leaves it half built: state_build takes it apart.
// With `Bd` (lld_frame_build_lines; L is then null) the lines come with BOTH descriptor sets in one copy from the frame's own pinned staging,
// line_matches is what the stereo matcher's kernels write, and nothing waits: the chain follows on the stream.
int state_fill(lld_frame* f, const lld_frame_lines* L, const lld_frame_lines_build* Bd) {
  lld_ctx* ctx = f->ctx;
  lld_frame_track_state* S = f->track;
  const int nt = f->nt, nl = Bd ? Bd->n_left : L ? L->n_left : 0, nr = Bd ? Bd->n_right : L ? L->n_right : 0, dim = Bd ? Bd->dim : L ? L->dim : 1;
  S->nl = nl; S->nr = nr; S->dim = dim; S->sx = Bd ? Bd->sx : L ? L->sx : 1.0; S->sy = Bd ? Bd->sy : L ? L->sy : 1.0;
  const int tracked_cap = 2 * nl + 16;
  S->seen_psize = seen_point_slots(nt); S->seen_lsize = seen_line_slots(nl);
  S->seen_lds = ((size_t)S->seen_psize + S->seen_lsize) * 4;
  if (S->seen_lds > kSeenLdsMax) return LLD_ERR_UNSUPPORTED;                                     // (lld_frame_set_lines refuses such frames first)
  // the attribute belongs to the kernel, not to the frame: raised to the budget, so that no frame's setting can shrink another's
  if (S->seen_lds > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(&track_mark_seen_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSeenLdsMax) != hipSuccess) return LLD_ERR_HIP;
  UploadBlock B;                                     // device only
  const auto has = B.take<uint8_t>(nt); const auto world = B.take<float>(nt, 3); const auto id = B.take<int32_t>(nt); const auto obs = B.take<uint8_t>(nt), out = B.take<uint8_t>(nt);
  const auto disc = B.take<int32_t>((size_t)nt + 1); const auto lhas = B.take<uint8_t>(nl); const auto lx0 = B.take<double>(nl, 3), ldir = B.take<double>(nl, 3);
  const auto lid = B.take<int32_t>(nl); const auto lout = B.take<uint8_t>(nl); const auto trk = B.take<int32_t>(tracked_cap), cnt = B.take<int32_t>(16);   // cnt: n_discard, n_tracked
  const auto pose = B.take<double>(7), pout = B.take<double>(12); const auto view = B.take<lld_frame_view>(1); const auto lp = B.take<LineTrackDevParams>(1);
  UploadBlock LB;                                    // the frame's lines, a block of their own inside the state: they arrive in one copy
  const auto ll = LB.take<float>(nl, 4); const auto lo = LB.take<int32_t>(nl); const auto lr = LB.take<float>(std::max(nr, 1), 4); const auto ro = LB.take<int32_t>(std::max(nr, 1));
  Span<int32_t> lm; Span<float> ld, rd; Span<double> md;
  if (!Bd) { lm = LB.take<int32_t>(nl); ld = LB.take<float>(nl, dim); LB.end_upload(); }
  else {
    // the right descriptors ride in the same copy and are dead once the match is made (the state keeps their nr * dim * 4 bytes allocated);
    // line_matches | match_dist behind the upload, contiguous: lld_frame_lines_download fetches both in one copy
    ld = LB.take<float>(nl, dim); rd = LB.take<float>(nr, dim); LB.end_upload();
    lm = LB.take<int32_t>(nl); md = LB.take<double>(nl);
  }
  const auto lc = LB.take<int32_t>(nl); const auto lines = B.take<char>(LB.size);
  S->rec_off = B.size;
  Span<RecHeader> rh[2]; Span<int32_t> rk[2], rl[2]; Span<uint8_t> rko[2], rlo[2];
  for (int s = 0; s < 2; s++) { rh[s] = B.take<RecHeader>(1); rk[s] = B.take<int32_t>(nt); rko[s] = B.take<uint8_t>(nt); rl[s] = B.take<int32_t>(nl); rlo[s] = B.take<uint8_t>(nl); }
  S->rec_bytes = B.size - S->rec_off;
  if (hipMalloc(reinterpret_cast<void**>(&S->d_state), B.size + 256) != hipSuccess) { S->d_state = nullptr; return LLD_ERR_ALLOC; }
  B.bind(nullptr, S->d_state);
  TrackDev& D = S->D;
  D.nt = nt; D.nl = nl; D.nr = nr; D.dim = dim;
  D.kp_has = B.dev(has); D.kp_world = B.dev(world); D.kp_id = B.dev(id); D.kp_obs = B.dev(obs); D.kp_outlier = B.dev(out);
  D.discard = B.dev(disc); D.n_discard = B.dev(cnt);
  D.ln_has = B.dev(lhas); D.ln_x0 = B.dev(lx0); D.ln_dir = B.dev(ldir); D.ln_id = B.dev(lid); D.ln_outlier = B.dev(lout);
  D.tracked = B.dev(trk); D.n_tracked = B.dev(cnt) + 1; D.tracked_cap = tracked_cap;
  D.pose_qt = B.dev(pose); D.pose_out = B.dev(pout); D.view = B.dev(view); D.line_params = B.dev(lp);
  for (int s = 0; s < 2; s++) { D.rec_h[s] = B.dev(rh[s]); D.rec_kp_id[s] = B.dev(rk[s]); D.rec_kp_out[s] = B.dev(rko[s]); D.rec_ln_id[s] = B.dev(rl[s]); D.rec_ln_out[s] = B.dev(rlo[s]); }
  LB.bind(nullptr, B.dev(lines));
  S->ln_left = LB.dev(ll); S->ln_loct = LB.dev(lo); S->ln_right = LB.dev(lr); S->ln_roct = LB.dev(ro); S->ln_match = LB.dev(lm); S->ln_desc = LB.dev(ld); S->ln_cell = LB.dev(lc);
  S->ln_mdist = Bd ? LB.dev(md) : nullptr; S->match_bytes = Bd ? (md.off - lm.off) + (size_t)nl * 8 : (size_t)nl * 4;
  LLD_HIP_TRY(hipMemsetAsync(B.d, 0, B.size, ctx->stream));
  if (Bd && nl > 0) {
    if (LB.up_bytes > f->h_lines_bytes) {
      // (no copy can be reading the old staging: a frame that had lines had a state, and replacing a state waits for the stream first)
      if (f->h_lines) LLD_HIP_TRY(hipHostFree(f->h_lines));
      f->h_lines = nullptr; f->h_lines_bytes = 0;
      auto& kept = ctx->line_staging;                                          // a buffer a destroyed frame handed back, if one is large enough
      for (size_t k = 0; k < kept.size() && !f->h_lines; k++)
        if (kept[k].second >= LB.up_bytes) { f->h_lines = kept[k].first; f->h_lines_bytes = kept[k].second; kept.erase(kept.begin() + k); }
      if (!f->h_lines) {
        const size_t want = LB.up_bytes + (LB.up_bytes >> 2) + 4096;
        if (hipHostMalloc(&f->h_lines, want, hipHostMallocDefault) != hipSuccess) { f->h_lines = nullptr; return LLD_ERR_ALLOC; }
        f->h_lines_bytes = want;
      }
    }
    void* d_match_work = nullptr;
    if (nr > 0) { const int st = lld_ctx_scratch(ctx, line_work_bytes(nl, nr), &d_match_work); if (st) return st; }   // device scratch: ordered by the stream
    LB.bind(static_cast<char*>(f->h_lines), LB.d);
    std::memset(LB.h, 0, LB.up_bytes);
    LB.stage(ll, Bd->left); LB.stage(lo, Bd->left_octave); LB.stage(ld, Bd->desc_left);
    if (nr > 0) { LB.stage(lr, Bd->right); LB.stage(ro, Bd->right_octave); LB.stage(rd, Bd->desc_right); }
    LLD_HIP_TRY(hipMemcpyAsync(LB.d, LB.h, LB.up_bytes, hipMemcpyHostToDevice, ctx->stream));
    int st = line_cells_dev(ctx->stream, S->ln_left, nl, S->sx, S->sy, S->ln_cell); if (st) return st;
    if (nr > 0) {
      const LineStereoDev in{nl, nr, dim, S->ln_left, S->ln_loct, S->ln_right, S->ln_roct, S->ln_desc, LB.dev(rd)};
      st = line_stereo_launch_dev(ctx->stream, Bd->stereo, in, d_match_work, LB.dev(lm), LB.dev(md)); if (st) return st;
    } else {
      hipLaunchKernelGGL(lines_unmatched_kernel, dim3((nl + 255) / 256), dim3(256), 0, ctx->stream, nl, LB.dev(lm), LB.dev(md));
      LLD_HIP_TRY(hipGetLastError());
    }
  } else if (nl > 0) {
    // the lines travel through the context's pinned staging (synchronous: the staging is the context's)
    void* hb; int st = lld_ctx_pinned(ctx, LB.up_bytes, &hb); if (st) return st;
    LB.bind(static_cast<char*>(hb), LB.d);
    std::memset(LB.h, 0, LB.up_bytes);
    LB.stage(ll, L->left); LB.stage(lo, L->left_octave);
    if (nr > 0) { LB.stage(lr, L->right); LB.stage(ro, L->right_octave); }
    LB.stage(lm, L->line_matches); LB.stage(ld, L->desc);
    LLD_HIP_TRY(hipMemcpyAsync(LB.d, LB.h, LB.up_bytes, hipMemcpyHostToDevice, ctx->stream));
    st = line_cells_dev(ctx->stream, S->ln_left, nl, S->sx, S->sy, S->ln_cell); if (st) return st;
  }
  if (!Bd) LLD_HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < 2; s++) LLD_HIP_TRY(hipEventCreateWithFlags(&S->uploaded[s], hipEventDisableTiming));
  return LLD_OK;
}

// (Re)builds the device state of a frame.  Every failure leaves the frame without one (hipFree waits for what state_fill queued on the block).
int state_build(lld_frame* f, const lld_frame_lines* L, const lld_frame_lines_build* Bd = nullptr) {
  lld_track::state_free(f);
  f->track = new lld_frame_track_state();
  const int st = state_fill(f, L, Bd);
  if (st) {
    if (Bd) (void)hipStreamSynchronize(f->ctx->stream);                      // the queued copy must have left the frame's staging before a next call packs it
    lld_track::state_free(f);
  }
  return st;
}

// The map lines of a stage (the last frame's, the local map's), then AddLinesFrom's matches behind the uploaded prefix.
struct LinesUp {
  int n = 0; Span<double> x0, dir, x1, x2; Span<uint8_t> skip; Span<float> desc; Span<int32_t> id, matches;
  void reserve(UploadBlock& B, int n_map, int dim) {
    n = n_map; x0 = B.take<double>(n, 3); dir = B.take<double>(n, 3); x1 = B.take<double>(n, 3); x2 = B.take<double>(n, 3);
    skip = B.take<uint8_t>(n); desc = B.take<float>(n, dim); id = B.take<int32_t>(n);
  }
  void reserve_scratch(UploadBlock& B) { matches = B.take<int32_t>(std::max(n, 1)); }
  void stage(const UploadBlock& B, const lld_map_lines* ML) const {
    if (!n) return;
    B.stage(x0, ML->x0); B.stage(dir, ML->dir); B.stage(x1, ML->x1); B.stage(x2, ML->x2); B.stage(skip, ML->skip, 0); B.stage(desc, ML->desc); B.stage(id, ML->id);
  }
  LineMapDev dev(const UploadBlock& B, const uint8_t* d_skip) const { return {n, B.dev(x0), B.dev(dir), B.dev(x1), B.dev(x2), d_skip, B.dev(desc)}; }
};

// mLastFrame's MapPoints as TrackWithMotionModel's SearchByProjection reads them, their descriptors and the caller's ids.
struct LastPointsUp {
  Span<float> pos, ang; Span<uint8_t> val, obs; Span<int32_t> oct, id; Span<uint32_t> desc;
  void reserve(UploadBlock& B, int nq) {
    pos = B.take<float>(nq, 3); val = B.take<uint8_t>(nq); oct = B.take<int32_t>(nq); ang = B.take<float>(nq); obs = B.take<uint8_t>(nq);
    desc = B.take<uint32_t>(nq, 8); id = B.take<int32_t>(nq);
  }
  void stage(const UploadBlock& B, const lld_last_frame_points* last, const int32_t* ids) const {
    B.stage(pos, last->world_pos); B.stage(val, last->valid); B.stage(oct, last->octave); B.stage(ang, last->angle, 0); B.stage(obs, last->has_obs, 1); B.stage(desc, last->desc); B.stage(id, ids);
  }
  LastFrameDev dev(const UploadBlock& B) const { return {(int)val.n, B.dev(pos), B.dev(val), B.dev(oct), B.dev(ang), B.dev(obs)}; }
};

// The local map's MapPoints as SearchLocalPoints reads them; skip2 (device only) = the caller's skip bytes or "already seen in this frame".
struct LocalPointsUp {
  Span<float> pos, nrm, maxd, mind; Span<uint8_t> obs, skip, skip2; Span<uint32_t> desc; Span<int32_t> id;
  void reserve(UploadBlock& B, int nq) {
    pos = B.take<float>(nq, 3); nrm = B.take<float>(nq, 3); maxd = B.take<float>(nq); mind = B.take<float>(nq); obs = B.take<uint8_t>(nq); skip = B.take<uint8_t>(nq);
    desc = B.take<uint32_t>(nq, 8); id = B.take<int32_t>(nq);
  }
  void reserve_scratch(UploadBlock& B) { skip2 = B.take<uint8_t>(skip.n); }
  void stage(const UploadBlock& B, const lld_map_points* mp, const int32_t* ids) const {
    B.stage(pos, mp->world_pos); B.stage(nrm, mp->normal); B.stage(maxd, mp->max_distance); B.stage(mind, mp->min_distance);
    B.stage(obs, mp->has_obs, 1); B.stage(skip, mp->skip, 0); B.stage(desc, mp->desc); B.stage(id, ids);
  }
  MapPointsDev dev(const UploadBlock& B) const { return {(int)skip.n, B.dev(pos), B.dev(nrm), B.dev(maxd), B.dev(mind), B.dev(obs), B.dev(skip2)}; }
};

// What a stage 1 that ran elsewhere left in the frame (lld_frame_held); trk: the held lines' ids, then the caller's further tracked ones.
struct HeldUp {
  int nl = 0, n_seen = 0, n_trk = 0; Span<int32_t> id, seen, lid, trk; Span<float> w; Span<uint8_t> obs, out, lout; Span<double> lx0, ldir;
  void reserve(UploadBlock& B, int nt, int nl_, int n_seen_, int n_trk_) {
    nl = nl_; n_seen = n_seen_; n_trk = n_trk_;
    id = B.take<int32_t>(nt); w = B.take<float>(nt, 3); obs = B.take<uint8_t>(nt); out = B.take<uint8_t>(nt); seen = B.take<int32_t>(std::max(n_seen, 1));
    lid = B.take<int32_t>(nl); lx0 = B.take<double>(nl, 3); ldir = B.take<double>(nl, 3); lout = B.take<uint8_t>(nl); trk = B.take<int32_t>(std::max(n_trk, 1));
  }
  void stage(const UploadBlock& B, const lld_frame_held* held) const {
    B.stage(id, held->kp_point_id); B.stage(w, held->kp_world_pos); B.stage(obs, held->kp_has_obs, 1); B.stage(out, held->kp_outlier, 0);
    if (n_seen) B.stage(seen, held->seen_point_id);
    if (!nl) return;
    const int32_t* lines = held->ln_line_id;                                  // null: the frame holds no lines (every id -1)
    B.stage(lid, lines, 0xff); B.stage(lx0, lines ? held->ln_x0 : nullptr, 0); B.stage(ldir, lines ? held->ln_dir : nullptr, 0); B.stage(lout, held->ln_outlier, 0);
    int32_t* t = B.host(trk); int at = 0;
    if (lines) for (int i = 0; i < nl; i++) if (lines[i] >= 0) t[at++] = lines[i];                     // a line the frame holds was tracked by it (tracked_last_id, :1117)
    for (int k = 0; k < held->n_tracked; k++) t[at++] = held->tracked_line_id[k];
  }
  HeldDev dev(const UploadBlock& B) const { return {B.dev(id), B.dev(w), B.dev(obs), B.dev(out), B.dev(seen), n_seen, B.dev(lid), B.dev(lx0), B.dev(ldir), B.dev(lout), B.dev(trk), nl ? n_trk : 0}; }
};

// lines half of a stage: AddLinesFrom on the uploaded map lines (skip bytes at `d_skip`), then the assignment into the frame
int run_lines(lld_frame* f, hipStream_t st, const lld_track_params* P, const UploadBlock& B, const LinesUp& U, const uint8_t* d_skip, void* d_line_work) {
  lld_frame_track_state* S = f->track;
  if (U.n <= 0 || S->nl <= 0) return LLD_OK;
  LineFrameDev Cur{S->nl, S->ln_left, S->ln_loct, S->ln_right, S->ln_match, S->D.ln_has, S->ln_cell, S->ln_desc, S->dim};
  const LineApplyDev ap{S->D.ln_has, S->D.ln_x0, S->D.ln_dir, S->D.ln_id, S->D.tracked, S->D.n_tracked, S->D.tracked_cap, B.dev(U.id)};
  return line_track_launch_dev(st, S->D.line_params, U.dev(B, d_skip), Cur, P->line_md_thr, d_line_work, B.dev(U.matches), ap);
}

int run_pose(lld_frame* f, hipStream_t st, const lld_track_params* P, void* d_pose_work, int stage) {
  lld_frame_track_state* S = f->track;
  const KeypointsDev K = resident_keypoints(f, false);
  PoseTrackDev in{};
  in.nt = f->nt; in.nl = S->nl;
  in.t_xy = K.xy; in.t_uright = K.uright; in.t_octave = K.octave;
  in.kp_has = S->D.kp_has; in.kp_world = S->D.kp_world;
  in.ln_left = S->ln_left; in.ln_loct = S->ln_loct; in.ln_right = S->ln_right; in.ln_roct = S->ln_roct; in.ln_match = S->ln_match;
  in.ln_has = S->D.ln_has; in.ln_x0 = S->D.ln_x0; in.ln_dir = S->D.ln_dir;
  in.pose_qt = S->D.pose_qt; in.cam = P->cam; in.gamma = P->pose.gamma;
  for (int l = 0; l < LLD_ORB_MAX_LEVELS; l++) in.inv_sigma2[l] = f->inv_sigma2[l];
  in.kp_outlier = S->D.kp_outlier; in.ln_outlier = S->D.ln_outlier; in.pose_out = S->D.pose_out;
  int s = pose_track_launch(f->ctx, st, in, P->pose, d_pose_work); if (s) return s;
  hipLaunchKernelGGL(track_after_pose_kernel, dim3(1), dim3(1024), 0, st, S->D, S->consts, stage);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

int check_lines(const lld_map_lines* ML) {
  if (!ML || ML->n == 0) return LLD_OK;
  return (ML->n < 0 || !ML->x0 || !ML->dir || !ML->x1 || !ML->x2 || !ML->desc || !ML->id) ? LLD_ERR_INVALID : LLD_OK;
}

// Stage 2 on nq local MapPoints and n_map local MapLines.  From the host (`map` null): the arrays travel in the stage's one upload.  From the
// resident map: only the search's problem record travels, a kernel of lld_map.hip fills the same buffers from the tables, and the entries
// behind the device-side counts are skipped entries.
// After an overflow of UpdateLocalMap the resident route must leave the frame as it found it, and it does so WITHOUT a predicate in the
// kernels below: the gather empties kp_has / ln_has and skips every entry, restore_launch puts the two tables back and blanks the record.
// That rests on every kernel between the two being a no-op on a frame that holds nothing and a local map of skipped entries:
//   track_mark_seen_kernel    writes only its own skip2 scratch;
//   the projection and orb_search_kernel   no query survives: nothing is applied to kp_has / kp_id / kp_world / kp_obs;
//   the line kernels          every map line is skipped: no assignment, n_tracked unchanged;
//   pose_track_launch         no edge: no flag is written, pose_out reports fewer than three point edges;
//   track_after_pose_kernel   nothing held: no discard; fewer than three edges: view, line camera and pose_qt stay.
// A kernel added to this stage that writes frame state regardless of what is held breaks that: give it the status word instead.
int local_map_stage(lld_frame* f, const lld_track_params* P, int nq, int n_map, const lld_map_points* mp, const int32_t* point_id, const lld_map_lines* local_lines,
                    const lld_map* map) {
  lld_frame_track_state* S = f->track; lld_ctx* ctx = f->ctx;
  const int nt = f->nt;
  // stage 2 reuses the work block from its start: stage 1's kernels are queued before this upload on the same stream, and stage_begin
  // synchronises the stream before it grows the block
  UploadBlock B; LocalPointsUp MPU; LinesUp U; SearchScratch sc;
  const auto prob = B.take<char>(orbs_problem_bytes());
  if (map) B.end_upload();
  MPU.reserve(B, nq); U.reserve(B, n_map, S->dim);
  if (!map) B.end_upload();
  U.reserve_scratch(B); MPU.reserve_scratch(B);
  const auto lskip2 = B.take<uint8_t>(std::max(n_map, 1)), inview = B.take<uint8_t>(std::max(nq, 1));
  sc.reserve(B, nq, nt);
  const auto lwork = B.take<char>(line_work_bytes(n_map, S->nl)), pwork = B.take<char>(pose_track_work_bytes(nt, S->nl));
  const auto bk_kp = B.take<uint8_t>(map ? nt : 0), bk_ln = B.take<uint8_t>(map ? S->nl : 0);
  int s = stage_begin(S, ctx, 1, B); if (s) return s;
  if (!map) { MPU.stage(B, mp, point_id); U.stage(B, local_lines); }
  const MapPointsDev MP = MPU.dev(B);
  const ApplyDev ap{S->D.kp_has, S->D.kp_world, S->D.kp_id, S->D.kp_obs, MP.pos, B.dev(MPU.id), MP.has_obs, S->D.rec_h[1]->i + RI_SEARCH1, 0, 0};
  orbs_fill_problem(f, 1, nq, S->D.kp_has, B.dev(sc.qrec), B.dev(MPU.desc), sc.out(B), B.dev(sc.cache), P->nnratio_local, 0, RunIf{}, ap, B.host(prob));
  hipStream_t st = ctx->stream;
  s = stage_submit(S, st, 1, B); if (s) return s;
  // ---- kernels
  lld_map_dev::GatherDst G{};
  if (map) {
    G.nt = nt; G.nl = S->nl;
    G.pos = B.dev(MPU.pos); G.nrm = B.dev(MPU.nrm); G.maxd = B.dev(MPU.maxd); G.mind = B.dev(MPU.mind); G.obs = B.dev(MPU.obs); G.skip = B.dev(MPU.skip);
    G.desc = B.dev(MPU.desc); G.id = B.dev(MPU.id);
    if (n_map > 0) { G.x0 = B.dev(U.x0); G.dir = B.dev(U.dir); G.x1 = B.dev(U.x1); G.x2 = B.dev(U.x2); G.lskip = B.dev(U.skip); G.ldesc = B.dev(U.desc); G.lid = B.dev(U.id); }
    G.kp_has = S->D.kp_has; G.ln_has = S->D.ln_has; G.bk_kp = B.dev(bk_kp); G.bk_ln = B.dev(bk_ln);
    G.rec2 = reinterpret_cast<int32_t*>(S->D.rec_h[1]); G.n_rec2 = (int)(sizeof(RecHeader) / 4);
    s = lld_map_dev::gather_launch(st, map, G); if (s) return s;
  }
  if (nq + n_map > 0)                                                          // (tables sized by state_build)
    hipLaunchKernelGGL(track_mark_seen_kernel, dim3(1), dim3(kSeenThreads), S->seen_lds, st, S->D, nq, B.dev(MPU.id), B.dev(MPU.skip), B.dev(MPU.skip2), n_map, B.dev(U.id),
                       B.dev(U.skip), B.dev(lskip2), S->seen_psize - 1, S->seen_lsize - 1);
  S->in_view_off = inview.off; S->n_in_view = nq;
  s = orbs_project_local_points(st, f->consts, nullptr, S->D.view, MP, P->viewing_cos_limit, P->th_local, B.dev(sc.qrec),
                                FrustumOut{B.dev(inview), nullptr, nullptr, nullptr, S->D.rec_h[1]->i + RI_IN_VIEW}); if (s) return s;
  s = orbs_launch_n(ctx, st, f, B.dev(prob), 1); if (s) return s;
  s = run_lines(f, st, P, B, U, B.dev(lskip2), B.dev(lwork)); if (s) return s;
  s = run_pose(f, st, P, B.dev(pwork), 1); if (s) return s;
  if (map) { s = lld_map_dev::restore_launch(st, map, G); if (s) return s; }
  S->finish_ready = true; S->stage2_queued = true;
  return LLD_OK;
}

}  // namespace

namespace lld_track {
int ensure_state(lld_frame* f) { return f->track ? LLD_OK : state_build(f, nullptr); }
int frame_max_lines(int nt) { return track_max_lines(nt); }
int frame_state_build_lines(lld_frame* f, const lld_frame_lines_build* Bd) { return state_build(f, nullptr, Bd); }
int ref_keyframe_check(const lld_ref_keyframe* kf, int* n_features) {
  const int n = kf->n, nn = kf->n_nodes;
  *n_features = 0;
  if (n < 0 || n > LLD_ORB_MAX_KEYPOINTS || nn < 0 || nn > n) return LLD_ERR_INVALID;
  if (n > 0 && (!kf->desc || !kf->angle || !kf->point_id || !kf->world_pos)) return LLD_ERR_INVALID;
  if (nn > 0 && (!kf->node || !kf->node_start || !kf->feature)) return LLD_ERR_INVALID;
  if (nn > 0) {
    if (kf->node_start[0] != 0) return LLD_ERR_INVALID;
    for (int i = 0; i < nn; i++) {
      if (kf->node_start[i + 1] < kf->node_start[i] || kf->node_start[i + 1] > n) return LLD_ERR_INVALID;   // a feature sits under one node
      if (i > 0 && kf->node[i] <= kf->node[i - 1]) return LLD_ERR_INVALID;
    }
    const int nv = kf->node_start[nn];
    for (int i = 0; i < nv; i++) if (kf->feature[i] < 0 || kf->feature[i] >= n) return LLD_ERR_INVALID;
    *n_features = nv;
  }
  return LLD_OK;
}
int track_reset_launch(hipStream_t st, lld_frame_track_state* S, const UploadBlock& B, const StageHeader& H) {
  const int nmax = std::max(std::max(S->D.nt, S->nl), 64);
  hipLaunchKernelGGL(track_reset_kernel, dim3((nmax + 255) / 256), dim3(256), 0, st, S->D, B.dev(H.pose), B.dev(H.view), B.dev(H.lp));
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}
}  // namespace lld_track

extern "C" {

void lld_track_params_default(lld_track_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  lld_pose_params_default(&p->pose);
  p->th_motion = 7.f; p->th_local = 1.f; p->nnratio_local = 0.8f; p->viewing_cos_limit = 0.5f;
  p->direction = 0; p->check_orientation = 1; p->wide_retry = 1; p->monocular = 0;
  p->line_thr_reproj_base = 2.0; p->line_md_thr = 0.9; p->line_use_grid = 1;
}

int lld_frame_set_lines(lld_frame* f, const lld_frame_lines* L) {
  if (!f) return LLD_ERR_INVALID;
  if (L) {
    if (L->n_left < 0 || L->n_right < 0 || L->dim <= 0 || L->dim > 128 || !(L->sx > 0) || !(L->sy > 0)) return LLD_ERR_INVALID;
    if (L->n_left > 0 && (!L->left || !L->left_octave || !L->line_matches || !L->desc)) return LLD_ERR_INVALID;
    if (L->n_right > 0 && (!L->right || !L->right_octave)) return LLD_ERR_INVALID;
    for (int i = 0; i < L->n_left; i++) {
      if (L->left_octave[i] < 0 || L->left_octave[i] > 64 || L->line_matches[i] >= L->n_right) return LLD_ERR_INVALID;
    }
    for (int i = 0; i < L->n_right; i++) if (L->right_octave[i] < 0 || L->right_octave[i] > 64) return LLD_ERR_INVALID;
    if (L->n_left > track_max_lines(f->nt)) return LLD_ERR_UNSUPPORTED;
  }
  LLD_HIP_TRY(hipSetDevice(f->ctx->device));
  LLD_HIP_TRY(hipStreamSynchronize(f->ctx->stream));
  return state_build(f, (L && L->n_left > 0) ? L : nullptr);
}

int lld_frame_track_motion_model(lld_frame* f, const lld_track_params* P, const lld_frame_view* view, const double* pose_qt, const lld_last_frame_points* last,
                                 const int32_t* last_point_id, const lld_map_lines* last_lines) {
  if (!f || !P || !view || !pose_qt || !last) return LLD_ERR_INVALID;
  const int nq = last->n, nt = f->nt;
  if (nq < 0 || (nq > 0 && (!last->world_pos || !last->valid || !last->octave || !last->desc || !last_point_id || (P->check_orientation && !last->angle)))) return LLD_ERR_INVALID;
  if (P->check_orientation && nt > 0 && !f->has_angle) return LLD_ERR_INVALID;
  if (view->n_levels != f->consts.n_levels) return LLD_ERR_INVALID;
  if (!(P->cam.fx > 0) || !(P->cam.fy > 0) || !f->has_inv_sigma2) return LLD_ERR_INVALID;   // PoseOptimization's intrinsics and information
  for (int i = 0; i < nq; i++) if (last->octave[i] < 0 || last->octave[i] >= f->consts.n_levels) return LLD_ERR_INVALID;
  lld_ctx* ctx = f->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  int s = ensure_state(f); if (s) return s;
  lld_frame_track_state* S = f->track;
  s = check_lines(last_lines); if (s) return s;
  const int n_map = (last_lines && S->nl > 0) ? last_lines->n : 0;
  fill_consts(S, P, view);
  // ---- layout of the uploaded block, then the device-only scratch behind it
  UploadBlock B; StageHeader H; LastPointsUp LP; LinesUp U; SearchScratch sc[2];
  const auto prob1 = B.take<char>(orbs_problem_bytes()), prob2 = B.take<char>(orbs_problem_bytes());
  H.reserve(B); LP.reserve(B, nq); U.reserve(B, n_map, S->dim);
  B.end_upload();
  U.reserve_scratch(B);
  sc[0].reserve(B, nq, nt); sc[1].reserve(B, nq, nt, &sc[0]);
  const auto lwork = B.take<char>(line_work_bytes(n_map, S->nl)), pwork = B.take<char>(pose_track_work_bytes(nt, S->nl));
  s = stage_begin(S, ctx, 0, B); if (s) return s;
  // ---- pack
  LP.stage(B, last, last_point_id); U.stage(B, last_lines); H.stage(B, S->consts, view, pose_qt);
  const SearchOut so[2] = {sc[0].out(B), sc[1].out(B)};
  const bool wide = P->wide_retry != 0;
  const RunIf gate{so[0].summary, 20, 1};                                     // if(nmatches<20) (src/Tracking.cc:907)
  const LastFrameDev LF = LP.dev(B);
  int32_t* counts = S->D.rec_h[0]->i + RI_SEARCH1;                            // RI_SEARCH1, RI_SEARCH, RI_WIDE are consecutive
  ApplyDev ap{S->D.kp_has, S->D.kp_world, S->D.kp_id, S->D.kp_obs, LF.pos, B.dev(LP.id), LF.has_obs, counts, wide ? 20 : 0, 0};
  char* qrec = B.dev(sc[0].qrec);
  orbs_fill_problem(f, 0, nq, S->D.kp_has, qrec, B.dev(LP.desc), so[0], B.dev(sc[0].cache), 0.f, P->check_orientation, RunIf{}, ap, B.host(prob1));
  ap.min_matches = 0; ap.is_retry = 1;
  orbs_fill_problem(f, 0, nq, S->D.kp_has, qrec, B.dev(LP.desc), so[1], B.dev(sc[0].cache), 0.f, P->check_orientation, gate, ap, B.host(prob2));
  hipStream_t st = ctx->stream;
  s = stage_submit(S, st, 0, B); if (s) return s;
  // ---- kernels
  s = track_reset_launch(st, S, B, H); if (s) return s;
  s = orbs_project_last_frame(st, f->consts, view, nullptr, LF, P->direction, P->th_motion, qrec, nullptr, RunIf{}); if (s) return s;
  s = orbs_launch_n(ctx, st, f, B.dev(prob1), 1); if (s) return s;
  if (wide) {
    s = orbs_project_last_frame(st, f->consts, view, nullptr, LF, P->direction, 2.f * P->th_motion, qrec, nullptr, gate); if (s) return s;
    s = orbs_launch_n(ctx, st, f, B.dev(prob2), 1); if (s) return s;
  }
  s = run_lines(f, st, P, B, U, B.dev(U.skip), B.dev(lwork)); if (s) return s;
  s = run_pose(f, st, P, B.dev(pwork), 0); if (s) return s;
  S->stage1_queued = true; S->local_map_of = nullptr; S->n_in_view = 0; S->finish_ready = false; S->stage2_queued = false;
  return LLD_OK;
}

// Tracking::TrackReferenceKeyFrame (src/Tracking.cc:773-817) as stage 1: SearchByBoW against the FeatureVector lld_frame_compute_bow left in the
// frame, mvpMapPoints = the matches, SetPose(mLastFrame.mTcw), PoseOptimization on the points alone, the discard of :796-814 (what
// track_after_pose_kernel does for stage 0: the flagged leave, their flag is cleared, their id is marked seen, nmatchesMap is counted).
int lld_frame_track_reference_keyframe(lld_frame* f, const lld_track_params* P, const lld_frame_view* view, const double* pose_qt, const lld_ref_keyframe* kf) {
  if (!f || !P || !view || !pose_qt || !kf) return LLD_ERR_INVALID;
  if (!f->has_bow) return LLD_ERR_INVALID;                                     // Frame::ComputeBoW comes first (:776)
  const int nt = f->nt;
  int nv = 0;
  if (int st = ref_keyframe_check(kf, &nv)) return st;
  if (nt > 0 && !f->has_angle) return LLD_ERR_INVALID;                         // ORBmatcher(0.7, true): mbCheckOrientation
  if (view->n_levels != f->consts.n_levels) return LLD_ERR_INVALID;
  if (!(P->cam.fx > 0) || !(P->cam.fy > 0) || !f->has_inv_sigma2) return LLD_ERR_INVALID;
  lld_ctx* ctx = f->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  int s = ensure_state(f); if (s) return s;
  lld_frame_track_state* S = f->track;
  fill_consts(S, P, view);
  UploadBlock B; StageHeader H; RefKeyframeUp KF;
  H.reserve(B); KF.reserve(B, *kf, nv);
  B.end_upload();
  const auto taken = B.take<int32_t>(nt); const auto pwork = B.take<char>(pose_track_work_bytes(nt, S->nl));
  s = stage_begin(S, ctx, 0, B); if (s) return s;
  H.stage(B, S->consts, view, pose_qt); KF.stage(B, *kf);
  hipStream_t st = ctx->stream;
  s = stage_submit(S, st, 0, B); if (s) return s;
  s = track_reset_launch(st, S, B, H); if (s) return s;
  BowSearchDev Bs{};
  bow_frame_side(f, Bs);
  Bs.n_kf_nodes = kf->n_nodes;
  const RefKeyframeUp::Query q = KF.dev(B, Bs);
  Bs.nnratio = 0.7f; Bs.check_orientation = 1;                                 // ORBmatcher matcher(0.7,true) (:780)
  Bs.taken = B.dev(taken);
  const ApplyDev ap{S->D.kp_has, S->D.kp_world, S->D.kp_id, S->D.kp_obs, q.pos, q.id, q.obs, S->D.rec_h[0]->i + RI_SEARCH1, 0, 0};
  s = bow_search_launch(st, Bs, ap); if (s) return s;
  s = run_pose(f, st, P, B.dev(pwork), 0); if (s) return s;                    // (no AddLinesFrom: track_reset_launch left the line tables empty)
  S->stage1_queued = true; S->local_map_of = nullptr; S->n_in_view = 0; S->finish_ready = false; S->stage2_queued = false;
  return LLD_OK;
}

int lld_frame_track_set_state(lld_frame* f, const lld_track_params* P, const lld_frame_view* view, const double* pose_qt, const lld_frame_held* held) {
  if (!f || !P || !view || !pose_qt || !held) return LLD_ERR_INVALID;
  const int nt = f->nt;
  if (view->n_levels != f->consts.n_levels) return LLD_ERR_INVALID;
  if (!(P->cam.fx > 0) || !(P->cam.fy > 0) || !f->has_inv_sigma2) return LLD_ERR_INVALID;
  if (nt > 0 && (!held->kp_point_id || !held->kp_world_pos)) return LLD_ERR_INVALID;
  if (held->n_seen < 0 || held->n_seen > nt || (held->n_seen > 0 && !held->seen_point_id)) return LLD_ERR_INVALID;   // the outlier discard marks at most one MapPoint per keypoint
  lld_ctx* ctx = f->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  int s = ensure_state(f); if (s) return s;
  lld_frame_track_state* S = f->track;
  const int nl = S->nl;
  if (nl > 0 && held->ln_line_id && (!held->ln_x0 || !held->ln_dir)) return LLD_ERR_INVALID;
  int n_held_lines = 0;
  if (nl > 0 && held->ln_line_id) for (int i = 0; i < nl; i++) n_held_lines += held->ln_line_id[i] >= 0;
  if (held->n_tracked < 0 || (held->n_tracked > 0 && !held->tracked_line_id) || n_held_lines + held->n_tracked > S->D.tracked_cap - nl) return LLD_ERR_INVALID;
  for (int k = 0; k < held->n_seen; k++) if (held->seen_point_id[k] < 0) return LLD_ERR_INVALID;
  for (int k = 0; k < held->n_tracked; k++) if (held->tracked_line_id[k] < 0) return LLD_ERR_INVALID;
  fill_consts(S, P, view);
  const int n_trk = n_held_lines + held->n_tracked;
  UploadBlock B; StageHeader H; HeldUp U;
  H.reserve(B); U.reserve(B, nt, nl, held->n_seen, n_trk);
  B.end_upload();                                                              // everything travels
  s = stage_begin(S, ctx, 0, B); if (s) return s;
  H.stage(B, S->consts, view, pose_qt); U.stage(B, held);
  hipStream_t st = ctx->stream;
  s = stage_submit(S, st, 0, B); if (s) return s;
  const int nmax = std::max(std::max(std::max(nt, nl), n_trk), 64);
  hipLaunchKernelGGL(track_load_kernel, dim3((nmax + 255) / 256), dim3(256), 0, st, S->D, U.dev(B), B.dev(H.pose), B.dev(H.view), B.dev(H.lp));
  LLD_HIP_TRY(hipGetLastError());
  S->stage1_queued = true; S->local_map_of = nullptr; S->n_in_view = 0; S->finish_ready = true; S->stage2_queued = false;
  return LLD_OK;
}

int lld_frame_track_local_map(lld_frame* f, const lld_track_params* P, const lld_map_points* mp, const int32_t* point_id, const lld_map_lines* local_lines) {
  if (!f || !P || !mp) return LLD_ERR_INVALID;
  lld_frame_track_state* S = f->track;
  if (!S || !S->stage1_queued) return LLD_ERR_INVALID;                        // the frame's pose and MapPoints come from lld_frame_track_motion_model
  const int nq = mp->n;
  if (nq < 0 || (nq > 0 && (!mp->world_pos || !mp->normal || !mp->max_distance || !mp->min_distance || !mp->desc || !point_id))) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(f->ctx->device));
  int s = check_lines(local_lines); if (s) return s;
  const int n_map = (local_lines && S->nl > 0) ? local_lines->n : 0;
  return local_map_stage(f, P, nq, n_map, mp, point_id, local_lines, nullptr);
}

int lld_frame_track_local_map_resident(lld_frame* f, const lld_track_params* P, lld_map* map) {
  if (!f || !P || !map) return LLD_ERR_INVALID;
  lld_frame_track_state* S = f->track;
  if (!S || !S->stage1_queued) return LLD_ERR_INVALID;
  const lld_map_dev::Limits L = lld_map_dev::limits(map);
  if (L.ctx != f->ctx || (S->nl > 0 && S->dim != L.line_dim)) return LLD_ERR_INVALID;
  if (L.poisoned) return LLD_ERR_HIP;
  if (S->local_map_of != map || S->local_map_serial != L.serial) return LLD_ERR_INVALID;                         // the lists must be this frame's: UpdateLocalMap comes first (src/Tracking.cc:1131)
  LLD_HIP_TRY(hipSetDevice(f->ctx->device));
  return local_map_stage(f, P, L.max_local_points, S->nl > 0 ? L.max_local_lines : 0, nullptr, nullptr, nullptr, map);
}

int lld_frame_track_download(lld_frame* f, lld_track_result* r1, lld_track_result* r2) {
  if (!f || !f->track || !f->track->stage1_queued) return LLD_ERR_INVALID;
  lld_frame_track_state* S = f->track; lld_ctx* ctx = f->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const bool want_view = r2 && r2->mp_in_view && S->n_in_view > 0;
  const size_t need = S->rec_bytes + (want_view ? (size_t)S->n_in_view : 0);
  if (need > S->h_rec_bytes) {
    if (S->h_rec) LLD_HIP_TRY(hipHostFree(S->h_rec));
    S->h_rec = nullptr; S->h_rec_bytes = 0;
    LLD_HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&S->h_rec), need + 4096, hipHostMallocDefault));
    S->h_rec_bytes = need + 4096;
  }
  LLD_HIP_TRY(hipMemcpyAsync(S->h_rec, S->d_state + S->rec_off, S->rec_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (want_view) LLD_HIP_TRY(hipMemcpyAsync(S->h_rec + S->rec_bytes, S->d_work + S->in_view_off, (size_t)S->n_in_view, hipMemcpyDeviceToHost, ctx->stream));
  LLD_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (want_view) std::memcpy(r2->mp_in_view, S->h_rec + S->rec_bytes, (size_t)S->n_in_view);
  const TrackDev& D = S->D;
  lld_track_result* rr[2] = {r1, r2};
  for (int s = 0; s < 2; s++) {
    lld_track_result* r = rr[s];
    if (!r) continue;
    auto at = [&](const void* dev) { return S->h_rec + (static_cast<const char*>(dev) - (S->d_state + S->rec_off)); };
    const RecHeader* H = reinterpret_cast<const RecHeader*>(at(D.rec_h[s]));
    std::memcpy(r->pose_qt, H->pose_qt, sizeof r->pose_qt); r->chi2 = H->chi2;
    r->n_inliers = H->i[RI_INL]; r->lm_iterations = H->i[RI_ITS]; r->lm_trials = H->i[RI_TRIALS]; r->n_edges = H->i[RI_EDGES];
    r->n_search_first = H->i[RI_SEARCH1]; r->n_search = H->i[RI_SEARCH]; r->used_wide = H->i[RI_WIDE]; r->n_points = H->i[RI_POINTS];
    r->n_points_map = H->i[RI_POINTS_MAP]; r->n_lines_matched = H->i[RI_LINES_MATCHED]; r->n_lines = H->i[RI_LINES]; r->n_discarded = H->i[RI_DISCARDED];
    r->n_point_edges = H->i[RI_POINT_EDGES]; r->n_in_view = H->i[RI_IN_VIEW];
    if (r->kp_point_id && D.nt) std::memcpy(r->kp_point_id, at(D.rec_kp_id[s]), (size_t)D.nt * 4);
    if (r->kp_outlier && D.nt) std::memcpy(r->kp_outlier, at(D.rec_kp_out[s]), D.nt);
    if (r->ln_line_id && D.nl) std::memcpy(r->ln_line_id, at(D.rec_ln_id[s]), (size_t)D.nl * 4);
    if (r->ln_outlier && D.nl) std::memcpy(r->ln_outlier, at(D.rec_ln_out[s]), D.nl);
  }
  return LLD_OK;
}

}  // extern "C"

