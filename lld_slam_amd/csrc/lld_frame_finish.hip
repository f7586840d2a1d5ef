// lld_frame_finish.hip — the tail of Tracking::Track on the resident frame (src/Tracking.cc:429-476 and what it calls), and the two other places
// the reference makes stereo MapPoints from a Frame's depths, as ONE kernel on the arrays the chain left in HBM:
//   lld_frame_track_finish          clean VO matches (:446-453) -> NeedNewKeyFrame's close-point counts and decision (:1223-1310) ->
//                                   CreateNewKeyFrame's depth-ordered points (:1386-1430) when a keyframe is made -> the outlier drop (:472-476)
//   lld_frame_create_stereo_points  UpdateLastFrame's temporal points (:830-882) / StereoInitialization's points (:535-550)
// The three creation loops share one body: the keypoints with depth > 0 sorted as pair<float,int>, the walk that counts every visited entry
// and stops at the first far one past the hundredth, Frame::UnprojectStereo (src/Frame.cc:730-744).  A frame is one workgroup
// (nt <= LLD_ORB_MAX_KEYPOINTS): the pairs become 64-bit keys (float bits << 32 | index - positive floats order as their bit patterns, so one key
// sort IS the pair sort, ties by index and +inf last) sorted in LDS; the end of the walk is a minimum over the sorted list; the new ids are an
// exclusive scan of the creation flags in sorted order.  The decision is taken by one lane between the counts and the creation, which the
// workgroup then runs or skips: no host round trip.  The state is the chain's (lld_frame_track_state.h).
// Everything here is integer work or single-rounding float arithmetic: no contraction anywhere in this file, so the positions are those of
// tests/frame_finish_ref.py bit for bit.
#pragma clang fp contract(off)

#include <climits>

#include "lld_common.h"
#include "lld_device_math.h"
#include "lld_frame_track_state.h"
#include "lld_track_internal.h"
#include "lld_wave.h"

namespace {

using namespace lld_track;

constexpr int kFinThreads = 1024;
constexpr int kFinWaves = kFinThreads / 64;
constexpr int kFinMaxKeys = LLD_ORB_MAX_KEYPOINTS;                     // 4096 keys of 8 bytes: 32 KB of LDS
constexpr unsigned long long kNoKey = ~0ull;
enum { FIN_TRACK = 0, FIN_LAST_FRAME = 1, FIN_INITIALIZATION = 2 };
enum { SC_TRACKED = 0, SC_NON_TRACKED, SC_NEED, SC_INTERRUPT, SC_MADE, SC_VISITED, SC_CREATED, SC_COUNT = 8 };

struct DecisionIn {                                                    // NeedNewKeyFrame's scalars (lld_frame_finish_params)
  int32_t force, only_tracking, mapper_stopped, mapper_idle, keyframes_in_queue, set_not_stop_ok, monocular, max_frames, min_frames, n_keyframes,
          n_ref_matches, n_matches_inliers;
  int64_t frame_id, last_reloc_frame_id, last_keyframe_id;
};
struct FinishDev {
  int nt, n_keys, mode;                                                // n_keys: the power of two >= max(nt, 2) the sort works on
  int restore;                                                         // RGB-D: put back the outlier MapPoints stage 2 took out of the frame (:1171 removes them for STEREO only)
  const float* depth; const float* xy;                                 // mvDepth, mvKeysUn
  float th_depth, cx, cy, invfx, invfy;
  int32_t first_id;
  const double* pose_up; const lld_frame_view* view_up; const LineTrackDevParams* lp_up;   // LLD_POINTS_LAST_FRAME with a new pose, else null
  int32_t* scal; uint8_t* created; int32_t* new_id; float* x3d; int32_t* kp_point_id; int32_t* order;   // the block that travels back
};

// Tracking::NeedNewKeyFrame (src/Tracking.cc:1227-1309) after its counting loop, in the reference's types.  *interrupt: InterruptBA was called (:1296).
__device__ bool need_new_keyframe(const DecisionIn& p, int n_tracked_close, int n_non_tracked_close, int matches_inliers, int* interrupt) {
  *interrupt = 0;
  if (p.only_tracking) return false;                                                                              // :1227
  if (p.mapper_stopped) return false;                                                                             // :1231
  const int nKFs = p.n_keyframes;
  if (p.frame_id < p.last_reloc_frame_id + (int64_t)p.max_frames && nKFs > p.max_frames) return false;            // :1237
  const int nRefMatches = p.n_ref_matches;
  const bool idle = p.mapper_idle != 0;
  const bool mono = p.monocular != 0;
  const bool need_close = (n_tracked_close < 100) && (n_non_tracked_close > 70);                                  // :1266
  float thRefRatio = 0.75f;
  if (nKFs < 2) thRefRatio = 0.4f;
  if (mono) thRefRatio = 0.9f;
  const bool c1a = p.frame_id >= p.last_keyframe_id + (int64_t)p.max_frames;                                      // :1278
  const bool c1b = p.frame_id >= p.last_keyframe_id + (int64_t)p.min_frames && idle;                              // :1280
  const bool c1c = !mono && ((double)matches_inliers < (double)nRefMatches * 0.25 || need_close);                 // :1282
  const bool c2 = (((float)matches_inliers < (float)nRefMatches * thRefRatio) || need_close) && matches_inliers > 15;   // :1284
  if (!((c1a || c1b || c1c) && c2)) return false;
  if (idle) return true;                                                                                          // :1290
  *interrupt = 1;                                                                                                 // :1296
  return !mono && p.keyframes_in_queue < 3;                                                                       // :1297-1305
}

__global__ __launch_bounds__(kFinThreads) void frame_finish_kernel(TrackDev D, FinishDev A, DecisionIn P) {
  __shared__ unsigned long long key[kFinMaxKeys];
  __shared__ int cnt[4];                                               // tracked close, non-tracked close, candidates
  __shared__ int wave_new[kFinWaves];
  __shared__ int s_made, s_first_far;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nt = A.nt, mode = A.mode;
  if (tid < 4) cnt[tid] = 0;
  if (tid == 0) s_first_far = INT_MAX;
  if (A.view_up) {                                                     // mLastFrame.SetPose (:825): the view the walk un-projects with
    if (tid == 0) { *D.view = *A.view_up; *D.line_params = *A.lp_up; }
    if (tid < 7) D.pose_qt[tid] = A.pose_up[tid];
  }
  __syncthreads();
  // ---- 1. clean VO matches, 2. the close-point counts, and the sort keys of the candidates
  int n_tc = 0, n_ntc = 0, n_cand = 0;
  for (int k = tid; k < A.n_keys; k += kFinThreads) {
    unsigned long long kk = kNoKey;
    if (k < nt) {
      const float z = A.depth[k];
      bool has = D.kp_has[k] != 0;
      bool outl = D.kp_outlier[k] != 0;
      if (A.restore && !has && D.rec_kp_out[1][k]) {                   // stage 2's record: held and flagged when PoseOptimization returned
        has = true;
        D.kp_has[k] = 1; D.kp_id[k] = D.rec_kp_id[1][k];
      }
      if (mode == FIN_TRACK && has && !D.kp_obs[k]) {                  // :449-452
        has = false; outl = false;
        D.kp_has[k] = 0; D.kp_id[k] = -1; D.kp_outlier[k] = 0;
      }
      const bool positive = z > 0.0f;                                  // (false for NaN)
      if (mode == FIN_TRACK && !P.monocular && positive && z < A.th_depth) {   // :1256
        if (has && !outl) n_tc++; else n_ntc++;
      }
      if (positive) {
        n_cand++;
        kk = mode == FIN_INITIALIZATION ? (unsigned long long)k : (((unsigned long long)__float_as_uint(z) << 32) | (unsigned)k);
      }
      A.created[k] = 0; A.new_id[k] = -1; A.order[k] = -1;
      A.x3d[3 * k] = 0.f; A.x3d[3 * k + 1] = 0.f; A.x3d[3 * k + 2] = 0.f;
    }
    key[k] = kk;
  }
  lld_wave::sum_each(n_tc, n_ntc, n_cand);
  if (lane == 0) { atomicAdd(&cnt[0], n_tc); atomicAdd(&cnt[1], n_ntc); atomicAdd(&cnt[2], n_cand); }
  __syncthreads();
  // ---- 3. the decision
  if (tid == 0) {
    int need = 0, interrupt = 0, made = 1;
    if (mode == FIN_TRACK) {
      const int inliers = P.n_matches_inliers >= 0 ? P.n_matches_inliers : D.rec_h[1]->i[RI_POINTS_MAP];   // mnMatchesInliers (:1164)
      need = need_new_keyframe(P, cnt[0], cnt[1], inliers, &interrupt) ? 1 : 0;
      made = P.force >= 0 ? P.force : (need && P.set_not_stop_ok ? 1 : 0);                                  // :465, :1369
    }
    s_made = made;
    A.scal[SC_TRACKED] = cnt[0]; A.scal[SC_NON_TRACKED] = cnt[1]; A.scal[SC_NEED] = need; A.scal[SC_INTERRUPT] = interrupt; A.scal[SC_MADE] = made;
    A.scal[SC_VISITED] = 0; A.scal[SC_CREATED] = 0; A.scal[7] = 0;
  }
  __syncthreads();
  const int m = cnt[2];                                                // vDepthIdx.size()
  // ---- 4. the creation (the whole workgroup takes the same branch)
  if (s_made && m > 0) {
    lld_wave::bitonic_sort<kFinThreads>(key, A.n_keys);                // sort(vDepthIdx): the empty slots (all ones) last
    // the walk ends behind the first entry j with nPoints = j + 1 > 100 and depth > mThDepth (:1427); it is itself processed
    if (mode != FIN_INITIALIZATION) {
      int first = INT_MAX;
      for (int j = 100 + tid; j < m; j += kFinThreads)
        if (__uint_as_float((unsigned)(key[j] >> 32)) > A.th_depth) { first = j; break; }
      first = lld_wave::min(first);
      if (lane == 0 && first != INT_MAX) atomicMin(&s_first_far, first);
    }
    __syncthreads();
    const int n_visited = s_first_far < m ? s_first_far + 1 : m;
    const lld_frame_view V = *D.view;
    // the visited entries in sorted order: rank of a created point = created points before it (ballot in the wavefront, wavefront totals in LDS)
    int base = 0;
    for (int j0 = 0; j0 < n_visited; j0 += kFinThreads) {
      const int j = j0 + tid;
      const bool in = j < n_visited;
      const int i = in ? (int)(unsigned)(key[j] & 0xffffffffull) : 0;
      const bool c = in && (!D.kp_has[i] || !D.kp_obs[i]);             // :1404-1410
      const unsigned long long cm = __ballot(c);
      if (lane == 0) wave_new[w] = __popcll(cm);
      __syncthreads();
      int before = 0, total = 0;
      for (int q = 0; q < kFinWaves; q++) { const int v = wave_new[q]; if (q < w) before += v; total += v; }
      if (in) A.order[i] = j;
      if (c) {
        const int32_t id = A.first_id + base + before + __popcll(cm & ((1ull << lane) - 1ull));
        const float z = A.depth[i], u = A.xy[2 * i], v = A.xy[2 * i + 1];
        const float xc[3] = {(u - A.cx) * z * A.invfx, (v - A.cy) * z * A.invfy, z};                      // Frame.cc:737-739
        float x[3];
        lld::rwc_mul(V.Rcw, xc, x);
        for (int q = 0; q < 3; q++) { x[q] = x[q] + V.Ow[q]; A.x3d[3 * i + q] = x[q]; D.kp_world[3 * i + q] = x[q]; }   // :740
        A.created[i] = 1; A.new_id[i] = id;
        D.kp_has[i] = 1; D.kp_id[i] = id; D.kp_obs[i] = mode == FIN_LAST_FRAME ? 0 : 1;                    // a temporal point has no observation
      }
      base += total;
      __syncthreads();
    }
    if (tid == 0) { A.scal[SC_VISITED] = n_visited; A.scal[SC_CREATED] = base; }
  }
  __syncthreads();
  // ---- 5. the outlier drop (:472-476), and what the frame holds on exit
  for (int k = tid; k < nt; k += kFinThreads) {
    bool has = D.kp_has[k] != 0;
    if (mode == FIN_TRACK && has && D.kp_outlier[k]) { has = false; D.kp_has[k] = 0; D.kp_id[k] = -1; }
    A.kp_point_id[k] = has ? D.kp_id[k] : -1;
  }
}

struct PoseArg { const lld_track_params* params; const lld_frame_view* view; const double* pose_qt; };

// what lld_frame_track_set_state refuses about a pose handed in
bool pose_arg_ok(const lld_frame* f, const PoseArg& a) {
  if (!a.view && !a.pose_qt) return true;
  if (!a.view || !a.pose_qt || !a.params) return false;
  if (a.view->n_levels != f->consts.n_levels) return false;
  return a.params->cam.fx > 0 && a.params->cam.fy > 0 && f->has_inv_sigma2;
}

// Validated arguments -> one upload (pose header and host depths, when either travels), the kernel, one download, one wait.
int run_finish(lld_frame* f, int mode, float th_depth, int32_t first_id, const DecisionIn& dec, bool rgbd, const float* depth_host, const PoseArg& pose,
               lld_frame_finish_result* out) {
  lld_ctx* ctx = f->ctx;
  const int nt = f->nt;
  if (nt > kFinMaxKeys) return LLD_ERR_UNSUPPORTED;                    // (no frame is created above LLD_ORB_MAX_KEYPOINTS)
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const bool built = f->stereo_built || f->mono_built;
  if (!f->track) { const int st = ensure_state(f); if (st) return st; }
  lld_frame_track_state* S = f->track;
  if (pose.view) fill_consts(S, pose.params, pose.view);
  UploadBlock B; StageHeader H;
  if (pose.view) H.reserve(B);
  const auto dh = B.take<float>(built ? 0 : nt);
  B.end_upload();
  const auto scal = B.take<int32_t>(SC_COUNT); const auto cr = B.take<uint8_t>(nt); const auto nid = B.take<int32_t>(nt); const auto x3 = B.take<float>(nt, 3);
  const auto pid = B.take<int32_t>(nt), ord = B.take<int32_t>(nt);
  void* hb; int st = lld_ctx_pinned(ctx, B.size, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind(static_cast<char*>(hb), static_cast<char*>(db));
  hipStream_t sm = ctx->stream;
  if (B.up_bytes) {
    if (pose.view) H.stage(B, S->consts, pose.view, pose.pose_qt);
    B.stage(dh, depth_host);
    LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, sm));
  }
  if (mode == FIN_INITIALIZATION) {                                    // a new frame's state with the pose handed in (SetPose(eye), :526)
    st = track_reset_launch(sm, S, B, H); if (st) return st;
    S->stage1_queued = true; S->local_map_of = nullptr; S->n_in_view = 0; S->finish_ready = false; S->stage2_queued = false;
  }
  FinishDev A{};
  A.nt = nt; A.n_keys = 2; while (A.n_keys < nt) A.n_keys <<= 1;
  A.mode = mode; A.restore = (mode == FIN_TRACK && rgbd && S->stage2_queued) ? 1 : 0;
  A.depth = built ? reinterpret_cast<const float*>(f->d + f->o_depth) : B.dev(dh);
  A.xy = resident_keypoints(f, false).xy;
  const ViewConsts& C = S->consts;
  A.th_depth = th_depth; A.cx = C.cx; A.cy = C.cy; A.invfx = 1.0f / C.fx; A.invfy = 1.0f / C.fy;       // invfx = 1.0f/fx (src/Frame.cc:150-151)
  A.first_id = first_id;
  if (pose.view && mode == FIN_LAST_FRAME) { A.pose_up = B.dev(H.pose); A.view_up = B.dev(H.view); A.lp_up = B.dev(H.lp); }
  A.scal = B.dev(scal); A.created = B.dev(cr); A.new_id = B.dev(nid); A.x3d = B.dev(x3); A.kp_point_id = B.dev(pid); A.order = B.dev(ord);
  hipLaunchKernelGGL(frame_finish_kernel, dim3(1), dim3(kFinThreads), 0, sm, S->D, A, dec);
  LLD_HIP_TRY(hipGetLastError());
  if (pose.view && mode == FIN_LAST_FRAME) S->stage1_queued = true;
  if (A.restore) S->stage2_queued = false;                             // (what stage 2 took out is back, or gone for good: not twice)
  const size_t back = B.size - B.up_bytes;
  LLD_HIP_TRY(hipMemcpyAsync(B.h + B.up_bytes, B.d + B.up_bytes, back, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  const int32_t* sc = B.host(scal);
  out->n_tracked_close = sc[SC_TRACKED]; out->n_non_tracked_close = sc[SC_NON_TRACKED]; out->need = sc[SC_NEED]; out->interrupt_ba = sc[SC_INTERRUPT];
  out->made = sc[SC_MADE]; out->n_visited = sc[SC_VISITED]; out->n_created = sc[SC_CREATED]; out->reserved = 0;
  if (out->created && nt) std::memcpy(out->created, B.host(cr), (size_t)nt);
  if (out->new_id && nt) std::memcpy(out->new_id, B.host(nid), (size_t)nt * 4);
  if (out->x3d && nt) std::memcpy(out->x3d, B.host(x3), (size_t)nt * 12);
  if (out->kp_point_id && nt) std::memcpy(out->kp_point_id, B.host(pid), (size_t)nt * 4);
  if (out->order && nt) std::memcpy(out->order, B.host(ord), (size_t)nt * 4);
  return LLD_OK;
}

bool has_depth(const lld_frame* f, const float* depth_host) { return f->stereo_built || f->mono_built || depth_host || f->nt == 0; }
bool ids_fit(int32_t first_id, int nt) { return first_id >= 0 && (int64_t)first_id + (int64_t)nt <= (int64_t)INT32_MAX; }

}  // namespace

extern "C" {

int lld_frame_track_finish(lld_frame* f, const lld_frame_finish_params* p, lld_frame_finish_result* out) {
  if (!f || !p || !out) return LLD_ERR_INVALID;
  if (!f->track || !f->track->finish_ready) return LLD_ERR_INVALID;    // mnMatchesInliers, the view and mvbOutlier are TrackLocalMap's
  if (!has_depth(f, p->depth) || !(p->th_depth > 0) || !ids_fit(p->first_new_id, f->nt) || p->force < -1 || p->force > 1) return LLD_ERR_INVALID;
  DecisionIn d{};
  d.force = p->force; d.only_tracking = p->only_tracking; d.mapper_stopped = p->mapper_stopped; d.mapper_idle = p->mapper_idle;
  d.keyframes_in_queue = p->keyframes_in_queue; d.set_not_stop_ok = p->set_not_stop_ok; d.monocular = p->monocular; d.max_frames = p->max_frames;
  d.min_frames = p->min_frames; d.n_keyframes = p->n_keyframes; d.n_ref_matches = p->n_ref_matches; d.n_matches_inliers = p->n_matches_inliers;
  d.frame_id = p->frame_id; d.last_reloc_frame_id = p->last_reloc_frame_id; d.last_keyframe_id = p->last_keyframe_id;
  return run_finish(f, FIN_TRACK, p->th_depth, p->first_new_id, d, p->sensor_rgbd != 0, p->depth, PoseArg{nullptr, nullptr, nullptr}, out);
}

int lld_frame_create_stereo_points(lld_frame* f, const lld_frame_points_params* p, lld_frame_finish_result* out) {
  if (!f || !p || !out) return LLD_ERR_INVALID;
  if (p->mode != LLD_POINTS_LAST_FRAME && p->mode != LLD_POINTS_INITIALIZATION) return LLD_ERR_INVALID;
  const bool init = p->mode == LLD_POINTS_INITIALIZATION;
  const PoseArg pose{p->params, p->view, p->pose_qt};
  if (!has_depth(f, p->depth) || !ids_fit(p->first_new_id, f->nt) || !pose_arg_ok(f, pose)) return LLD_ERR_INVALID;
  if (init ? !p->view : (!(p->th_depth > 0) || (!p->view && !(f->track && f->track->stage1_queued)))) return LLD_ERR_INVALID;
  DecisionIn d{};
  d.force = -1;
  return run_finish(f, init ? FIN_INITIALIZATION : FIN_LAST_FRAME, init ? 1.0f : p->th_depth, p->first_new_id, d, false, p->depth, pose, out);
}

}  // extern "C"
