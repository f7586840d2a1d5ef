// lld_frame_lines.hip — the frame's lines without a host trip: lld_frame_build_lines (TwoFrameLineMatcher::MatchLines of src/Frame.cc:121-122
// on the frame, its result written where the chain reads Frame::line_matches), lld_frame_lines_download, and lld_frame_new_map_lines
// (Tracking::MatchLinesLastKF, src/Tracking.cc:1449-1611, between two resident frames).
//
// The matching kernels are lld_line_match.hip's (line_candidates_kernel, line_resolve_kernel, line_cells_kernel, line_lastkf_kernel), reached
// through lld_track_internal.h; the state is lld_frame_track.hip's (frame_state_build_lines).  The device code of this file is what the
// reference does around MatchLinesLastKF's loop: "was this line of the last frame tracked by the current one" (:1518) as an id look-up, and
// the numbering of the created MapLines in creation order (:1597-1606) with their entry into mCurrentFrame.mvpMapLines (:1602).
#include "lld_common.h"
#include "lld_frame_track_state.h"
#include "lld_track_internal.h"

namespace {

using namespace lld_track;

constexpr int kSkipThreads = 1024;
constexpr size_t kSkipLdsMax = 150 * 1024;               // the budget of TrackLocalMap's skip test, whose line table this kernel rebuilds

// last_skip[li] = mLastFrame.mvpMapLines[li] && its tracked_last_id == mCurrentFrame.mnId (src/Tracking.cc:1518): the current frame's tracked
// ids go into an open-addressing set in LDS (at most half full: lsize >= 2 * tracked_cap, as in track_mark_seen_kernel), then every line the
// last frame holds probes its id.  One workgroup.
__global__ __launch_bounds__(kSkipThreads) void lines_last_skip_kernel(const int32_t* __restrict__ cur_tracked, const int32_t* __restrict__ cur_n_tracked, int tracked_cap,
                                                                      int n_last, const uint8_t* __restrict__ last_has, const int32_t* __restrict__ last_id,
                                                                      uint8_t* __restrict__ skip, unsigned lmask) {
  extern __shared__ int32_t skip_tab[];                  // [lmask + 1]
  const int tid = threadIdx.x;
  for (unsigned k = tid; k < lmask + 1; k += kSkipThreads) skip_tab[k] = -1;
  const int ntr = min(*cur_n_tracked, tracked_cap);
  __syncthreads();
  for (int k = tid; k < ntr; k += kSkipThreads) { const int32_t id = cur_tracked[k]; if (id >= 0) seen_insert(skip_tab, lmask, id); }
  __syncthreads();
  for (int li = tid; li < n_last; li += kSkipThreads) skip[li] = (last_has[li] && last_id[li] >= 0 && seen_lookup(skip_tab, lmask, last_id[li])) ? 1 : 0;
}

// The created lines in ascending i get first_id + rank and enter the frame (mCurrentFrame.mvpMapLines[i] = ml, :1602); counts[0] = mapline_cnt,
// counts[1] = cnt0 (lines the frame held on entry: a created line was not held, :1477).  One workgroup; the rank of a line is the count of created
// lines before it: a ballot inside its wavefront, sixteen wavefront totals through LDS, a running base over the chunks of 1024 lines.
constexpr int kNumberThreads = 1024;
__global__ __launch_bounds__(kNumberThreads) void lines_number_kernel(int n, const uint8_t* __restrict__ created, const double* __restrict__ x0, const double* __restrict__ dir,
                                                                     int32_t first_id, uint8_t* __restrict__ ln_has, int32_t* __restrict__ ln_id, double* __restrict__ ln_x0,
                                                                     double* __restrict__ ln_dir, int32_t* __restrict__ new_id, int32_t* __restrict__ counts) {
  __shared__ int wave_new[kNumberThreads / 64], wave_held[kNumberThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int base = 0, held = 0;
  for (int i0 = 0; i0 < n; i0 += kNumberThreads) {
    const int i = i0 + tid;
    const bool in = i < n;
    const bool c = in && created[i] != 0, h = in && ln_has[i] != 0;
    const unsigned long long cm = __ballot(c), hm = __ballot(h);
    if (lane == 0) { wave_new[w] = __popcll(cm); wave_held[w] = __popcll(hm); }
    __syncthreads();
    int before = 0, total = 0, htotal = 0;
    for (int k = 0; k < kNumberThreads / 64; k++) { const int v = wave_new[k]; if (k < w) before += v; total += v; htotal += wave_held[k]; }
    if (in) {
      int32_t id = -1;
      if (c) {
        id = first_id + base + before + __popcll(cm & ((1ull << lane) - 1ull));
        ln_has[i] = 1; ln_id[i] = id;
        for (int k = 0; k < 3; k++) { ln_x0[3 * i + k] = x0[3 * i + k]; ln_dir[3 * i + k] = dir[3 * i + k]; }
      }
      new_id[i] = id;
    }
    base += total; held += htotal;
    __syncthreads();
  }
  if (tid == 0) { counts[0] = base; counts[1] = held; }
}

bool octaves_ok(const int32_t* oct, int n) {
  for (int i = 0; i < n; i++) if (oct[i] < 0 || oct[i] > 64) return false;
  return true;
}

// a frame B can read: lines, and a pose some stage or lld_frame_track_set_state left
bool has_lines_and_pose(const lld_frame* f) { return f->track && f->track->stage1_queued && f->track->nl > 0; }

LineFrameDev frame_lines_dev(const lld_frame_track_state* S) {
  return LineFrameDev{S->nl, S->ln_left, S->ln_loct, S->ln_right, S->ln_match, S->D.ln_has, S->ln_cell, S->ln_desc, S->dim};
}

}  // namespace

extern "C" {

int lld_frame_build_lines(lld_frame* f, const lld_frame_lines_build* L) {
  if (!f) return LLD_ERR_INVALID;
  if (L) {
    if (L->n_left < 0 || L->n_right < 0 || L->dim <= 0 || !(L->sx > 0) || !(L->sy > 0)) return LLD_ERR_INVALID;
    if (L->n_left > 0 && (!L->left || !L->left_octave || !L->desc_left)) return LLD_ERR_INVALID;
    if (L->n_right > 0 && (!L->right || !L->right_octave || !L->desc_right)) return LLD_ERR_INVALID;
    if (!octaves_ok(L->left_octave, L->n_left) || !octaves_ok(L->right_octave, L->n_right)) return LLD_ERR_INVALID;
    if (L->n_left > frame_max_lines(f->nt)) return LLD_ERR_UNSUPPORTED;
    if (const int st = line_limits_check(L->n_left, L->n_right, L->dim)) return st;
  }
  LLD_HIP_TRY(hipSetDevice(f->ctx->device));
  if (f->track) LLD_HIP_TRY(hipStreamSynchronize(f->ctx->stream));          // kernels of the state this call replaces may still run
  return frame_state_build_lines(f, (L && L->n_left > 0) ? L : nullptr);
}

int lld_frame_lines_download(lld_frame* f, int32_t* line_matches, double* match_dist) {
  if (!f) return LLD_ERR_INVALID;
  lld_ctx* ctx = f->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  lld_frame_track_state* S = f->track;
  if (!S || S->nl <= 0) { LLD_HIP_TRY(hipStreamSynchronize(ctx->stream)); return LLD_OK; }
  if (!line_matches) return LLD_ERR_INVALID;
  const size_t nl = (size_t)S->nl;
  const size_t bytes = (match_dist && S->ln_mdist) ? S->match_bytes : nl * 4;
  void* hb; if (const int st = lld_ctx_pinned(ctx, bytes, &hb)) return st;      // (a landing buffer: this call waits before it returns)
  LLD_HIP_TRY(hipMemcpyAsync(hb, S->ln_match, bytes, hipMemcpyDeviceToHost, ctx->stream));
  LLD_HIP_TRY(hipStreamSynchronize(ctx->stream));
  std::memcpy(line_matches, hb, nl * 4);
  if (match_dist) {
    if (S->ln_mdist) std::memcpy(match_dist, static_cast<char*>(hb) + (reinterpret_cast<const char*>(S->ln_mdist) - reinterpret_cast<const char*>(S->ln_match)), nl * 8);
    else for (size_t i = 0; i < nl; i++) match_dist[i] = 1.7976931348623157e308;
  }
  return LLD_OK;
}

int lld_frame_new_map_lines(lld_frame* cur, lld_frame* last, const lld_frame_new_lines_params* p, lld_frame_new_lines_result* out) {
  if (!cur || !last || !p || !out || cur == last || cur->ctx != last->ctx) return LLD_ERR_INVALID;
  if (!has_lines_and_pose(cur) || !has_lines_and_pose(last)) return LLD_ERR_INVALID;
  lld_frame_track_state* Sc = cur->track; lld_frame_track_state* Sl = last->track;
  if (Sc->dim != Sl->dim) return LLD_ERR_INVALID;
  const int n = Sc->nl, n_last = Sl->nl;
  if (p->first_new_id < 0 || (int64_t)p->first_new_id + (int64_t)n > (int64_t)INT32_MAX) return LLD_ERR_INVALID;
  lld_ctx* ctx = cur->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  // ---- the downloaded block, then the skip flags behind it (device scratch of the context: ordered by the stream)
  UploadBlock B;
  const auto ml = B.take<int32_t>(n), nid = B.take<int32_t>(n), cnt = B.take<int32_t>(4); const auto cr = B.take<uint8_t>(n);
  const auto x0 = B.take<double>(n, 3), dir = B.take<double>(n, 3);
  B.end_upload();                                                               // (here: the prefix that travels back)
  const auto skip = B.take<uint8_t>(n_last);
  void* hb; int st = lld_ctx_pinned(ctx, B.up_bytes, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind(static_cast<char*>(hb), static_cast<char*>(db));
  const size_t lds = (size_t)Sc->seen_lsize * 4;
  if (lds > kSkipLdsMax) return LLD_ERR_UNSUPPORTED;                            // (cannot happen: the frame's line limit keeps the table inside the budget)
  if (lds > 48 * 1024) LLD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&lines_last_skip_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSkipLdsMax));
  hipStream_t sm = ctx->stream;
  hipLaunchKernelGGL(lines_last_skip_kernel, dim3(1), dim3(kSkipThreads), lds, sm, Sc->D.tracked, Sc->D.n_tracked, Sc->D.tracked_cap, n_last, Sl->D.ln_has, Sl->D.ln_id,
                     B.dev(skip), Sc->seen_lsize - 1);
  LLD_HIP_TRY(hipGetLastError());
  const LastKfDev in{frame_lines_dev(Sc), frame_lines_dev(Sl), B.dev(skip), Sc->D.line_params, Sl->D.line_params};
  st = line_lastkf_launch_dev(sm, in, p->thr_reproj_base, p->md_thr, p->use_grid, B.dev(ml), B.dev(cr), B.dev(x0), B.dev(dir)); if (st) return st;
  hipLaunchKernelGGL(lines_number_kernel, dim3(1), dim3(kNumberThreads), 0, sm, n, B.dev(cr), B.dev(x0), B.dev(dir), p->first_new_id, Sc->D.ln_has, Sc->D.ln_id, Sc->D.ln_x0,
                     Sc->D.ln_dir, B.dev(nid), B.dev(cnt));
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(B.h, B.d, B.up_bytes, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  out->n_created = B.host(cnt)[0]; out->n_held = B.host(cnt)[1];
  if (out->match_last) std::memcpy(out->match_last, B.host(ml), (size_t)n * 4);
  if (out->new_id) std::memcpy(out->new_id, B.host(nid), (size_t)n * 4);
  if (out->created) std::memcpy(out->created, B.host(cr), (size_t)n);
  if (out->x0) std::memcpy(out->x0, B.host(x0), (size_t)n * 24);
  if (out->dir) std::memcpy(out->dir, B.host(dir), (size_t)n * 24);
  return LLD_OK;
}

}  // extern "C"
