// lld_map_fuse.hip — ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:825-958) on the resident map's tables, the call
// LocalMapping::SearchInNeighbors (src/LocalMapping.cc:455-535) makes 10-30 times per keyframe.  The rules are stated in include/lld_amd.h.
//
// Search, on the device: everything it reads is a table of the map - the target keyframe's k_uvr / k_oct / k_desc rows, the candidates'
// fixed rows and observation rows, the target's point row.
//   fu_search_kernel   one wavefront per candidate, four per workgroup, ceil(n / 4) workgroups.  The wavefront decides the skip (slot -1,
//                      never set, bad, the target in the observation row - the lanes stride over the row, one ballot), projects with the
//                      float operations of project_fuse_kernel (lld_project_math.h, contraction off; the scalar work is the same in every
//                      lane), then its lanes stride over the target's keypoints: window, PosInGrid cell inside the grid and inside
//                      GetFeaturesInArea's cell range, level gate, chi2 gate, Hamming distance on eight words.  One 64-bit key per lane,
//                      distance << 48 | cell << 24 | index with cell = column * rows + row, and one wavefront minimum: the first minimum
//                      in GetFeaturesInArea's order.  With the match it writes the candidate's Observations() and state for the walk.
//   fu_holders_kernel  one lane per entry of the target's point row: Observations() and state of the point it holds
// No atomics, no scratch, no LDS but the two level tables.  Every stored index is held to the row it points into before it is followed.
//
// Walk, on the host: serial by nature and tiny.  It runs on copies of the rows the map mirrors (RowPool) and of the downloaded counts and
// flags - the closed set it can touch is the candidates and the entries of the target's point row - until every limit has been checked.
// Then RowPool::plan / reserve / commit / launch place the changed rows (no second allocator), fu_fixed_kernel scatters the changed counts
// and flags, lld_map_refresh.hip's descriptor kernels run for the survivors behind them on the stream, and fu_lengths_kernel reads the
// changed rows' lengths back: a disagreement with the host poisons the map, as in lld_map_ba_apply.
#pragma clang fp contract(off)

#include <algorithm>
#include <chrono>
#include <unordered_map>
#include <vector>

#include "lld_common.h"
#include "lld_map_tables.h"
#include "lld_project_math.h"
#include "lld_round_trip.h"
#include "lld_wave.h"

namespace {

using lld_map_dev::MapBa;
using lld_map_dev::MapDesc;
using lld_map_dev::MapDev;
using lld_map_dev::MapExt;
using lld_map_dev::PoolPlan;
using lld_map_dev::RowPool;
using lld_rt::blocks;
using lld_rt::copy_out;
using lld_rt::round_trip;
using lld_track::Span;
using lld_track::UploadBlock;
typedef unsigned long long u64;

constexpr int kWave = 64, kWaves = 4, kThreads = kWave * kWaves;
constexpr int kThLow = 50;                         // TH_LOW, src/ORBmatcher.cc:38
constexpr int kIndexBits = 24, kCellBits = 24;     // of the packed key; the distance (at most 256) sits above them
constexpr u64 kNone = ~0ull;

struct FuArgs {
  lld_frame_view V;
  float scale[LLD_ORB_MAX_LEVELS], inv_sigma2[LLD_ORB_MAX_LEVELS];
  float th, min_x, min_y, winv, hinv;
  int32_t cols, rows, n_levels;
  int32_t n, target, source, n_row;
  int32_t obs_cap, kpt_cap, uvr_cap, oct_cap, kdesc_cap;   // entries of obs_pool / kpt_pool / uvr_pool / oct_pool / kdesc_pool
  const int32_t* slot;                             // null: the candidates are the source keyframe's point row
  int32_t* match; int32_t* c_nobs; uint8_t* c_state;
  int32_t* h_nobs; uint8_t* h_state;
};

// The projection (src/ORBmatcher.cc:852-890, the operations of project_fuse_kernel) and the search among the target's keypoints (:892-932)
// for point slot s.  The whole wavefront calls it with the same s; returns bestIdx or -1 in every lane.
__device__ __forceinline__ int fu_search_one(const MapDev& M, const MapExt& X, const MapBa& Y, const MapDesc& Z, const FuArgs& A, const float* lv, int s, int lane) {
  using namespace lld_proj;
  const float P[3] = {M.p_pos[3 * (size_t)s], M.p_pos[3 * (size_t)s + 1], M.p_pos[3 * (size_t)s + 2]};
  float Pc[3]; cv_transform(A.V, P, Pc);
  if (Pc[2] < 0.0f) return -1;
  const float invz = __fdiv_rn(1.0f, Pc[2]);
  const float x = __fmul_rn(Pc[0], invz), y = __fmul_rn(Pc[1], invz);
  const float u = __fadd_rn(__fmul_rn(A.V.fx, x), A.V.cx), v = __fadd_rn(__fmul_rn(A.V.fy, y), A.V.cy);
  if (!(u >= A.V.min_x && u < A.V.max_x && v >= A.V.min_y && v < A.V.max_y)) return -1;        // KeyFrame::IsInImage
  const float ur = __fsub_rn(u, __fmul_rn(A.V.bf, invz));
  const float maxd = M.p_maxd[s];
  const float maxDistance = __fmul_rn(1.2f, maxd), minDistance = __fmul_rn(0.8f, M.p_mind[s]);
  const float PO[3] = {__fsub_rn(P[0], A.V.Ow[0]), __fsub_rn(P[1], A.V.Ow[1]), __fsub_rn(P[2], A.V.Ow[2])};
  const float dist3D = cv_norm3(PO);
  if (dist3D < minDistance || dist3D > maxDistance) return -1;
  const float Pn[3] = {M.p_nrm[3 * (size_t)s], M.p_nrm[3 * (size_t)s + 1], M.p_nrm[3 * (size_t)s + 2]};
  if (cv_dot3(PO, Pn) < __dmul_rn(0.5, (double)dist3D)) return -1;                               // PO.dot(Pn)<0.5*dist3D
  const int lvl = predict_scale(maxd, dist3D, A.V);
  const float r = __fmul_rn(A.th, lv[lvl]);
  // GetFeaturesInArea's cell range (src/KeyFrame.cc:592-610): float arithmetic, floor / ceil, clamps and early returns
  const int minCX = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(u, A.min_x), r), A.winv)));
  const int maxCX = min(A.cols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(u, A.min_x), r), A.winv)));
  const int minCY = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(v, A.min_y), r), A.hinv)));
  const int maxCY = min(A.rows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(v, A.min_y), r), A.hinv)));
  if (!(minCX < A.cols && maxCX >= 0 && minCY < A.rows && maxCY >= 0)) return -1;
  // the target's rows; the host holds their lengths to the point row's, the device to each other
  const int2 kp = M.k_pt[A.target], ku = Y.k_uvr[A.target], ko = X.k_oct[A.target], kd = Z.k_desc[A.target];
  int nt = min(min(kp.y, ku.y / 3), min(ko.y, kd.y / 8));
  if (ku.x < 0 || ko.x < 0 || kd.x < 0 || (long long)ku.x + 3LL * nt > A.uvr_cap || (long long)ko.x + nt > A.oct_cap || (long long)kd.x + 8LL * nt > A.kdesc_cap) nt = 0;   // ... and to their pools
  uint32_t qd[8];
#pragma unroll
  for (int w = 0; w < 8; w++) qd[w] = M.p_desc[8 * (size_t)s + w];
  u64 best = kNone;
  for (int k = lane; k < nt; k += kWave) {
    const int32_t* f = Y.uvr_pool + ku.x + 3 * (size_t)k;
    const float kx = __int_as_float(f[0]), ky = __int_as_float(f[1]), kur = __int_as_float(f[2]);
    if (!(fabsf(__fsub_rn(kx, u)) < r && fabsf(__fsub_rn(ky, v)) < r)) continue;                 // KeyFrame.cc:620-624
    const int px = (int)roundf(__fmul_rn(__fsub_rn(kx, A.min_x), A.winv)), py = (int)roundf(__fmul_rn(__fsub_rn(ky, A.min_y), A.hinv));   // PosInGrid
    if (px < 0 || px >= A.cols || py < 0 || py >= A.rows) continue;                              // never assigned to the grid
    if (px < minCX || px > maxCX || py < minCY || py > maxCY) continue;
    const int oct = X.oct_pool[ko.x + k];
    if (oct < 0 || oct < lvl - 1 || oct > lvl) continue;                                         // :907-908
    const float ex = __fsub_rn(u, kx), ey = __fsub_rn(v, ky);                                    // :912-931
    float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    if (kur >= 0.f) {
      const float er = __fsub_rn(ur, kur);
      e2 = __fadd_rn(e2, __fmul_rn(er, er));
      if ((double)__fmul_rn(e2, lv[LLD_ORB_MAX_LEVELS + oct]) > 7.8) continue;
    } else {
      if ((double)__fmul_rn(e2, lv[LLD_ORB_MAX_LEVELS + oct]) > 5.99) continue;
    }
    const int d = lld_wave::hamming256(qd, reinterpret_cast<const uint4*>(Z.kdesc_pool + kd.x + 8 * (size_t)k));   // rows start at multiples of eight words
    const u64 key = ((u64)(unsigned)d << (kIndexBits + kCellBits)) | ((u64)(unsigned)(px * A.rows + py) << kIndexBits) | (u64)(unsigned)k;
    best = key < best ? key : best;
  }
  best = lld_wave::min(best);
  if (best == kNone || (int)(best >> (kIndexBits + kCellBits)) > kThLow) return -1;              // if(bestDist<=TH_LOW)
  return (int)(best & ((1ull << kIndexBits) - 1));
}

__global__ __launch_bounds__(kThreads) void fu_search_kernel(MapDev M, MapExt X, MapBa Y, MapDesc Z, FuArgs A) {
  __shared__ float lv[2 * LLD_ORB_MAX_LEVELS];     // level_scale, then 1 / sigma2
  if (threadIdx.x < LLD_ORB_MAX_LEVELS) { lv[threadIdx.x] = A.scale[threadIdx.x]; lv[LLD_ORB_MAX_LEVELS + threadIdx.x] = A.inv_sigma2[threadIdx.x]; }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1), q = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (q >= A.n) return;                            // (uniform over the wavefront, as everything below up to the keypoint loop)
  int s = -1;
  if (A.slot) s = A.slot[q];
  else {
    const int2 sr = M.k_pt[A.source];
    if (q < sr.y && sr.x >= 0 && (long long)sr.x + q < A.kpt_cap) s = M.kpt_pool[sr.x + q];
  }
  if (s < 0 || s >= M.max_pt) s = -1;              // NULL
  int state = 0, nobs = 0, best = -1;
  if (s >= 0) { state = M.p_state[s]; nobs = X.p_nobs[s]; }
  if (state == 1) {                                // neither never set nor bad
    const int2 row = M.p_obs[s];
    if (row.x >= 0 && row.y >= 0 && (long long)row.x + row.y <= A.obs_cap) {
      bool in_kf = false;                          // pMP->IsInKeyFrame(pKF)
      for (int j = lane; j < row.y; j += kWave) in_kf = in_kf || M.obs_pool[row.x + j] == A.target;
      if (!__ballot(in_kf)) best = fu_search_one(M, X, Y, Z, A, lv, s, lane);
    }
  }
  if (lane == 0) { A.match[q] = best; A.c_nobs[q] = nobs; A.c_state[q] = (uint8_t)state; }
}

__global__ void fu_holders_kernel(MapDev M, MapExt X, FuArgs A) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.n_row) return;
  const int2 kp = M.k_pt[A.target];
  int s = -1;
  if (j < kp.y && kp.x >= 0 && (long long)kp.x + j < A.kpt_cap) s = M.kpt_pool[kp.x + j];
  const bool ok = s >= 0 && s < M.max_pt;
  A.h_nobs[j] = ok ? X.p_nobs[s] : 0; A.h_state[j] = ok ? M.p_state[s] : 0;
}

// the counts and flags the walk changed (the host names a slot once, in range)
__global__ void fu_fixed_kernel(int n, const int32_t* slot, const int32_t* nobs, const uint8_t* state, int32_t* p_nobs, uint8_t* p_state) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { p_nobs[slot[i]] = nobs[i]; p_state[slot[i]] = state[i]; }
}
__global__ void fu_lengths_kernel(int n, const int32_t* slot, const int2* p_obs, const int2* p_idx, int32_t* len_obs, int32_t* len_idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { len_obs[i] = p_obs[slot[i]].y; len_idx[i] = p_idx[slot[i]].y; }
}
__global__ void fu_counts_kernel(int n, const int32_t* slot, const int32_t* p_nobs, int32_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = p_nobs ? p_nobs[slot[i]] : 0;
}

// ------------------------------------------------------------------------------------------------ the walk (src/ORBmatcher.cc:934-956)
// Copies of the rows it changes, keyed by slot, over the map's mirrors; the counts and flags of the closed set it can touch.
struct Walk {
  lld_map* m;
  std::unordered_map<int, std::vector<int32_t>> obs, idx, kpt;
  std::unordered_map<int, int32_t> nobs; std::unordered_map<int, uint8_t> state;
  std::vector<int> pt_order, kf_order, fixed_order, survivors;       // first-touch order: what the upload lists
  std::unordered_map<int, uint8_t> fixed_seen;
  bool broken = false;                              // an index row of another length than its observation row, or a slot outside the closed set

  struct View { const int32_t* p; int n; };
  static View view_of(const std::unordered_map<int, std::vector<int32_t>>& over, const RowPool& R, int s) {
    const auto it = over.find(s);
    if (it != over.end()) return {it->second.data(), (int)it->second.size()};
    return {R.mirror.data() + R.off[s], R.len[s]};
  }
  static std::vector<int32_t>& edit(std::unordered_map<int, std::vector<int32_t>>& over, const RowPool& R, int s, std::vector<int>* order) {
    auto it = over.find(s);
    if (it == over.end()) {
      it = over.emplace(s, std::vector<int32_t>(R.mirror.begin() + R.off[s], R.mirror.begin() + R.off[s] + R.len[s])).first;
      if (order) order->push_back(s);
    }
    return it->second;
  }
  View obs_of(int s) const { return view_of(obs, m->obs, s); }
  View kpt_of(int kf) const { return view_of(kpt, m->kpt, kf); }
  bool in_keyframe(int s, int kf) const { const View r = obs_of(s); return std::find(r.p, r.p + r.n, kf) != r.p + r.n; }
  int32_t nobs_of(int s) { const auto it = nobs.find(s); if (it == nobs.end()) { broken = true; return 0; } return it->second; }
  uint8_t state_of(int s) { const auto it = state.find(s); if (it == state.end()) { broken = true; return 0; } return it->second; }
  void touch_fixed(int s) { if (!fixed_seen[s]) { fixed_seen[s] = 1; fixed_order.push_back(s); } }
  bool stereo(int kf, int i) const {                // mvuRight[idx] >= 0
    if (!m->d_ba || 3 * (long long)i + 2 >= m->kuvr.len[kf]) return false;
    float ur; std::memcpy(&ur, &m->kuvr.mirror[m->kuvr.off[kf] + 3 * (size_t)i + 2], 4);
    return ur >= 0.f;
  }
  void set_match(int kf, int i, int32_t v) { if (i < kpt_of(kf).n) edit(kpt, m->kpt, kf, &kf_order)[i] = v; }
  // MapPoint::AddObservation (src/MapPoint.cc:67-78); the new entry goes where std::map<KeyFrame*, size_t> would hold it
  void add_observation(int s, int kf, int i) {
    if (in_keyframe(s, kf)) return;
    std::vector<int32_t>& o = edit(obs, m->obs, s, &pt_order); std::vector<int32_t>& x = edit(idx, m->idx, s, nullptr);
    if (o.size() != x.size()) { broken = true; return; }
    size_t at = 0;
    while (at < o.size() && m->kf_key[o[at]] <= m->kf_key[kf]) at++;
    o.insert(o.begin() + at, kf); x.insert(x.begin() + at, i);
    nobs[s] = nobs_of(s) + (stereo(kf, i) ? 2 : 1); touch_fixed(s);
  }
  // loser->Replace(survivor) (src/MapPoint.cc:176-220)
  void replace(int loser, int surv) {
    if (loser == surv) return;
    std::vector<int32_t>& lo = edit(obs, m->obs, loser, &pt_order); std::vector<int32_t>& lx = edit(idx, m->idx, loser, nullptr);
    if (lo.size() != lx.size()) { broken = true; return; }
    const std::vector<int32_t> kfs = lo, ids = lx;
    lo.clear(); lx.clear();
    state[loser] = 2; touch_fixed(loser);
    for (size_t j = 0; j < kfs.size(); j++) {
      if (!in_keyframe(surv, kfs[j])) { set_match(kfs[j], ids[j], surv); add_observation(surv, kfs[j], ids[j]); }
      else set_match(kfs[j], ids[j], -1);
    }
    if (std::find(survivors.begin(), survivors.end(), surv) == survivors.end()) survivors.push_back(surv);
  }
};

struct Rows { std::vector<int32_t> slot, start, data; };
Rows rows_of(const std::vector<int>& order, const std::unordered_map<int, std::vector<int32_t>>& over) {
  Rows R; R.start.push_back(0);
  for (int s : order) { const std::vector<int32_t>& r = over.at(s); R.slot.push_back(s); R.data.insert(R.data.end(), r.begin(), r.end()); R.start.push_back((int32_t)R.data.size()); }
  return R;
}

}  // namespace

extern "C" {

int lld_map_fuse(lld_map* m, const lld_map_fuse_in* in, lld_map_fuse_out* out) {
  if (!m || !in || !out) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  const int n = in->n_points, tg = in->target, src = in->source_keyframe;
  if (n < 0 || tg < 0 || tg >= m->lim.max_keyframes || !m->kf_set[tg]) return LLD_ERR_INVALID;
  if (!m->d_ext || !m->d_ba || !m->d_desc || !m->kf_feat[tg]) return LLD_ERR_INVALID;
  const int nt = m->kpt.len[tg];
  if (m->kuvr.len[tg] != 3 * (long long)nt || m->koct.len[tg] != nt || m->kdesc.len[tg] != 8 * (long long)nt) return LLD_ERR_INVALID;
  if ((in->point_slot != nullptr) == (src >= 0) || src < -1 || src >= m->lim.max_keyframes) return LLD_ERR_INVALID;
  if (src >= 0 && (!m->kf_set[src] || n != m->kpt.len[src])) return LLD_ERR_INVALID;
  if (!(in->th > 0.f) || !(in->view.fx > 0.f) || !(in->view.fy > 0.f)) return LLD_ERR_INVALID;
  if (in->n_levels < 1 || in->n_levels > LLD_ORB_MAX_LEVELS || in->view.n_levels != in->n_levels || !in->level_scale || !in->level_inv_sigma2) return LLD_ERR_INVALID;
  if (in->grid_cols < 1 || in->grid_rows < 1 || out->survivor_capacity < 0 || (out->survivor_capacity > 0 && !out->survivor)) return LLD_ERR_INVALID;
  if (n > 0 && (!out->match || !out->action || !out->other)) return LLD_ERR_INVALID;
  if (nt > (1 << kIndexBits) || (long long)in->grid_cols * in->grid_rows > (1 << kCellBits)) return LLD_ERR_UNSUPPORTED;
  std::vector<int32_t> cand(n);
  if (n) std::memcpy(cand.data(), src >= 0 ? m->kpt.mirror.data() + m->kpt.off[src] : in->point_slot, (size_t)n * 4);     // (a copy: the walk may change the source's row)
  for (int i = 0; i < n; i++) if (cand[i] < -1 || cand[i] >= m->lim.max_points) return LLD_ERR_INVALID;
  out->n_fused = out->n_added = out->n_replaced = out->n_survivors = 0;
  if (n == 0) return LLD_OK;
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  // ---------------------------------------------------------------- the search
  const size_t nn = (size_t)n;
  UploadBlock B;
  const auto u_slot = B.take<int32_t>(src >= 0 ? 0 : nn);
  B.end_upload();
  const auto r_match = B.take<int32_t>(nn), r_cn = B.take<int32_t>(nn); const auto r_cs = B.take<uint8_t>(nn);
  const auto r_hn = B.take<int32_t>(nt); const auto r_hs = B.take<uint8_t>(nt);
  B.end_download();
  int st = m->fu.grow(ctx->stream, B.travel_bytes(), B.size); if (st) return st;
  B.bind(m->fu.h, m->fu.d);
  if (src < 0) B.stage(u_slot, in->point_slot);
  FuArgs A{};
  A.V = in->view;
  for (int l = 0; l < in->n_levels; l++) { A.scale[l] = in->level_scale[l]; A.inv_sigma2[l] = in->level_inv_sigma2[l]; }
  A.th = in->th; A.min_x = in->grid_min_x; A.min_y = in->grid_min_y; A.winv = in->grid_width_inv; A.hinv = in->grid_height_inv;
  A.cols = in->grid_cols; A.rows = in->grid_rows; A.n_levels = in->n_levels;
  A.n = n; A.target = tg; A.source = src; A.n_row = nt;
  A.obs_cap = (int32_t)m->obs.mirror.size(); A.kpt_cap = (int32_t)m->kpt.mirror.size();
  A.uvr_cap = (int32_t)m->kuvr.mirror.size(); A.oct_cap = (int32_t)m->koct.mirror.size(); A.kdesc_cap = (int32_t)m->kdesc.mirror.size();
  A.slot = src >= 0 ? nullptr : B.dev(u_slot);
  A.match = B.dev(r_match); A.c_nobs = B.dev(r_cn); A.c_state = B.dev(r_cs); A.h_nobs = B.dev(r_hn); A.h_state = B.dev(r_hs);
  float t3[3] = {0.f, 0.f, 0.f};
  st = round_trip(ctx->stream, B, out->phase_ms ? t3 : nullptr, [&](hipStream_t sm) {
    hipLaunchKernelGGL(fu_search_kernel, blocks(nn, kWaves), dim3(kThreads), 0, sm, m->D, m->X, m->Y, m->Z, A);
    if (nt) hipLaunchKernelGGL(fu_holders_kernel, blocks(nt, 256), dim3(256), 0, sm, m->D, m->X, A);
    return LLD_OK;
  });
  if (st) return st;                               // nothing has changed yet
  const auto t_walk = std::chrono::steady_clock::now();

  // ---------------------------------------------------------------- the walk, on copies
  const int32_t* match = B.host(r_match);
  Walk W; W.m = m;
  for (int i = 0; i < n; i++) if (cand[i] >= 0) { W.nobs[cand[i]] = B.host(r_cn)[i]; W.state[cand[i]] = B.host(r_cs)[i]; }
  {
    const int32_t* row = m->kpt.mirror.data() + m->kpt.off[tg];
    for (int j = 0; j < nt; j++) if (row[j] >= 0 && row[j] < m->lim.max_points) { W.nobs[row[j]] = B.host(r_hn)[j]; W.state[row[j]] = B.host(r_hs)[j]; }
  }
  std::vector<uint8_t> action(nn, LLD_MAP_FUSE_NONE); std::vector<int32_t> other(nn, -1);
  int n_fused = 0, n_added = 0, n_replaced = 0;
  for (int i = 0; i < n; i++) {
    const int b = match[i];
    if (b < 0) continue;
    const int s = cand[i];
    if (s < 0 || b >= nt) return LLD_ERR_HIP;      // the search never matches a NULL entry or past the row: the device's tables are not the host's
    if (W.state_of(s) != 1 || W.in_keyframe(s, tg)) { action[i] = LLD_MAP_FUSE_SKIPPED; continue; }
    const int h = W.kpt_of(tg).p[b];
    if (h < 0) { W.add_observation(s, tg, b); W.set_match(tg, b, s); action[i] = LLD_MAP_FUSE_ADDED; n_added++; }
    else if (W.state_of(h) != 1) { action[i] = LLD_MAP_FUSE_HOLDER_BAD; other[i] = h; }
    else {
      other[i] = h; n_replaced++;
      if (W.nobs_of(h) > W.nobs_of(s)) { action[i] = LLD_MAP_FUSE_CANDIDATE_REPLACED; W.replace(s, h); }
      else { action[i] = LLD_MAP_FUSE_HOLDER_REPLACED; W.replace(h, s); }
    }
    n_fused++;
  }
  if (W.broken) return LLD_ERR_INVALID;            // (the walk went on on its copies; nothing has been queued)
  const int ns = (int)W.survivors.size();
  if (ns > out->survivor_capacity) { out->n_survivors = ns; return LLD_ERR_INVALID; }
  for (int s : W.survivors) if (W.obs_of(s).n > LLD_LANDMARK_MAX_OBS) return LLD_ERR_UNSUPPORTED;
  const Rows Ro = rows_of(W.pt_order, W.obs), Ri = rows_of(W.pt_order, W.idx), Rk = rows_of(W.kf_order, W.kpt);
  const int npc = (int)W.pt_order.size(), nkc = (int)W.kf_order.size(), nf = (int)W.fixed_order.size();
  PoolPlan Po, Pi, Pk;
  if (!m->obs.plan(npc, Ro.slot.data(), Ro.start.data(), Po) || !m->idx.plan(npc, Ri.slot.data(), Ri.start.data(), Pi) ||
      !m->kpt.plan(nkc, Rk.slot.data(), Rk.start.data(), Pk)) return LLD_ERR_UNSUPPORTED;

  // ---------------------------------------------------------------- the changed rows, counts and flags; the survivors' descriptors
  std::vector<int32_t> match_keep(match, match + n);                   // (the staging is about to be packed again)
  if (npc || nkc || nf) {
    UploadBlock C;
    m->obs.reserve(C, Po); m->idx.reserve(C, Pi); m->kpt.reserve(C, Pk);
    const auto u_fs = C.take<int32_t>(nf), u_fn = C.take<int32_t>(nf); const auto u_fst = C.take<uint8_t>(nf);
    const auto u_ss = C.take<int32_t>(ns), u_sl = C.take<int32_t>(ns), u_cs = C.take<int32_t>(npc);
    C.end_upload();
    const auto r_lo = C.take<int32_t>(npc), r_li = C.take<int32_t>(npc);
    C.end_download();
    const auto t_v = C.take<uint8_t>(ns), t_upd = C.take<uint8_t>(ns); const auto t_ref = C.take<int32_t>(ns), t_lv = C.take<int32_t>(ns), t_best = C.take<int32_t>(ns), t_med = C.take<int32_t>(ns);
    st = m->fu.grow(ctx->stream, C.travel_bytes(), C.size); if (st) return st;
    C.bind(m->fu.h, m->fu.d);
    // from here on the tables move: a HIP failure leaves host rows and device rows apart
    m->mutations++; m->win.valid = false;
    m->obs.commit(C, Po, npc, Ro.slot.data(), Ro.start.data(), Ro.data.data());
    m->idx.commit(C, Pi, npc, Ri.slot.data(), Ri.start.data(), Ri.data.data());
    m->kpt.commit(C, Pk, nkc, Rk.slot.data(), Rk.start.data(), Rk.data.data());
    for (int i = 0; i < nf; i++) { const int s = W.fixed_order[i]; C.host(u_fs)[i] = s; C.host(u_fn)[i] = W.nobs.at(s); C.host(u_fst)[i] = W.state.at(s); }
    int n_wave = 0;                                // the two launch lists of the descriptor kernels, by the new row's length
    for (int i = 0; i < ns; i++) { C.host(u_ss)[i] = W.survivors[i]; if (m->obs.len[W.survivors[i]] <= kWave) C.host(u_sl)[n_wave++] = i; }
    for (int i = 0, k = n_wave; i < ns; i++) if (m->obs.len[W.survivors[i]] > kWave) C.host(u_sl)[k++] = i;
    for (int i = 0; i < npc; i++) C.host(u_cs)[i] = W.pt_order[i];
    const lld_map_dev::DescRefresh R{ns, n_wave, C.dev(u_ss), C.dev(u_sl), C.dev(t_v), C.dev(t_ref), C.dev(t_lv), C.dev(t_best), C.dev(t_med), C.dev(t_upd)};
    st = round_trip(ctx->stream, C, nullptr, [&](hipStream_t sm) {
      int rc = m->obs.launch(sm, C, Po);
      if (!rc) rc = m->idx.launch(sm, C, Pi);
      if (!rc) rc = m->kpt.launch(sm, C, Pk);
      if (rc) return rc;
      if (nf) hipLaunchKernelGGL(fu_fixed_kernel, blocks(nf, 256), dim3(256), 0, sm, nf, C.dev(u_fs), C.dev(u_fn), C.dev(u_fst), m->X.p_nobs, m->D.p_state);
      rc = lld_map_dev::refresh_descriptors_queue(sm, m, R);
      if (rc) return rc;
      if (npc) hipLaunchKernelGGL(fu_lengths_kernel, blocks(npc, 256), dim3(256), 0, sm, npc, C.dev(u_cs), m->D.p_obs, m->X.p_idx, C.dev(r_lo), C.dev(r_li));
      return LLD_OK;
    });
    if (st) { m->poisoned = true; return st; }
    for (int i = 0; i < npc; i++) {
      const int s = W.pt_order[i];
      if (C.host(r_lo)[i] != m->obs.len[s] || C.host(r_li)[i] != m->idx.len[s]) { m->poisoned = true; return LLD_ERR_HIP; }    // never with a sound map
    }
  }
  out->n_fused = n_fused; out->n_added = n_added; out->n_replaced = n_replaced; out->n_survivors = ns;
  std::memcpy(out->match, match_keep.data(), nn * 4); std::memcpy(out->action, action.data(), nn); std::memcpy(out->other, other.data(), nn * 4);
  if (ns) std::memcpy(out->survivor, W.survivors.data(), (size_t)ns * 4);
  if (out->phase_ms) {
    out->phase_ms[0] = t3[0]; out->phase_ms[1] = t3[1]; out->phase_ms[3] = t3[2];
    out->phase_ms[2] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_walk).count();
  }
  return LLD_OK;
}

int lld_map_download_point_counts(lld_map* m, int32_t n, const int32_t* slot, int32_t* n_obs) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !n_obs) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (slot[i] < 0 || slot[i] >= m->lim.max_points) return LLD_ERR_INVALID;
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const size_t nn = (size_t)n;
  UploadBlock B;
  const auto u_slot = B.take<int32_t>(nn);
  B.end_upload();
  const auto r_n = B.take<int32_t>(nn);
  B.end_download();
  int st;
  void* hb; st = lld_ctx_pinned(ctx, B.size, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind((char*)hb, (char*)db);
  B.stage(u_slot, slot);
  st = round_trip(ctx->stream, B, nullptr, [&](hipStream_t sm) {
    hipLaunchKernelGGL(fu_counts_kernel, blocks(nn, 256), dim3(256), 0, sm, n, B.dev(u_slot), m->d_ext ? m->X.p_nobs : (const int32_t*)nullptr, B.dev(r_n));
    return LLD_OK;
  });
  if (st) return st;
  copy_out(n_obs, B, r_n, nn);
  return LLD_OK;
}

}  // extern "C"
