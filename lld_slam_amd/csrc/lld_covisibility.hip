// lld_covisibility.hip — covisibility counting for a batch of keyframes (lld_covisibility, include/lld_amd.h):
// KeyFrame::UpdateConnections (src/KeyFrame.cc:312-402), the vote of Tracking::UpdateLocalKeyFrames and the redundancy count of
// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:633-697).  Hand-written HIP for gfx950.  Every result is an integer.
//   covis_query  one workgroup of 256 per query.  A group of 16 lanes walks one query entry's observation range (consecutive
//                lanes read consecutive obs_kf / obs_octave entries), so four entries are in flight per wavefront.
//                Connections: atomicAdd on int counters in LDS, one per keyframe slot (integer adds commute: the counters do not
//                depend on the order).  Culling: the qualifying observations of an entry are summed over its group by lane
//                shuffles, the two per-query sums over the wavefront, then one LDS atomic per wavefront.
//                Finishing pass: the non-zero counters are compacted in slot order (ballot + prefix over the four wavefronts),
//                which gives every connected keyframe its rank; rank rises with slot.  The maximum is reduced on the key
//                (weight, ~rank) so that the lowest slot wins, the counters >= th go out as 64-bit keys (weight << 32 | rank), come
//                back into the LDS the counters occupied, and a bitonic sort orders them; they are written in descending order.
//                Both lists go to a per-query staging range whose size the host bounds by min(n_kf, observations of the query's entries).
//   covis_pack   the library's one pack kernel, for this call and for lld_map_covisibility (lld_covis::pack_launch).  One workgroup per
//                query: the exclusive sums of the per-query counts give conn_start / ordered_start and the totals; if both totals
//                fit the capacities the staged lists are copied to their packed places, the ordered keyframes through their ranks.
// No workgroup reads what another workgroup of the same kernel writes, so a query's result cannot depend on the batch.
// From the staged lists onward the two calls share everything (lld_covis_lists.h); the host half of that is defined at the end of this file.
#include <cmath>
#include <vector>

#include "lld_common.h"
#include "lld_covis_lists.h"
#include "lld_wave.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kGroup = 16;                   // lanes per query entry
constexpr int kGroups = kThreads / kGroup;

typedef unsigned long long u64;
using lld_covis::Lists;
using lld_track::UploadBlock;

struct CovisArgs {
  const int32_t* obs_start; const int32_t* obs_kf; const int32_t* obs_octave; const uint8_t* point_bad; const int32_t* point_nobs;
  const int32_t* query_kf; const int32_t* q_start; const int32_t* q_point; const int32_t* q_octave; const float* q_depth;
  const float* q_th_depth;
  int32_t n_kf, monocular, th, th_obs; uint32_t flags; double ratio;
  Lists L;
};

__global__ __launch_bounds__(kThreads) void covis_query(CovisArgs A) {
  extern __shared__ u64 dyn[];               // int counter[n_kf] while counting, the sort keys afterwards
  int* counter = reinterpret_cast<int*>(dyn);
  __shared__ int s_wave[2][kWaves];
  __shared__ u64 s_best[kWaves];
  __shared__ int s_cull[2];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  const bool conn = (A.flags & LLD_COVIS_CONNECTIONS) != 0, cull = (A.flags & LLD_COVIS_CULLING) != 0;
  const int own = A.query_kf[q], e0 = A.q_start[q], e1 = A.q_start[q + 1];
  if (conn) for (int i = t; i < A.n_kf; i += kThreads) counter[i] = 0;
  if (t < 2) s_cull[t] = 0;
  __syncthreads();

  const int g = t / kGroup, gl = t % kGroup;
  const float th_depth = cull ? A.q_th_depth[q] : 0.f;
  int my_mps = 0, my_red = 0;                // kept by the first lane of each group
  for (int base = e0; base < e1; base += kGroups) {                          // uniform over the workgroup: the shuffles below are safe
    const int e = base + g;
    int s = 0, f = 0, lvl = 0;
    bool count_cull = false;
    if (e < e1) {
      const int p = A.q_point[e];
      if (!A.point_bad[p]) {
        bool walk = conn;
        if (cull) {
          const float depth = A.q_depth[e];
          if (lld_covis::depth_counts(A.monocular, depth, th_depth)) {
            if (gl == 0) my_mps++;
            if (A.point_nobs[p] > A.th_obs) { count_cull = true; walk = true; lvl = A.q_octave[e] + 1; }
          }
        }
        if (walk) { s = A.obs_start[p]; f = A.obs_start[p + 1]; }
      }
    }
    int c = 0;
    for (int o = s + gl; o < f; o += kGroup) {
      const int kf = A.obs_kf[o];
      if (kf == own) continue;
      if (conn) atomicAdd(&counter[kf], 1);
      if (count_cull && A.obs_octave[o] <= lvl) c++;
    }
    if (cull) {
      c = lld_wave::sum<kGroup>(c);
      if (gl == 0 && count_cull && c >= A.th_obs) my_red++;
    }
  }
  if (cull) {
    lld_wave::sum_each(my_mps, my_red);
    if (lane == 0) { atomicAdd(&s_cull[0], my_mps); atomicAdd(&s_cull[1], my_red); }
    __syncthreads();
    if (t == 0) lld_covis::publish_cull(A.L, q, s_cull[0], s_cull[1], A.ratio);
  }
  if (!conn) return;
  __syncthreads();

  // ---- the non-zero counters in slot order (their rank), the maximum with its lowest rank, the counters >= th as keys
  const Lists& L = A.L;
  const size_t off = (size_t)L.stage_off[q];
  const u64 below = lane == 0 ? 0ull : (~0ull >> (kWave - lane));
  int n_conn = 0, n_sel = 0;
  u64 best = 0;
  for (int c0 = 0; c0 < A.n_kf; c0 += kThreads) {
    const int slot = c0 + t;
    const int w = slot < A.n_kf ? counter[slot] : 0;
    const bool nz = w > 0, sel = nz && w >= A.th;
    const u64 bz = __ballot(nz), bs = __ballot(sel);
    if (lane == 0) { s_wave[0][wv] = __popcll(bz); s_wave[1][wv] = __popcll(bs); }
    __syncthreads();
    int wz = 0, ws = 0, tz = 0, ts = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const int a = s_wave[0][k], b = s_wave[1][k];
      if (k < wv) { wz += a; ws += b; }
      tz += a; ts += b;
    }
    if (nz) {
      const uint32_t rank = (uint32_t)(n_conn + wz + __popcll(bz & below));
      L.st_kf[off + rank] = slot; L.st_w[off + rank] = w;
      const u64 key = ((u64)(uint32_t)w << 32) | (0xffffffffu - rank);
      if (key > best) best = key;
      if (sel) L.st_key[off + n_sel + ws + __popcll(bs & below)] = ((u64)(uint32_t)w << 32) | rank;
    }
    n_conn += tz; n_sel += ts;
    __syncthreads();                         // (the last one also stands between the st_kf writes and lane 0's read of st_kf[off + rmax] below)
  }
  best = lld_wave::max(best);
  if (lane == 0) s_best[wv] = best;
  __syncthreads();
  best = s_best[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) if (s_best[k] > best) best = s_best[k];
  const int nmax = n_conn ? (int)(best >> 32) : 0;
  const uint32_t rmax = 0xffffffffu - (uint32_t)best;
  const int n_ord = n_sel ? n_sel : (n_conn ? 1 : 0);
  if (t == 0) {
    L.cnt_conn[q] = n_conn; L.cnt_ord[q] = n_ord; L.n_max[q] = nmax; L.kf_max[q] = n_conn ? L.st_kf[off + rmax] : -1; L.updated[q] = n_conn ? 1 : 0;
    if (n_conn && !n_sel) L.st_key[off] = ((u64)(uint32_t)nmax << 32) | rmax;              // the fallback pair (nmax, pKFmax)
  }
  if (n_sel < 2) return;
  // ---- descending (weight, rank), which is descending (weight, slot): the staged keys come back into the LDS the counters held
  int npad = 1;
  while (npad < n_sel) npad <<= 1;
  for (int i = t; i < npad; i += kThreads) dyn[i] = i < n_sel ? L.st_key[off + i] : 0ull;   // a real key is above 0: its weight is >= 1
  __syncthreads();
  lld_wave::bitonic_sort<kThreads>(dyn, npad);
  for (int i = t; i < n_sel; i += kThreads) L.st_key[off + i] = dyn[npad - 1 - i];
}

__global__ __launch_bounds__(kThreads) void covis_pack(Lists A) {
  __shared__ int s_sum[4][kWaves];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
  int v[4] = {0, 0, 0, 0};                   // conn before q, ordered before q, conn total, ordered total
  for (int j = t; j < A.n_queries; j += kThreads) {
    const int a = A.cnt_conn[j], b = A.cnt_ord[j];
    if (j < q) { v[0] += a; v[1] += b; }
    v[2] += a; v[3] += b;
  }
  lld_wave::sum_each(v[0], v[1], v[2], v[3]);
  if (lane == 0) for (int k = 0; k < 4; ++k) s_sum[k][wv] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[k] = 0; for (int w = 0; w < kWaves; ++w) v[k] += s_sum[k][w]; }
  if (t == 0) {
    A.conn_start[q] = v[0]; A.ord_start[q] = v[1];
    if (q == A.n_queries - 1) { A.conn_start[A.n_queries] = v[2]; A.ord_start[A.n_queries] = v[3]; A.totals[0] = v[2]; A.totals[1] = v[3]; }
  }
  if (v[2] > A.cap_conn || v[3] > A.cap_ord) return;                       // a short capacity: only the totals go back
  const size_t off = (size_t)A.stage_off[q];
  const int nc = A.cnt_conn[q], no = A.cnt_ord[q];
  for (int i = t; i < nc; i += kThreads) { A.conn_kf[v[0] + i] = A.st_kf[off + i]; A.conn_w[v[0] + i] = A.st_w[off + i]; }
  for (int i = t; i < no; i += kThreads) {
    const u64 key = A.st_key[off + i];
    A.ord_kf[v[1] + i] = A.st_kf[off + (uint32_t)key]; A.ord_w[v[1] + i] = (int32_t)(key >> 32);
  }
}

bool csr_ok(int32_t n, int32_t total, const int32_t* start) {
  if (start[0] != 0 || start[n] != total) return false;
  for (int i = 0; i < n; ++i) if (start[i + 1] < start[i]) return false;
  return true;
}

}  // namespace

extern "C" {

void lld_covisibility_params_default(lld_covisibility_params* p) {
  if (!p) return;
  p->th = 15; p->th_obs = 3; p->redundant_ratio = 0.9;
}

int lld_covisibility(lld_ctx* ctx, const lld_covisibility_in* in, lld_covisibility_out* out) {
  if (!ctx || !in || !out) return LLD_ERR_INVALID;
  const int32_t n_kf = in->n_kf, np = in->n_points, n_obs = in->n_obs, nq = in->n_queries, ne = in->n_entries;
  const bool conn = (in->flags & LLD_COVIS_CONNECTIONS) != 0, cull = (in->flags & LLD_COVIS_CULLING) != 0;
  if (n_kf < 0 || np < 0 || n_obs < 0 || nq < 0 || ne < 0) return LLD_ERR_INVALID;
  if ((in->flags & ~(uint32_t)(LLD_COVIS_CONNECTIONS | LLD_COVIS_CULLING)) || !(conn || cull)) return LLD_ERR_INVALID;
  if (nq == 0) return LLD_OK;
  if (!in->obs_start || !in->query_kf || !in->q_start || (n_obs > 0 && !in->obs_kf) || (np > 0 && !in->point_bad) || (ne > 0 && !in->q_point))
    return LLD_ERR_INVALID;
  if (cull && ((n_obs > 0 && !in->obs_octave) || (np > 0 && !in->point_nobs) || (ne > 0 && (!in->q_octave || !in->q_depth)) ||
               !in->q_th_depth))
    return LLD_ERR_INVALID;
  if (lld_covis::check_out(out, conn, cull)) return LLD_ERR_INVALID;
  if (!csr_ok(np, n_obs, in->obs_start) || !csr_ok(nq, ne, in->q_start)) return LLD_ERR_INVALID;
  for (int o = 0; o < n_obs; ++o) if (in->obs_kf[o] < 0 || in->obs_kf[o] >= n_kf) return LLD_ERR_INVALID;
  for (int q = 0; q < nq; ++q) if (in->query_kf[q] < -1 || in->query_kf[q] >= n_kf) return LLD_ERR_INVALID;
  for (int e = 0; e < ne; ++e) if (in->q_point[e] < 0 || in->q_point[e] >= np) return LLD_ERR_INVALID;
  if (n_kf > LLD_COVIS_MAX_KF) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  // the staging range of a query: it cannot connect to more keyframes than exist, nor to more than its entries hold observations
  std::vector<int32_t> stage_off;
  long long stage_total = 0, stage_max = 0;
  if (conn) {
    stage_off.resize((size_t)nq + 1);
    for (int q = 0; q < nq; ++q) {
      long long b = 0;
      for (int e = in->q_start[q]; e < in->q_start[q + 1] && b < n_kf; ++e) b += in->obs_start[in->q_point[e] + 1] - in->obs_start[in->q_point[e]];
      if (b > n_kf) b = n_kf;
      stage_off[q] = (int32_t)stage_total;
      stage_total += b;
      if (b > stage_max) stage_max = b;
    }
    if (stage_total > 0x7fffffffLL) return LLD_ERR_UNSUPPORTED;
    stage_off[nq] = (int32_t)stage_total;
  }

  UploadBlock B;
  const auto i_os = B.take<int32_t>((size_t)np + 1), i_ok = B.take<int32_t>(n_obs); const auto i_pb = B.take<uint8_t>(np);
  const auto i_qk = B.take<int32_t>(nq), i_qs = B.take<int32_t>((size_t)nq + 1), i_qp = B.take<int32_t>(ne);
  const auto i_oo = B.take<int32_t>(cull ? n_obs : 0), i_pn = B.take<int32_t>(cull ? np : 0), i_qo = B.take<int32_t>(cull ? ne : 0);
  const auto i_qd = B.take<float>(cull ? ne : 0), i_qt = B.take<float>(cull ? nq : 0);
  lld_covis::Plan P;
  P.outputs(B, out, conn, cull, nq, stage_total);
  P.scratch(B);
  CovisArgs A;
  const int st = P.bind(ctx, B, stage_off.data(), A.L); if (st) return st;
  B.stage(i_os, in->obs_start); B.stage(i_ok, in->obs_kf); B.stage(i_pb, in->point_bad);
  B.stage(i_qk, in->query_kf); B.stage(i_qs, in->q_start); B.stage(i_qp, in->q_point);
  B.stage(i_oo, in->obs_octave); B.stage(i_pn, in->point_nobs); B.stage(i_qo, in->q_octave); B.stage(i_qd, in->q_depth); B.stage(i_qt, in->q_th_depth);
  A.obs_start = B.dev(i_os); A.obs_kf = B.dev(i_ok); A.obs_octave = B.dev(i_oo); A.point_bad = B.dev(i_pb); A.point_nobs = B.dev(i_pn);
  A.query_kf = B.dev(i_qk); A.q_start = B.dev(i_qs); A.q_point = B.dev(i_qp); A.q_octave = B.dev(i_qo); A.q_depth = B.dev(i_qd); A.q_th_depth = B.dev(i_qt);
  A.n_kf = n_kf; A.monocular = in->monocular ? 1 : 0; A.th = in->params.th; A.th_obs = in->params.th_obs;
  A.flags = in->flags; A.ratio = in->params.redundant_ratio;

  // LDS: the counters, then the sort keys of the longest list any query can select (a power of two of 8-byte keys)
  size_t lds = 0;
  if (conn) {
    size_t npad = 1;
    while ((long long)npad < stage_max) npad <<= 1;
    lds = std::max((size_t)n_kf * 4, npad * 8);
    lds = (lds + 15) & ~size_t(15);
    if (lds > 48 * 1024)
      LLD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&covis_query), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  const int ran = lld_covis::run(ctx->stream, B, P, A.L, out->phase_ms,
                                 [&](hipStream_t sm) { hipLaunchKernelGGL(covis_query, dim3(nq), dim3(kThreads), lds, sm, A); });
  return ran ? ran : P.copy_back(B, out);
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ lld_covis_lists.h, the host half
namespace lld_covis {

int check_out(const lld_covisibility_out* out, bool conn, bool cull) {
  if (cull && (!out->n_mps || !out->n_redundant || !out->redundant)) return LLD_ERR_INVALID;
  if (conn) {
    if (out->conn_capacity < 0 || out->ordered_capacity < 0) return LLD_ERR_INVALID;
    if (!out->conn_start || !out->ordered_start || !out->n_max || !out->kf_max || !out->updated) return LLD_ERR_INVALID;
    if (out->conn_capacity > 0 && (!out->conn_kf || !out->conn_weight)) return LLD_ERR_INVALID;
    if (out->ordered_capacity > 0 && (!out->ordered_kf || !out->ordered_weight)) return LLD_ERR_INVALID;
  }
  return LLD_OK;
}

void pack_launch(hipStream_t st, const Lists& L) { hipLaunchKernelGGL(covis_pack, dim3(L.n_queries), dim3(kThreads), 0, st, L); }

void Plan::outputs(UploadBlock& B, const lld_covisibility_out* out, bool conn_, bool cull_, int32_t nq_, long long stage_total_) {
  conn = conn_; cull = cull_; nq = nq_; stage_total = (size_t)stage_total_;
  cap_conn = conn ? (int32_t)std::min<long long>(out->conn_capacity, stage_total_) : 0;
  cap_ord = conn ? (int32_t)std::min<long long>(out->ordered_capacity, stage_total_) : 0;
  const size_t nc = conn ? nq : 0, nu = cull ? nq : 0;
  stage_off = B.take<int32_t>(conn ? nc + 1 : 0);
  B.end_upload();
  out_off = B.size;
  conn_start = B.take<int32_t>(conn ? nc + 1 : 0); ord_start = B.take<int32_t>(conn ? nc + 1 : 0); totals = B.take<int32_t>(conn ? 2 : 0);
  n_max = B.take<int32_t>(nc); kf_max = B.take<int32_t>(nc); updated = B.take<uint8_t>(nc);
  n_mps = B.take<int32_t>(nu); n_red = B.take<int32_t>(nu); redundant = B.take<uint8_t>(nu);
  conn_kf = B.take<int32_t>(cap_conn); conn_w = B.take<int32_t>(cap_conn); ord_kf = B.take<int32_t>(cap_ord); ord_w = B.take<int32_t>(cap_ord);
}

void Plan::scratch(UploadBlock& B) {
  out_bytes = B.size - out_off;
  cnt_conn = B.take<int32_t>(conn ? nq : 0); cnt_ord = B.take<int32_t>(conn ? nq : 0);
  st_kf = B.take<int32_t>(stage_total); st_w = B.take<int32_t>(stage_total); st_key = B.take<u64>(stage_total);
}

int Plan::bind(lld_ctx* ctx, UploadBlock& B, const int32_t* stage_off_host, Lists& L) const {
  int st;
  void* hb; st = lld_ctx_pinned(ctx, out_off + out_bytes, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind((char*)hb, (char*)db);
  if (conn) B.stage(stage_off, stage_off_host);
  L.stage_off = B.dev(stage_off); L.n_queries = nq;
  L.st_kf = B.dev(st_kf); L.st_w = B.dev(st_w); L.st_key = B.dev(st_key);
  L.cnt_conn = B.dev(cnt_conn); L.cnt_ord = B.dev(cnt_ord); L.n_max = B.dev(n_max); L.kf_max = B.dev(kf_max); L.updated = B.dev(updated);
  L.n_mps = B.dev(n_mps); L.n_red = B.dev(n_red); L.redundant = B.dev(redundant);
  L.cap_conn = cap_conn; L.cap_ord = cap_ord;
  L.conn_start = B.dev(conn_start); L.ord_start = B.dev(ord_start); L.totals = B.dev(totals);
  L.conn_kf = B.dev(conn_kf); L.conn_w = B.dev(conn_w); L.ord_kf = B.dev(ord_kf); L.ord_w = B.dev(ord_w);
  return LLD_OK;
}

int Plan::copy_back(const UploadBlock& B, lld_covisibility_out* out) const {
  if (conn) {
    const int32_t* tot = B.host(totals);
    out->n_conn = tot[0]; out->n_ordered = tot[1];
    if (tot[0] > out->conn_capacity || tot[1] > out->ordered_capacity) return LLD_ERR_INVALID;
    std::memcpy(out->conn_start, B.host(conn_start), (size_t)(nq + 1) * 4); std::memcpy(out->ordered_start, B.host(ord_start), (size_t)(nq + 1) * 4);
    std::memcpy(out->n_max, B.host(n_max), (size_t)nq * 4); std::memcpy(out->kf_max, B.host(kf_max), (size_t)nq * 4); std::memcpy(out->updated, B.host(updated), (size_t)nq);
    if (tot[0]) { std::memcpy(out->conn_kf, B.host(conn_kf), (size_t)tot[0] * 4); std::memcpy(out->conn_weight, B.host(conn_w), (size_t)tot[0] * 4); }
    if (tot[1]) { std::memcpy(out->ordered_kf, B.host(ord_kf), (size_t)tot[1] * 4); std::memcpy(out->ordered_weight, B.host(ord_w), (size_t)tot[1] * 4); }
  }
  if (cull) {
    std::memcpy(out->n_mps, B.host(n_mps), (size_t)nq * 4); std::memcpy(out->n_redundant, B.host(n_red), (size_t)nq * 4); std::memcpy(out->redundant, B.host(redundant), (size_t)nq);
  }
  return LLD_OK;
}

}  // namespace lld_covis
