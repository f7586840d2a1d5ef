// lld_covisibility.hip — covisibility counting for a batch of keyframes (lld_covisibility, include/lld_amd.h):
// KeyFrame::UpdateConnections (src/KeyFrame.cc:312-402), the vote of Tracking::UpdateLocalKeyFrames and the redundancy count of
// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:633-697).  Hand-written HIP for gfx950.  Every result is an integer.
//   covis_query  one workgroup of 256 per query.  A group of 16 lanes walks one query entry's observation range (consecutive
//                lanes read consecutive obs_kf / obs_octave entries), so four entries are in flight per wavefront.
//                Connections: atomicAdd on int counters in LDS, one per keyframe slot (integer adds commute: the counters do not
//                depend on the order).  Culling: the qualifying observations of an entry are summed over its group by lane
//                shuffles, the two per-query sums over the wavefront, then one LDS atomic per wavefront.
//                Finishing pass: the non-zero counters are compacted in slot order (ballot + prefix over the four wavefronts),
//                the maximum is reduced on the key (weight, ~slot) so that the lowest slot wins, the counters >= th go out as
//                64-bit keys (weight << 32 | slot), come back into the LDS the counters occupied, and a bitonic sort orders
//                them; they are written in descending order.  Both lists go to a per-query staging range whose size the host
//                bounds by min(n_kf, observations of the query's entries).
//   covis_pack   one workgroup per query: the exclusive sums of the per-query counts give conn_start / ordered_start and the
//                totals; if both totals fit the capacities the staged lists are copied to their packed places.
// No workgroup reads what another workgroup of the same kernel writes, so a query's result cannot depend on the batch.
#include <cmath>
#include <vector>

#include "lld_common.h"
#include "lld_wave.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kGroup = 16;                   // lanes per query entry
constexpr int kGroups = kThreads / kGroup;

typedef unsigned long long u64;

struct CovisArgs {
  const int32_t* obs_start; const int32_t* obs_kf; const int32_t* obs_octave; const uint8_t* point_bad; const int32_t* point_nobs;
  const int32_t* query_kf; const int32_t* q_start; const int32_t* q_point; const int32_t* q_octave; const float* q_depth;
  const float* q_th_depth;
  const int32_t* stage_off;                  // [n_queries+1] the staging range of each query
  int32_t n_kf, n_queries, monocular, th, th_obs; uint32_t flags; double ratio;
  int32_t* st_kf; int32_t* st_w; u64* st_key;                               // staging
  int32_t* cnt_conn; int32_t* cnt_ord; int32_t* n_max; int32_t* kf_max; uint8_t* updated;
  int32_t* n_mps; int32_t* n_red; uint8_t* redundant;
  int32_t cap_conn, cap_ord;
  int32_t* conn_start; int32_t* ord_start; int32_t* totals;                 // packed outputs
  int32_t* conn_kf; int32_t* conn_w; int32_t* ord_kf; int32_t* ord_w;
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
          if (A.monocular || !(depth > th_depth || depth < 0.f)) {
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
    if (t == 0) {
      const int nm = s_cull[0], nr = s_cull[1];
      A.n_mps[q] = nm; A.n_red[q] = nr;
      A.redundant[q] = ((double)nr > A.ratio * (double)nm) ? 1 : 0;          // nRedundantObservations > 0.9*nMPs: int against double
    }
  }
  if (!conn) return;
  __syncthreads();

  // ---- the non-zero counters in slot order, the maximum with its lowest slot, the counters >= th as keys
  const size_t off = (size_t)A.stage_off[q];
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
      const size_t i = off + n_conn + wz + __popcll(bz & below);
      A.st_kf[i] = slot; A.st_w[i] = w;
      const u64 key = ((u64)(uint32_t)w << 32) | (uint32_t)(0xffffffffu - (uint32_t)slot);
      if (key > best) best = key;
    }
    if (sel) A.st_key[off + n_sel + ws + __popcll(bs & below)] = ((u64)(uint32_t)w << 32) | (uint32_t)slot;
    n_conn += tz; n_sel += ts;
    __syncthreads();
  }
  best = lld_wave::max(best);
  if (lane == 0) s_best[wv] = best;
  __syncthreads();
  best = s_best[0];
#pragma unroll
  for (int k = 1; k < kWaves; ++k) if (s_best[k] > best) best = s_best[k];
  const int nmax = n_conn ? (int)(best >> 32) : 0;
  const int kfmax = n_conn ? (int)(0xffffffffu - (uint32_t)best) : -1;
  const int n_ord = n_sel ? n_sel : (n_conn ? 1 : 0);
  if (t == 0) {
    A.cnt_conn[q] = n_conn; A.cnt_ord[q] = n_ord; A.n_max[q] = nmax; A.kf_max[q] = kfmax; A.updated[q] = n_conn ? 1 : 0;
    if (n_conn && !n_sel) A.st_key[off] = ((u64)(uint32_t)nmax << 32) | (uint32_t)kfmax;   // the fallback pair (nmax, pKFmax)
  }
  if (n_sel < 2) return;
  // ---- descending (weight, slot): the staged keys come back into the LDS the counters held
  int npad = 1;
  while (npad < n_sel) npad <<= 1;
  for (int i = t; i < npad; i += kThreads) dyn[i] = i < n_sel ? A.st_key[off + i] : 0ull;   // a real key is above 0: its weight is >= 1
  __syncthreads();
  lld_wave::bitonic_sort<kThreads>(dyn, npad);
  for (int i = t; i < n_sel; i += kThreads) A.st_key[off + i] = dyn[npad - 1 - i];
}

__global__ __launch_bounds__(kThreads) void covis_pack(CovisArgs A) {
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
    A.ord_kf[v[1] + i] = (int32_t)(uint32_t)key; A.ord_w[v[1] + i] = (int32_t)(key >> 32);
  }
}

inline size_t al(size_t b) { return (b + 255) & ~size_t(255); }

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
               !in->q_th_depth || !out->n_mps || !out->n_redundant || !out->redundant))
    return LLD_ERR_INVALID;
  if (conn) {
    if (out->conn_capacity < 0 || out->ordered_capacity < 0) return LLD_ERR_INVALID;
    if (!out->conn_start || !out->ordered_start || !out->n_max || !out->kf_max || !out->updated) return LLD_ERR_INVALID;
    if (out->conn_capacity > 0 && (!out->conn_kf || !out->conn_weight)) return LLD_ERR_INVALID;
    if (out->ordered_capacity > 0 && (!out->ordered_kf || !out->ordered_weight)) return LLD_ERR_INVALID;
  }
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
  const int32_t cap_conn = conn ? (int32_t)std::min<long long>(out->conn_capacity, stage_total) : 0;
  const int32_t cap_ord = conn ? (int32_t)std::min<long long>(out->ordered_capacity, stage_total) : 0;

  size_t inb = 0, outb = 0, tmpb = 0;
  auto add_in = [&](size_t b) { const size_t o = inb; inb += al(b); return o; };
  auto add_out = [&](size_t b) { const size_t o = outb; outb += al(b); return o; };
  auto add_tmp = [&](size_t b) { const size_t o = tmpb; tmpb += al(b); return o; };
  const size_t o_os = add_in((size_t)(np + 1) * 4), o_ok = add_in((size_t)n_obs * 4), o_pb = add_in((size_t)np);
  const size_t o_qk = add_in((size_t)nq * 4), o_qs = add_in((size_t)(nq + 1) * 4), o_qp = add_in((size_t)ne * 4);
  const size_t o_oo = cull ? add_in((size_t)n_obs * 4) : 0, o_pn = cull ? add_in((size_t)np * 4) : 0;
  const size_t o_qo = cull ? add_in((size_t)ne * 4) : 0, o_qd = cull ? add_in((size_t)ne * 4) : 0, o_qt = cull ? add_in((size_t)nq * 4) : 0;
  const size_t o_so = conn ? add_in((size_t)(nq + 1) * 4) : 0;
  const size_t r_cs = conn ? add_out((size_t)(nq + 1) * 4) : 0, r_rs = conn ? add_out((size_t)(nq + 1) * 4) : 0;
  const size_t r_tot = conn ? add_out(8) : 0, r_nm = conn ? add_out((size_t)nq * 4) : 0, r_km = conn ? add_out((size_t)nq * 4) : 0;
  const size_t r_up = conn ? add_out((size_t)nq) : 0;
  const size_t r_ck = conn ? add_out((size_t)cap_conn * 4) : 0, r_cw = conn ? add_out((size_t)cap_conn * 4) : 0;
  const size_t r_rk = conn ? add_out((size_t)cap_ord * 4) : 0, r_rw = conn ? add_out((size_t)cap_ord * 4) : 0;
  const size_t r_mp = cull ? add_out((size_t)nq * 4) : 0, r_rd = cull ? add_out((size_t)nq * 4) : 0, r_rf = cull ? add_out((size_t)nq) : 0;
  const size_t t_cc = conn ? add_tmp((size_t)nq * 4) : 0, t_co = conn ? add_tmp((size_t)nq * 4) : 0;
  const size_t t_kf = conn ? add_tmp((size_t)stage_total * 4) : 0, t_w = conn ? add_tmp((size_t)stage_total * 4) : 0;
  const size_t t_key = conn ? add_tmp((size_t)stage_total * 8) : 0;
  int st;
  void* hb; st = lld_ctx_pinned(ctx, inb + outb, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, inb + outb + tmpb + 256, &db); if (st) return st;
  char* h = (char*)hb; char* d = (char*)db; char* h_out = h + inb; char* d_out = d + inb; char* d_tmp = d_out + outb;
  std::memcpy(h + o_os, in->obs_start, (size_t)(np + 1) * 4);
  if (n_obs) std::memcpy(h + o_ok, in->obs_kf, (size_t)n_obs * 4);
  if (np) std::memcpy(h + o_pb, in->point_bad, (size_t)np);
  std::memcpy(h + o_qk, in->query_kf, (size_t)nq * 4);
  std::memcpy(h + o_qs, in->q_start, (size_t)(nq + 1) * 4);
  if (ne) std::memcpy(h + o_qp, in->q_point, (size_t)ne * 4);
  if (cull) {
    if (n_obs) std::memcpy(h + o_oo, in->obs_octave, (size_t)n_obs * 4);
    if (np) std::memcpy(h + o_pn, in->point_nobs, (size_t)np * 4);
    if (ne) { std::memcpy(h + o_qo, in->q_octave, (size_t)ne * 4); std::memcpy(h + o_qd, in->q_depth, (size_t)ne * 4); }
    std::memcpy(h + o_qt, in->q_th_depth, (size_t)nq * 4);
  }
  if (conn) std::memcpy(h + o_so, stage_off.data(), (size_t)(nq + 1) * 4);

  CovisArgs A;
  auto I32 = [](char* p) { return reinterpret_cast<int32_t*>(p); };
  A.obs_start = I32(d + o_os); A.obs_kf = I32(d + o_ok); A.obs_octave = I32(d + o_oo); A.point_bad = reinterpret_cast<uint8_t*>(d + o_pb);
  A.point_nobs = I32(d + o_pn); A.query_kf = I32(d + o_qk); A.q_start = I32(d + o_qs); A.q_point = I32(d + o_qp);
  A.q_octave = I32(d + o_qo); A.q_depth = reinterpret_cast<float*>(d + o_qd); A.q_th_depth = reinterpret_cast<float*>(d + o_qt);
  A.stage_off = I32(d + o_so);
  A.n_kf = n_kf; A.n_queries = nq; A.monocular = in->monocular ? 1 : 0; A.th = in->params.th; A.th_obs = in->params.th_obs;
  A.flags = in->flags; A.ratio = in->params.redundant_ratio;
  A.st_kf = I32(d_tmp + t_kf); A.st_w = I32(d_tmp + t_w); A.st_key = reinterpret_cast<u64*>(d_tmp + t_key);
  A.cnt_conn = I32(d_tmp + t_cc); A.cnt_ord = I32(d_tmp + t_co);
  A.n_max = I32(d_out + r_nm); A.kf_max = I32(d_out + r_km); A.updated = reinterpret_cast<uint8_t*>(d_out + r_up);
  A.n_mps = I32(d_out + r_mp); A.n_red = I32(d_out + r_rd); A.redundant = reinterpret_cast<uint8_t*>(d_out + r_rf);
  A.cap_conn = cap_conn; A.cap_ord = cap_ord;
  A.conn_start = I32(d_out + r_cs); A.ord_start = I32(d_out + r_rs); A.totals = I32(d_out + r_tot);
  A.conn_kf = I32(d_out + r_ck); A.conn_w = I32(d_out + r_cw); A.ord_kf = I32(d_out + r_rk); A.ord_w = I32(d_out + r_rw);

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
  hipStream_t sm = ctx->stream;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  const bool timed = out->phase_ms != nullptr;
  if (timed) for (int k = 0; k < 4; ++k) LLD_HIP_TRY(hipEventCreate(&ev[k]));
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[0], sm));
  LLD_HIP_TRY(hipMemcpyAsync(d, h, inb, hipMemcpyHostToDevice, sm));
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[1], sm));
  hipLaunchKernelGGL(covis_query, dim3(nq), dim3(kThreads), lds, sm, A);
  if (conn) hipLaunchKernelGGL(covis_pack, dim3(nq), dim3(kThreads), 0, sm, A);
  LLD_HIP_TRY(hipGetLastError());
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[2], sm));
  LLD_HIP_TRY(hipMemcpyAsync(h_out, d_out, outb, hipMemcpyDeviceToHost, sm));
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[3], sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  if (timed) {
    for (int k = 0; k < 3; ++k) LLD_HIP_TRY(hipEventElapsedTime(&out->phase_ms[k], ev[k], ev[k + 1]));
    for (int k = 0; k < 4; ++k) LLD_HIP_TRY(hipEventDestroy(ev[k]));
  }

  if (conn) {
    const int32_t* tot = reinterpret_cast<const int32_t*>(h_out + r_tot);
    out->n_conn = tot[0]; out->n_ordered = tot[1];
    if (tot[0] > out->conn_capacity || tot[1] > out->ordered_capacity) return LLD_ERR_INVALID;
    std::memcpy(out->conn_start, h_out + r_cs, (size_t)(nq + 1) * 4);
    std::memcpy(out->ordered_start, h_out + r_rs, (size_t)(nq + 1) * 4);
    std::memcpy(out->n_max, h_out + r_nm, (size_t)nq * 4);
    std::memcpy(out->kf_max, h_out + r_km, (size_t)nq * 4);
    std::memcpy(out->updated, h_out + r_up, (size_t)nq);
    if (tot[0]) { std::memcpy(out->conn_kf, h_out + r_ck, (size_t)tot[0] * 4); std::memcpy(out->conn_weight, h_out + r_cw, (size_t)tot[0] * 4); }
    if (tot[1]) { std::memcpy(out->ordered_kf, h_out + r_rk, (size_t)tot[1] * 4); std::memcpy(out->ordered_weight, h_out + r_rw, (size_t)tot[1] * 4); }
  }
  if (cull) {
    std::memcpy(out->n_mps, h_out + r_mp, (size_t)nq * 4);
    std::memcpy(out->n_redundant, h_out + r_rd, (size_t)nq * 4);
    std::memcpy(out->redundant, h_out + r_rf, (size_t)nq);
  }
  return LLD_OK;
}

}  // extern "C"
