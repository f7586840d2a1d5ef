// lld_map_covis.hip — covisibility on the resident map's tables (lld_map.hip, lld_map_tables.h): lld_map_covisibility, which is
// KeyFrame::UpdateConnections, src/KeyFrame.cc:312-402, and the redundancy count of LocalMapping::KeyFrameCulling,
// src/LocalMapping.cc:646-694.  map_covis_query_kernel, one workgroup per query, finds and counts a query's observations here; from the
// staged lists onward the call is lld_covisibility's (lld_covis_lists.h: the pack kernel, the layout, the timed run, the copy-back).
// The culling part reads four members more (MapExt: keypoint index per observation, nObs per point, octave / depth / mThDepth per keyframe);
// their tables and pools are allocated by the first lld_map_set_observations_indexed / lld_map_set_keyframe_keypoints, never by lld_map_create.
#include "lld_common.h"
#include "lld_covis_lists.h"
#include "lld_map_tables.h"
#include "lld_wave.h"

namespace {

using lld_covis::Lists;
using lld_map_dev::MapDev;
using lld_map_dev::MapExt;
using lld_map_dev::u64;
using lld_track::UploadBlock;

// ------------------------------------------------------------------------------------------------ covisibility on the tables
// map_covis_query_kernel, one workgroup of 256 per query.  A group of 16 lanes walks the observation row of one entry of the query
// keyframe's point row, so sixteen entries are in flight.
//   Connections: a map has up to 2^18 keyframe slots and a query meets a few hundred of them, so the counts live in an open-addressing table
//     in LDS keyed by slot (8192 cells: int key[], int count[], 64 KB; home cell = slot mod 8192, linear probing).  A lane claims an empty
//     cell by atomicCAS and then adds to the cell's count; integer adds commute, so the counts do not depend on the order.  Claims are counted:
//     beyond LLD_MAP_COVIS_MAX_CONNECTED the query is an overflow and nothing more is inserted (at most one claim per lane goes through
//     behind the limit, so the table is never full and every probe ends).
//   Finishing: the cells in use are compacted to the query's staging range in HBM (the table is dead from here), their order_key fetched,
//     and (key, position) sorted in the LDS the table held (lld_wave::bitonic_sort_pairs): the rank in that order is map order, conn_* go
//     out by rank, the maximum is reduced on (weight, ~rank) so that the lowest rank wins, and the counts >= th are sorted once more as
//     weight << 32 | rank; read from the top that is descending weight, then descending order_key.
//   Culling: the qualifying observations of an entry are summed over its group by lane shuffles, the two per-query sums over the wavefront,
//     then one LDS atomic per wavefront.  Two dependent loads more per observation than on flat tables: the keypoint index, then the octave
//     in the observing keyframe's row - each behind a comparison of the index with that row's length.
// No workgroup reads what another workgroup of the same kernel writes, so a query's result cannot depend on the batch.
constexpr int kCovThreads = 256, kCovGroup = 16, kCovGroups = kCovThreads / kCovGroup;
constexpr int kCovMax = LLD_MAP_COVIS_MAX_CONNECTED, kCovCells = 2 * kCovMax;
static_assert((kCovCells & (kCovCells - 1)) == 0 && kCovMax + 2 * kCovThreads < kCovCells, "the table keeps empty cells behind an overflow");
constexpr size_t kCovLds = (size_t)kCovCells * 8;
enum { CS_CLAIMED = 0, CS_NO_KP, CS_MPS, CS_RED, CS_WORDS };

struct CovArgs {
  const int32_t* query;
  int32_t monocular, th, th_obs, has_ext; uint32_t flags; double ratio;
  int32_t* st_slot; int32_t* st_cnt;         // staging: the table's cells in use, in cell order; L.st_kf / L.st_w hold the same in map order
  uint8_t* status;
  Lists L;
};

__device__ __forceinline__ void cov_count(int* tkey, int* tcnt, int* s_st, int kf) {
  if (*(volatile int*)&s_st[CS_CLAIMED] > kCovMax) return;
  int h = kf & (kCovCells - 1);
  for (;;) {
    int k = *(volatile int*)&tkey[h];
    if (k == -1) {
      k = atomicCAS(&tkey[h], -1, kf);
      if (k == -1) { atomicAdd(&s_st[CS_CLAIMED], 1); k = kf; }
    }
    if (k == kf) break;
    h = (h + 1) & (kCovCells - 1);
  }
  atomicAdd(&tcnt[h], 1);
}

__global__ __launch_bounds__(kCovThreads) void map_covis_query_kernel(MapDev M, MapExt X, CovArgs A) {
  extern __shared__ __align__(16) unsigned char cov_lds[];
  int* tkey = reinterpret_cast<int*>(cov_lds);
  int* tcnt = tkey + kCovCells;
  u64* keys = reinterpret_cast<u64*>(cov_lds);                         // behind the compaction: 32 KB of sort keys, 16 KB of values
  int* vals = reinterpret_cast<int*>(keys + kCovMax);
  __shared__ int s_st[CS_WORDS];
  __shared__ int s_scan[kCovThreads / 64];
  __shared__ u64 s_best[kCovThreads / 64];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const bool conn = (A.flags & LLD_COVIS_CONNECTIONS) != 0, cull = (A.flags & LLD_COVIS_CULLING) != 0;
  const Lists& L = A.L;
  const int own = A.query[q];
  const int2 rp = M.k_pt[own];
  if (conn) for (int i = t; i < kCovCells; i += kCovThreads) { tkey[i] = -1; tcnt[i] = 0; }
  if (t < CS_WORDS) s_st[t] = 0;
  // culling reads the keyframe's keypoint row beside its point row: only a row of the same length is read at all
  int2 ro = make_int2(0, 0), rd = make_int2(0, 0);
  float th_depth = 0.f;
  bool kp_ok = false;
  if (cull && A.has_ext) { ro = X.k_oct[own]; rd = X.k_dep[own]; th_depth = X.k_thd[own]; kp_ok = ro.y == rp.y && rd.y == rp.y; }
  const bool cull_run = cull && kp_ok;
  __syncthreads();

  const int g = t / kCovGroup, gl = t % kCovGroup;
  int my_mps = 0, my_red = 0;                                          // kept by the first lane of each group
  const int n_row = (conn || cull_run) ? rp.y : 0;
  for (int base = 0; base < n_row; base += kCovGroups) {               // uniform over the workgroup: the shuffles below are safe
    const int j = base + g;
    int s = 0, f = 0, lvl = 0, to_idx = 0;
    bool count_cull = false;
    if (j < n_row) {
      const int p = M.kpt_pool[rp.x + j];
      const int state = p >= 0 ? M.p_state[p] : 2;                     // NULL entries and bad points are skipped by both routines
      if (state != 2) {
        bool walk = conn && state == 1;                                // a point never set has an empty row
        if (cull_run) {
          const float depth = __int_as_float(X.dep_pool[rd.x + j]);
          if (lld_covis::depth_counts(A.monocular, depth, th_depth)) {
            if (gl == 0) my_mps++;
            if (state == 1) {                                          // never set: Observations() == 0
              // a row without an index row of its length came through lld_map_set_observations: its n_obs is not known either
              const int2 row = M.p_obs[p], ir = X.p_idx[p];
              if (ir.y != row.y) s_st[CS_NO_KP] = 1;
              else if (X.p_nobs[p] > A.th_obs) { count_cull = true; lvl = X.oct_pool[ro.x + j] + 1; to_idx = ir.x - row.x; }
            }
          }
        }
        if (walk || count_cull) { const int2 row = M.p_obs[p]; s = row.x; f = row.x + row.y; }
      }
    }
    int c = 0;
    for (int o = s + gl; o < f; o += kCovGroup) {
      const int kf = M.obs_pool[o];
      if (kf == own) continue;
      if (conn) cov_count(tkey, tcnt, s_st, kf);
      if (count_cull) {
        const int idx = X.idx_pool[o + to_idx];
        const int2 orow = X.k_oct[kf];
        if (idx < 0 || idx >= orow.y) s_st[CS_NO_KP] = 1;              // an index outside the observer's keypoint row
        else if (X.oct_pool[orow.x + idx] <= lvl) c++;
      }
    }
    if (cull_run) {
      c = lld_wave::sum<kCovGroup>(c);
      if (gl == 0 && count_cull && c >= A.th_obs) my_red++;
    }
  }
  if (cull_run) {
    lld_wave::sum_each(my_mps, my_red);
    if (lane == 0) { atomicAdd(&s_st[CS_MPS], my_mps); atomicAdd(&s_st[CS_RED], my_red); }
  }
  __syncthreads();
  int status = 0;
  if (cull) {
    const bool no_kp = !kp_ok || s_st[CS_NO_KP] != 0;
    if (no_kp) status |= LLD_MAP_COVIS_NO_KEYPOINT_DATA;
    if (t == 0) lld_covis::publish_cull(L, q, no_kp ? 0 : s_st[CS_MPS], no_kp ? 0 : s_st[CS_RED], A.ratio);
  }
  if (!conn) { if (t == 0) A.status[q] = (uint8_t)status; return; }
  const int claimed = s_st[CS_CLAIMED];
  if (claimed == 0 || claimed > kCovMax) {
    // keyframeCounter.empty() (:346-347), or more keyframes than the table answers for: no entries, the cov row stays
    if (t == 0) {
      L.cnt_conn[q] = 0; L.cnt_ord[q] = 0; L.n_max[q] = 0; L.kf_max[q] = -1; L.updated[q] = 0;
      A.status[q] = (uint8_t)(status | (claimed ? LLD_MAP_COVIS_CONN_OVERFLOW : 0));
    }
    return;
  }
  // ---- the cells in use, to the staging
  const size_t off = (size_t)L.stage_off[q];
  int n = 0;
  for (int c0 = 0; c0 < kCovCells && n < claimed; c0 += kCovThreads) {
    const int k = tkey[c0 + t], w = tcnt[c0 + t];
    int tot;
    const int r = lld_wave::block_excl_scan<kCovThreads>(k >= 0 ? 1 : 0, s_scan, tot);
    if (k >= 0) { A.st_slot[off + n + r] = k; A.st_cnt[off + n + r] = w; }
    n += tot;
  }
  __syncthreads();                                                     // the table is dead; the staged cells are visible to the workgroup
  // ---- map order: ascending order_key
  int npad = 2;
  while (npad < n) npad <<= 1;
  for (int i = t; i < npad; i += kCovThreads) { keys[i] = i < n ? M.k_key[A.st_slot[off + i]] : ~0ull; vals[i] = i < n ? i : -1; }
  __syncthreads();
  lld_wave::bitonic_sort_pairs<kCovThreads>(keys, vals, npad);
  u64 best = 0;
  int n_sel = 0;
  for (int r = t; r < npad; r += kCovThreads) {
    u64 k2 = 0;                                                        // a selected key is above 0: its weight is >= 1
    if (r < n) {
      const int i = vals[r], slot = A.st_slot[off + i], w = A.st_cnt[off + i];
      L.st_kf[off + r] = slot; L.st_w[off + r] = w;
      const u64 b = ((u64)(uint32_t)w << 32) | (uint32_t)(0xffffffffu - (uint32_t)r);     // it->second > nmax: the first of the greatest
      if (b > best) best = b;
      if (w >= A.th) { k2 = ((u64)(uint32_t)w << 32) | (uint32_t)r; n_sel++; }
    }
    keys[r] = k2;                                                      // rank r's key was this lane's to read
  }
  best = lld_wave::max(best);
  if (lane == 0) s_best[wv] = best;
  n_sel = lld_wave::block_sum(n_sel, s_scan);                          // (its barriers also publish s_best and the keys)
  best = s_best[0];
#pragma unroll
  for (int k = 1; k < kCovThreads / 64; ++k) if (s_best[k] > best) best = s_best[k];
  const int nmax = (int)(best >> 32), rmax = (int)(0xffffffffu - (uint32_t)best);
  const int n_ord = n_sel ? n_sel : 1;                                 // none reaches th: the single pair (nmax, pKFmax) (:371-375)
  lld_wave::bitonic_sort<kCovThreads>(keys, npad);                     // descending (weight, order_key) from the top
  for (int i = t; i < n_sel; i += kCovThreads) L.st_key[off + i] = keys[npad - 1 - i];
  if (t == 0) {
    if (!n_sel) L.st_key[off] = ((u64)(uint32_t)nmax << 32) | (uint32_t)rmax;
    L.cnt_conn[q] = n; L.cnt_ord[q] = n_ord; L.n_max[q] = nmax; L.kf_max[q] = L.st_kf[off + rmax]; L.updated[q] = 1;
    A.status[q] = (uint8_t)status;
  }
  if ((A.flags & LLD_MAP_COVIS_WRITE_COV) && status == 0) {
    // mvpOrderedConnectedKeyFrames' first ten: what Tracking::UpdateLocalMap reads as GetBestCovisibilityKeyFrames(10)
    const int nc = min(n_ord, 10);
    if (t < nc) M.k_cov[10 * own + t] = L.st_kf[off + (n_sel ? (uint32_t)keys[npad - 1 - t] : (uint32_t)rmax)];
    if (t == 0) M.k_ncov[own] = nc;
  }
}

}  // namespace

extern "C" {

int lld_map_covisibility(lld_map* m, const lld_map_covisibility_in* in, lld_map_covisibility_out* out) {
  if (!m || !in || !out) return LLD_ERR_INVALID;
  const int32_t nq = in->n_queries;
  const bool conn = (in->flags & LLD_COVIS_CONNECTIONS) != 0, cull = (in->flags & LLD_COVIS_CULLING) != 0;
  if (nq < 0) return LLD_ERR_INVALID;
  if ((in->flags & ~(uint32_t)(LLD_COVIS_CONNECTIONS | LLD_COVIS_CULLING | LLD_MAP_COVIS_WRITE_COV)) || !(conn || cull)) return LLD_ERR_INVALID;
  if ((in->flags & LLD_MAP_COVIS_WRITE_COV) && !conn) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (nq == 0) return LLD_OK;
  if (!in->kf_slot || !out->status) return LLD_ERR_INVALID;
  if (lld_covis::check_out(&out->lists, conn, cull)) return LLD_ERR_INVALID;
  for (int q = 0; q < nq; q++) if (in->kf_slot[q] < 0 || in->kf_slot[q] >= m->lim.max_keyframes || !m->kf_set[in->kf_slot[q]]) return LLD_ERR_INVALID;
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  // the staging range of a query: it cannot meet more keyframes than its points hold observations, nor more than the table answers for
  // (the host's rows are the device's: every update before this call is queued before its kernels)
  std::vector<int32_t> stage_off;
  long long stage_total = 0;
  if (conn) {
    stage_off.resize((size_t)nq + 1);
    for (int q = 0; q < nq; q++) {
      const int s = in->kf_slot[q];
      const int32_t* row = m->kpt.mirror.data() + m->kpt.off[s];
      long long b = 0;
      for (int j = 0; j < m->kpt.len[s] && b < kCovMax; j++) if (row[j] >= 0) b += m->obs.len[row[j]];
      stage_off[q] = (int32_t)stage_total;
      stage_total += std::min<long long>(b, kCovMax);
    }
    if (stage_total > 0x7fffffffLL) return LLD_ERR_UNSUPPORTED;
    stage_off[nq] = (int32_t)stage_total;
  }

  UploadBlock B;
  const auto i_q = B.take<int32_t>(nq);
  lld_covis::Plan P;
  P.outputs(B, &out->lists, conn, cull, nq, stage_total);
  const auto r_st = B.take<uint8_t>(nq);
  P.scratch(B);
  const auto t_sl = B.take<int32_t>((size_t)stage_total), t_sc = B.take<int32_t>((size_t)stage_total);
  CovArgs A;
  int st = P.bind(ctx, B, stage_off.data(), A.L); if (st) return st;
  B.stage(i_q, in->kf_slot);
  A.query = B.dev(i_q);
  A.monocular = in->monocular ? 1 : 0; A.th = in->params.th; A.th_obs = in->params.th_obs; A.has_ext = m->d_ext ? 1 : 0;
  A.flags = in->flags; A.ratio = in->params.redundant_ratio;
  A.st_slot = B.dev(t_sl); A.st_cnt = B.dev(t_sc); A.status = B.dev(r_st);

  if (in->flags & LLD_MAP_COVIS_WRITE_COV) m->mutations++;             // cov rows change: a staged BA window is no longer this map's
  if (conn && !m->cov_lds_set) {
    LLD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&map_covis_query_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCovLds));
    m->cov_lds_set = true;
  }
  st = lld_covis::run(ctx->stream, B, P, A.L, out->lists.phase_ms, [&](hipStream_t sm) {
    hipLaunchKernelGGL(map_covis_query_kernel, dim3(nq), dim3(kCovThreads), conn ? kCovLds : 0, sm, m->D, m->X, A);
  });
  if (!st) st = P.copy_back(B, &out->lists);
  if (st) return st;
  std::memcpy(out->status, B.host(r_st), (size_t)nq);
  return LLD_OK;
}

}  // extern "C"
