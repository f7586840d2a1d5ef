// lld_map.hip — the map as flat tables resident in HBM (lld_map_*), and Tracking::UpdateLocalMap (src/Tracking.cc:1667-1835) run on them
// between the two stages of the frame chain (lld_frame_track_update_local_map).
//
// The reference walks objects: mCurrentFrame.mvpMapPoints[i]->GetObservations() for the vote (:1730-1746), a std::map<KeyFrame*,int> in pointer
// order for the local keyframes (:1758-1774), GetBestCovisibilityKeyFrames(10) / GetChilds() / GetParent() for their extension (:1778-1828),
// GetMapPointMatches() / GetMapLineMatches() of every local keyframe for the local points and lines (:1684-1722).  Here every object is a slot
// (a caller-chosen dense index) and every member a row of a table:
//
//   point slot s     p_pos, p_nrm, p_mind, p_maxd, p_desc, p_state (0 never set, 1 live, 2 isBad), p_obs = (offset, length) of mObservations in obs_pool
//   line slot s      l_x0, l_dir, l_x1, l_x2, l_desc, l_bad (1: isBad or never set)
//   keyframe slot s  k_key (the position in std::map / std::set iteration), k_bad (1: isBad or never set), k_parent, k_cov[10] / k_ncov,
//                    k_child / k_pt / k_ln = (offset, length) into child_pool / kpt_pool / kln_pool
//
// The variable-length rows live in pools of twice the limit given at creation (RowPool).  The host keeps each row's offset, length and capacity
// and a copy of the pool: a replacement that fits the row's capacity is written in place, a longer one goes to the pool's tail, and when the
// tail is exhausted the pool is repacked from the host copy (the live entries fit by construction) and sent whole.  So no replacement fails
// while the live total stays inside the limit.  Every lld_map_set_* call validates everything first, then packs ONE pinned block, queues ONE
// copy and the kernels that scatter it into the tables, all on the context's stream.
//
// Kernels of UpdateLocalMap: map_vote_kernel (one lane per keypoint), map_local_keyframes_kernel (one workgroup: sort, maximum, prefetch,
// one wavefront for the order-dependent extension loop out of LDS), map_first_kernel / map_count_kernel / map_write_kernel (first occurrences
// by 64-bit atomicMin, per-keyframe counts, ordered compaction), and map_gather_kernel for stage 2 (lld_frame_track_local_map_resident).
//
// The tables' declarations are in lld_map_tables.h, and so is Staging, the grow-only pinned and device pair the setters (up_begin) and the
// other call families on the handle stage through; covisibility on the same tables (lld_map_covisibility) is in lld_map_covis.hip.
#include "lld_common.h"
#include "lld_device_math.h"
#include "lld_frame_track_state.h"
#include "lld_map_internal.h"
#include "lld_map_tables.h"
#include "lld_track_internal.h"
#include "lld_wave.h"

namespace {

using lld_map_dev::MapDev;
using lld_map_dev::MapBa;
using lld_map_dev::MapExt;
using lld_map_dev::PoolPlan;
using lld_map_dev::RowPool;
using lld_map_dev::u64;
using lld_track::Span;
using lld_track::TrackDev;
using lld_track::UploadBlock;

constexpr int kMaxVoted = 1024;                    // voted keyframes one workgroup sorts in LDS
constexpr int kLkfCap = LLD_MAP_MAX_LOCAL_KEYFRAMES;
static_assert(kLkfCap >= kMaxVoted + 3 * 81, "list capacity");    // the list: the voted ones, and at most three more per entry visited while it holds <= 80
constexpr int kMaxKeyframes = 1 << 18;             // the marks are a bit set in LDS: 32 KB at this size
enum { ST_STATUS = 0, ST_VOTED, ST_NKF, ST_NPTS, ST_NLNS, ST_CLEARED, ST_REF, ST_EMPTY, ST_STAGE2, ST_WORDS = 16 };
enum { FC_TOUCHED = 0, FC_CLEARED, FC_WORDS = 4 };

// ------------------------------------------------------------------------------------------------ scatter kernels of lld_map_set_*
__global__ void map_scatter_kernel(int n, const int32_t* slot, const int32_t* v, int32_t* dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[slot[i]] = v[i];
}
__global__ void map_drop_rows_kernel(int n, const int32_t* slot, int2* d_row) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d_row[slot[i]] = make_int2(0, 0);
}
__global__ void map_rows_kernel(int n, const int32_t* slot, const int2* row, const int32_t* src, const int32_t* data, int2* d_row, int32_t* pool) {
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    const int2 w = row[r]; const int32_t from = src[r];
    for (int j = threadIdx.x; j < w.y; j += blockDim.x) pool[w.x + j] = data[from + j];
    if (threadIdx.x == 0) d_row[slot[r]] = w;
  }
}
__global__ void map_set_points_kernel(MapDev M, int n, const int32_t* slot, const float* pos, const float* nrm, const float* mind, const float* maxd, const uint32_t* desc,
                                      const uint8_t* bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  for (int c = 0; c < 3; c++) { M.p_pos[3 * s + c] = pos[3 * i + c]; M.p_nrm[3 * s + c] = nrm[3 * i + c]; }
  M.p_mind[s] = mind[i]; M.p_maxd[s] = maxd[i];
  for (int w = 0; w < 8; w++) M.p_desc[8 * s + w] = desc[8 * i + w];
  M.p_state[s] = bad[i] ? 2 : 1;
}
// W = max(dim, 16) lanes per row: lane c copies descriptor float c, the first twelve also one double of the four vectors, lane 12 the flag
__global__ void map_set_lines_kernel(MapDev M, int n, int W, const int32_t* slot, const double* x0, const double* dir, const double* x1, const double* x2, const float* desc,
                                     const uint8_t* bad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)n * W) return;
  const int r = (int)(i / W), c = (int)(i % W), s = slot[r];
  if (c < M.dim) M.l_desc[(size_t)s * M.dim + c] = desc[(size_t)r * M.dim + c];
  if (c < 12) {
    const double* from = c < 3 ? x0 : c < 6 ? dir : c < 9 ? x1 : x2;
    double* to = c < 3 ? M.l_x0 : c < 6 ? M.l_dir : c < 9 ? M.l_x1 : M.l_x2;
    to[3 * s + c % 3] = from[3 * r + c % 3];
  }
  if (c == 12) M.l_bad[s] = bad[r] ? 1 : 0;
}
__global__ void map_set_keyframes_kernel(MapDev M, int n, const int32_t* slot, const u64* key, const uint8_t* bad, const int32_t* parent, const int32_t* cov_start, const int32_t* cov) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  M.k_key[s] = key[i]; M.k_bad[s] = bad[i] ? 1 : 0; M.k_parent[s] = parent[i];
  const int c0 = cov_start[i], nc = min(cov_start[i + 1] - c0, 10);          // GetBestCovisibilityKeyFrames(10)
  M.k_ncov[s] = nc;
  for (int j = 0; j < nc; j++) M.k_cov[10 * s + j] = cov[c0 + j];
}
__global__ void map_set_cov_kernel(MapDev M, int n, const int32_t* slot, const int32_t* cov_start, const int32_t* cov) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i], c0 = cov_start[i], nc = min(cov_start[i + 1] - c0, 10);
  M.k_ncov[s] = nc;
  for (int j = 0; j < nc; j++) M.k_cov[10 * s + j] = cov[c0 + j];
}
// lld_map_set_keyframe_features / _poses: mnId (id null: poses only), the pose as SE3Quat and its camera centre, "has features"
__global__ void map_set_kf_pose_kernel(MapBa Y, int n, const int32_t* slot, const u64* id, const double* qt, const float* ow) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  for (int c = 0; c < 7; c++) Y.k_qt[7 * (size_t)s + c] = qt[7 * (size_t)i + c];
  for (int c = 0; c < 3; c++) Y.k_ow[3 * (size_t)s + c] = ow[3 * (size_t)i + c];
  if (id) { Y.k_id[s] = id[i]; Y.k_feat[s] = 1; }
}
// lld_map_download_links: what Tracking::UpdateLocalMap reads of a keyframe besides its points - parent, cov row, child row - back to the host
__global__ void map_links_kernel(MapDev M, int n, const int32_t* slot, const int32_t* out_start, int32_t* parent, int32_t* ncov, int32_t* cov, int32_t* nchild, int32_t* child) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const int s = slot[i];
  const int2 row = M.k_child[s];
  const int room = out_start[i + 1] - out_start[i];
  if (threadIdx.x == 0) { parent[i] = M.k_parent[s]; ncov[i] = M.k_ncov[s]; nchild[i] = row.y; }
  if (threadIdx.x < 10) cov[10 * i + threadIdx.x] = (int)threadIdx.x < M.k_ncov[s] ? M.k_cov[10 * s + threadIdx.x] : -1;
  for (int j = threadIdx.x; j < min(row.y, room); j += blockDim.x) child[out_start[i] + j] = M.child_pool[row.x + j];
}

// ------------------------------------------------------------------------------------------------ UpdateLocalKeyFrames: the vote (:1730-1746)
// One lane per keypoint.  A bad MapPoint leaves the frame (mvpMapPoints[i] = NULL; mvbOutlier stays); an id the map does not hold is a temporal
// point of UpdateLastFrame and votes for nothing.  The first vote a keyframe receives puts its slot on the touched list.
__global__ void map_vote_kernel(MapDev M, TrackDev D) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= D.nt || !D.kp_has[k]) return;
  const int32_t id = D.kp_id[k];
  if (id < 0 || id >= M.max_pt) return;
  const uint8_t state = M.p_state[id];
  if (state == 0) return;
  if (state == 2) { D.kp_has[k] = 0; D.kp_id[k] = -1; atomicAdd(&M.fc[FC_CLEARED], 1); return; }
  const int2 row = M.p_obs[id];
  for (int j = 0; j < row.y; j++) {
    const int kf = M.obs_pool[row.x + j];
    if (atomicAdd(&M.cnt[kf], 1) == 0) M.touched[atomicAdd(&M.fc[FC_TOUCHED], 1)] = kf;
  }
}

// ------------------------------------------------------------------------------------------------ UpdateLocalKeyFrames: the list (:1748-1834)
// One workgroup.  LDS (dynamic): keys[1024] u64 | child[1024] int2 | slot[1024] | parent[1024] | 40 KB for the entries the extension loop can
// visit | scan[16] | marks (bit set over the keyframe slots = mnTrackReferenceForFrame == mCurrentFrame.mnId).  The loop visits entry i only
// while the list holds at most 80, and the list holds at least i + 1: never more than the first 80 entries.  For those (kVisit, padded) the
// 40 KB hold cov[kVisit][10], and the first kChildLds children of each with their keys, bad ones already dropped - fetched by the whole
// workgroup in parallel, so that the one wavefront of the loop reads LDS (a longer child list is walked in HBM behind that).
constexpr int kLkfThreads = 1024;
constexpr int kVisit = 96, kChildLds = 32;
static_assert(kVisit * 10 + kVisit * kChildLds * 3 <= 10240 && (kVisit * 10) % 2 == 0, "the visited entries' prefetch fits the 40 KB");
constexpr size_t kLkfLdsFixed = 1024 * 8 + 1024 * 8 + 1024 * 4 + 1024 * 4 + 1024 * 40 + 64 + 16;
__device__ __forceinline__ bool marked(const unsigned* marks, int s) { return (marks[s >> 5] >> (s & 31)) & 1u; }
__device__ __forceinline__ void mark(unsigned* marks, int s) { atomicOr(&marks[s >> 5], 1u << (s & 31)); }

__global__ __launch_bounds__(kLkfThreads) void map_local_keyframes_kernel(MapDev M, int mark_words) {
  extern __shared__ __align__(16) unsigned char lkf_lds[];
  u64* keys = reinterpret_cast<u64*>(lkf_lds);
  int2* s_child = reinterpret_cast<int2*>(keys + 1024);
  int* s_slot = reinterpret_cast<int*>(s_child + 1024);
  int* s_parent = s_slot + 1024;
  int* s_cov = s_parent + 1024;
  u64* s_ck = reinterpret_cast<u64*>(s_cov + kVisit * 10);
  int* s_cs = s_cov + kVisit * 10 + kVisit * kChildLds * 2;
  int* s_scan = s_cov + 10240;
  u64* s_best = reinterpret_cast<u64*>(s_scan + 16);
  unsigned* marks = reinterpret_cast<unsigned*>(s_best + 2);
  // the sorted keys are not read again: their 8 KB then hold what the loop appends (at most three per visited entry) and the listed slots
  int* s_app = reinterpret_cast<int*>(keys);
  int* s_lslot = reinterpret_cast<int*>(keys) + 512;
  const int tid = threadIdx.x;
  const int nv = M.fc[FC_TOUCHED];
  if (nv == 0 || nv > kMaxVoted) {
    // keyframeCounter.empty(): the routine returns, list and reference keyframe stay (:1748).  Too many: nothing is listed, the status says so.
    for (int t = tid; t < nv; t += kLkfThreads) M.cnt[M.touched[t]] = 0;
    if (tid == 0) { M.st[ST_STATUS] = nv ? LLD_LOCAL_MAP_KEYFRAME_OVERFLOW : 0; M.st[ST_VOTED] = nv; M.st[ST_CLEARED] = M.fc[FC_CLEARED]; M.st[ST_REF] = -1; M.st[ST_EMPTY] = nv == 0; }
    return;
  }
  int npad = 2; while (npad < nv) npad <<= 1;
  for (int t = tid; t < npad; t += kLkfThreads) {
    const int s = t < nv ? M.touched[t] : -1;
    keys[t] = t < nv ? M.k_key[s] : ~0ull; s_slot[t] = s;
  }
  for (int w = tid; w < mark_words; w += kLkfThreads) marks[w] = 0;
  if (tid == 0) s_best[0] = 0;
  __syncthreads();
  lld_wave::bitonic_sort_pairs<kLkfThreads>(keys, s_slot, npad);       // std::map<KeyFrame*,int> iteration order
  // the voted keyframes in that order: bad ones are neither listed nor marked nor candidates for the maximum (:1763-1764)
  const int slot = tid < nv ? s_slot[tid] : -1;
  int votes = 0; bool listed = false;
  if (slot >= 0) { votes = M.cnt[slot]; M.cnt[slot] = 0; listed = M.k_bad[slot] == 0; }
  int n_listed;
  const int pos = lld_wave::block_excl_scan<kLkfThreads>(listed ? 1 : 0, s_scan, n_listed);
  if (listed) atomicMax(s_best, ((u64)(unsigned)votes << 32) | (unsigned)(0x7fffffff - tid));   // it->second > max: the first of the greatest
  if (listed) {
    M.lkf[pos] = slot; mark(marks, slot);
    s_parent[pos] = M.k_parent[slot]; s_child[pos] = M.k_child[slot]; s_lslot[pos] = slot;
  }
  __syncthreads();
  // cov and children of the entries the loop can visit, one entry of one list per lane: three dependent loads, once, side by side
  for (int w = tid; w < kVisit * 10; w += kLkfThreads) {
    const int e = w / 10, j = w % 10;
    int c = -1;
    if (e < n_listed) {
      const int sl = s_lslot[e];
      if (j < M.k_ncov[sl]) { c = M.k_cov[10 * sl + j]; if (M.k_bad[c]) c = -1; }   // if(!pNeighKF->isBad())
    }
    s_cov[w] = c;
  }
  for (int w = tid; w < kVisit * kChildLds; w += kLkfThreads) {
    const int e = w / kChildLds, j = w % kChildLds;
    int ch = -1; u64 key = ~0ull;
    if (e < n_listed) {
      const int2 row = s_child[e];
      if (j < row.y) { ch = M.child_pool[row.x + j]; if (M.k_bad[ch]) ch = -1; else key = M.k_key[ch]; }
    }
    s_cs[w] = ch; s_ck[w] = key;
  }
  __syncthreads();
  const u64 best = s_best[0];
  const int ref = best ? s_slot[0x7fffffff - (int)(unsigned)(best & 0xffffffffu)] : -1;
  int n_list = n_listed;
  if (tid < 64) {
    // the order-dependent part, one wavefront, everything it reads about the voted entries already in LDS.  The end iterator was taken before
    // the pushes: only the voted entries are visited (:1778).
    const int lane = tid;
    for (int i = 0; i < n_listed; i++) {
      if (n_list > 80) break;                                          // if(mvpLocalKeyFrames.size()>80) break;
      const int c = lane < 10 ? s_cov[10 * i + lane] : -1;
      const u64 bc = __ballot(c >= 0 && !marked(marks, c));
      if (bc) {
        const int cs = __shfl(c, __ffsll((long long)bc) - 1);
        if (lane == 0) { s_app[n_list - n_listed] = cs; mark(marks, cs); }
        n_list++;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      // std::set<KeyFrame*> order: the child with the smallest key that is neither bad nor marked
      const int2 row = s_child[i];
      u64 ck = ~0ull; int cslot = -1;
      if (lane < kChildLds) {
        const int ch = s_cs[i * kChildLds + lane];
        if (ch >= 0 && !marked(marks, ch)) { cslot = ch; ck = s_ck[i * kChildLds + lane]; }
      }
      for (int j = kChildLds + lane; j < row.y; j += 64) {
        const int ch = M.child_pool[row.x + j];
        if (M.k_bad[ch] || marked(marks, ch)) continue;
        const u64 key = M.k_key[ch];
        if (cslot < 0 || key < ck) { ck = key; cslot = ch; }
      }
      const u64 has = __ballot(cslot >= 0);
      if (has) {
        const u64 mk = lld_wave::min(cslot >= 0 ? ck : ~0ull);
        const u64 who = __ballot(cslot >= 0 && ck == mk);
        const int cs = __shfl(cslot, __ffsll((long long)who) - 1);
        if (lane == 0) { s_app[n_list - n_listed] = cs; mark(marks, cs); }
        n_list++;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      const int par = s_parent[i];
      if (par >= 0 && !marked(marks, par)) {                           // the parent's isBad is not read (:1819-1826)
        if (lane == 0) { s_app[n_list - n_listed] = par; mark(marks, par); }
        n_list++;
        break;                                                         // this break leaves the OUTER loop (:1824)
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    // (inside the loop nothing goes to HBM: a store there would sit in front of every wavefront fence)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (int j = lane; j < n_list - n_listed; j += 64) M.lkf[n_listed + j] = s_app[j];
    if (lane == 0) {
      M.st[ST_STATUS] = 0; M.st[ST_VOTED] = nv; M.st[ST_NKF] = n_list; M.st[ST_CLEARED] = M.fc[FC_CLEARED]; M.st[ST_REF] = ref; M.st[ST_EMPTY] = 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------ UpdateLocalPoints (:1684-1722)
// mnTrackReferenceForFrame of a point = the first (list position, keypoint index) at which the walk meets it: a 64-bit atomicMin per slot.
__device__ __forceinline__ bool lkf_block(const MapDev& M, int& p, int& kf) {
  if (M.st[ST_STATUS] & LLD_LOCAL_MAP_KEYFRAME_OVERFLOW) return false;
  p = blockIdx.x;
  if (p >= M.st[ST_NKF]) return false;
  kf = M.lkf[p];
  return true;
}
__global__ __launch_bounds__(256) void map_first_kernel(MapDev M) {
  int p, kf;
  if (!lkf_block(M, p, kf)) return;
  const int2 rp = M.k_pt[kf], rl = M.k_ln[kf];
  for (int j = threadIdx.x; j < rp.y; j += 256) {
    const int s = M.kpt_pool[rp.x + j];
    if (s >= 0 && M.p_state[s] == 1) atomicMin(&M.p_first[s], ((u64)p << 32) | (unsigned)j);
  }
  for (int j = threadIdx.x; j < rl.y; j += 256) {
    const int s = M.kln_pool[rl.x + j];
    if (s >= 0 && !M.l_bad[s]) atomicMin(&M.l_first[s], ((u64)p << 32) | (unsigned)j);
  }
}
__global__ __launch_bounds__(256) void map_count_kernel(MapDev M) {
  __shared__ int lds[4];
  int p, kf;
  if (!lkf_block(M, p, kf)) return;
  const int2 rp = M.k_pt[kf], rl = M.k_ln[kf];
  int np = 0, nl = 0;
  for (int j = threadIdx.x; j < rp.y; j += 256) {
    const int s = M.kpt_pool[rp.x + j];
    if (s >= 0 && M.p_state[s] == 1 && M.p_first[s] == (((u64)p << 32) | (unsigned)j)) np++;
  }
  for (int j = threadIdx.x; j < rl.y; j += 256) {
    const int s = M.kln_pool[rl.x + j];
    if (s >= 0 && !M.l_bad[s] && M.l_first[s] == (((u64)p << 32) | (unsigned)j)) nl++;
  }
  np = lld_wave::block_sum(np, lds); nl = lld_wave::block_sum(nl, lds);
  if (threadIdx.x == 0) { M.lkf_np[p] = np; M.lkf_nl[p] = nl; }
}
// Ordered compaction: every workgroup sums the counts of the keyframes before its own, then writes its keyframe's first occurrences in
// keypoint order.  A list longer than its limit is not written at all (never a silently shortened local map): the status names it.
__global__ __launch_bounds__(256) void map_write_kernel(MapDev M) {
  __shared__ int lds[4];
  if (M.st[ST_STATUS] & LLD_LOCAL_MAP_KEYFRAME_OVERFLOW) return;
  const int p = blockIdx.x, nkf = M.st[ST_NKF], tid = threadIdx.x;
  if (p >= nkf && p != 0) return;
  int a = 0, b = 0, ta = 0, tb = 0;
  for (int q = tid; q < nkf; q += 256) { const int c = M.lkf_np[q], d = M.lkf_nl[q]; ta += c; tb += d; if (q < p) { a += c; b += d; } }
  a = lld_wave::block_sum(a, lds); b = lld_wave::block_sum(b, lds); ta = lld_wave::block_sum(ta, lds); tb = lld_wave::block_sum(tb, lds);
  if (p == 0 && tid == 0) {
    M.st[ST_NPTS] = ta; M.st[ST_NLNS] = tb;
    if (ta > M.max_lp) atomicOr(&M.st[ST_STATUS], LLD_LOCAL_MAP_POINT_OVERFLOW);
    if (tb > M.max_ll) atomicOr(&M.st[ST_STATUS], LLD_LOCAL_MAP_LINE_OVERFLOW);
  }
  if (p >= nkf) return;
  const int kf = M.lkf[p];
  const int2 rp = M.k_pt[kf], rl = M.k_ln[kf];
  if (ta <= M.max_lp)
    for (int j0 = 0, run = a; j0 < rp.y; j0 += 256) {
      const int j = j0 + tid;
      int s = -1; bool w = false;
      if (j < rp.y) { s = M.kpt_pool[rp.x + j]; w = s >= 0 && M.p_state[s] == 1 && M.p_first[s] == (((u64)p << 32) | (unsigned)j); }
      int tot; const int r = lld_wave::block_excl_scan<256>(w ? 1 : 0, lds, tot);
      if (w) M.lpts[run + r] = s;
      run += tot;
    }
  if (tb <= M.max_ll)
    for (int j0 = 0, run = b; j0 < rl.y; j0 += 256) {
      const int j = j0 + tid;
      int s = -1; bool w = false;
      if (j < rl.y) { s = M.kln_pool[rl.x + j]; w = s >= 0 && !M.l_bad[s] && M.l_first[s] == (((u64)p << 32) | (unsigned)j); }
      int tot; const int r = lld_wave::block_excl_scan<256>(w ? 1 : 0, lds, tot);
      if (w) M.llns[run + r] = s;
      run += tot;
    }
}

// ------------------------------------------------------------------------------------------------ stage 2's inputs from the tables
__global__ void map_gather_kernel(MapDev M, lld_map_dev::GatherDst G) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = M.st[ST_STATUS] == 0;
  const int np = ok ? M.st[ST_NPTS] : 0, nl = ok ? M.st[ST_NLNS] : 0;
  if (i == 0) M.st[ST_STAGE2] = ok;
  if (i < (long long)M.max_lp * 8) {
    const int q = (int)(i >> 3), w = (int)(i & 7);
    const int s = q < np ? M.lpts[q] : -1;
    G.desc[i] = s >= 0 ? M.p_desc[8 * (size_t)s + w] : 0u;
    if (w < 3) { G.pos[3 * q + w] = s >= 0 ? M.p_pos[3 * s + w] : 0.f; G.nrm[3 * q + w] = s >= 0 ? M.p_nrm[3 * s + w] : 0.f; }
    if (w == 3) { G.maxd[q] = s >= 0 ? M.p_maxd[s] : 0.f; G.mind[q] = s >= 0 ? M.p_mind[s] : 0.f; }
    if (w == 4) { G.obs[q] = s >= 0 && M.p_obs[s].y > 0; G.skip[q] = s < 0; G.id[q] = s; }
  }
  const int W = max(M.dim, 16);
  if (G.lid && i < (long long)M.max_ll * W) {
    const int q = (int)(i / W), c = (int)(i % W);
    const int s = q < nl ? M.llns[q] : -1;
    if (c < M.dim) G.ldesc[(size_t)q * M.dim + c] = s >= 0 ? M.l_desc[(size_t)s * M.dim + c] : 0.f;
    if (c < 12) {
      const double* from = c < 3 ? M.l_x0 : c < 6 ? M.l_dir : c < 9 ? M.l_x1 : M.l_x2;
      double* to = c < 3 ? G.x0 : c < 6 ? G.dir : c < 9 ? G.x1 : G.x2;
      to[3 * q + c % 3] = s >= 0 ? from[3 * s + c % 3] : 0.0;
    }
    if (c == 12) { G.lskip[q] = s < 0; G.lid[q] = s; }
  }
  if (!ok) {
    if (i < G.nt) { G.bk_kp[i] = G.kp_has[i]; G.kp_has[i] = 0; }
    if (i < G.nl) { G.bk_ln[i] = G.ln_has[i]; G.ln_has[i] = 0; }
  }
}
__global__ void map_restore_kernel(MapDev M, lld_map_dev::GatherDst G) {
  if (M.st[ST_STATUS] == 0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < G.nt) G.kp_has[i] = G.bk_kp[i];
  if (i < G.nl) G.ln_has[i] = G.bk_ln[i];
  if (i < G.n_rec2) G.rec2[i] = 0;
}

bool starts_ok(int n, const int32_t* start) {
  if (!start || start[0] != 0) return false;
  for (int i = 0; i < n; i++) if (start[i + 1] < start[i]) return false;
  return true;
}
bool entries_in(const int32_t* v, int n, int lo, int hi) {        // lo <= v < hi
  for (int i = 0; i < n; i++) if (v[i] < lo || v[i] >= hi) return false;
  return true;
}

}  // namespace

int lld_map_dev::RowPool::launch(hipStream_t st, const UploadBlock& B, const PoolPlan& P) const {
  if (P.n_up <= 0) return LLD_OK;
  hipLaunchKernelGGL(map_rows_kernel, dim3(std::min(P.n_up, 4096)), dim3(64), 0, st, P.n_up, B.dev(P.slot), B.dev(P.row), B.dev(P.src), B.dev(P.data), d_row, d_pool);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

namespace {

using lld_map_dev::slots_ok;

int up_begin(lld_map* m, UploadBlock& B) {
  B.end_upload();
  if (m->upload_pending) { LLD_HIP_TRY(hipEventSynchronize(m->uploaded)); m->upload_pending = false; }
  const int st = m->up.grow(m->ctx->stream, B.size, B.size); if (st) return st;
  B.bind(m->up.h, m->up.d);
  return LLD_OK;
}
int up_submit(lld_map* m, const UploadBlock& B) {
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, m->ctx->stream));
  LLD_HIP_TRY(hipEventRecord(m->uploaded, m->ctx->stream)); m->upload_pending = true;
  return LLD_OK;
}

int tables_reset(lld_map* m) {
  hipStream_t st = m->ctx->stream;
  LLD_HIP_TRY(hipMemsetAsync(m->d_tables, 0, m->tables_bytes, st));
  LLD_HIP_TRY(hipMemsetAsync(m->D.k_bad, 1, (size_t)m->lim.max_keyframes, st));    // never set: neither listed nor a neighbour
  LLD_HIP_TRY(hipMemsetAsync(m->D.l_bad, 1, (size_t)std::max(m->lim.max_lines, 1), st));
  LLD_HIP_TRY(hipMemsetAsync(m->D.k_parent, 0xff, (size_t)m->lim.max_keyframes * 4, st));
  LLD_HIP_TRY(hipMemsetAsync(m->D.st + ST_REF, 0xff, 4, st));
  m->obs.reset(); m->child.reset(); m->kpt.reset(); m->kln.reset();
  m->mutations++; m->win.valid = false;
  if (m->d_ref) LLD_HIP_TRY(hipMemsetAsync(m->d_ref, 0xff, (size_t)m->lim.max_points * 4, st));
  std::fill(m->kf_set.begin(), m->kf_set.end(), (uint8_t)0); std::fill(m->kf_key.begin(), m->kf_key.end(), 0ull);
  if (m->d_ext) {
    LLD_HIP_TRY(hipMemsetAsync(m->d_ext, 0, m->ext_bytes, st));
    m->idx.reset(); m->koct.reset(); m->kdep.reset();
  }
  if (m->d_ba) {
    LLD_HIP_TRY(hipMemsetAsync(m->d_ba, 0, m->ba_bytes, st));
    LLD_HIP_TRY(hipMemsetAsync(m->Y.l_nobs, 0xff, (size_t)std::max(m->lim.max_lines, 1) * 4, st));     // no observation row
    m->kuvr.reset(); m->kkl.reset(); m->lobs.reset(); m->lidx.reset();
    std::fill(m->kf_feat.begin(), m->kf_feat.end(), (uint8_t)0);
  }
  if (m->d_desc) {
    LLD_HIP_TRY(hipMemsetAsync(m->d_desc, 0, m->desc_bytes, st));
    m->kdesc.reset(); m->kldesc.reset();
  }
  return LLD_OK;
}

// The culling tables and their pools, on the first call that fills them.  A failure leaves the map as it was.
int ext_ensure(lld_map* m) {
  if (m->d_ext) return LLD_OK;
  const size_t nk = m->lim.max_keyframes, np = m->lim.max_points;
  m->idx.init((int)np, m->lim.max_observations); m->koct.init((int)nk, m->lim.max_kf_points); m->kdep.init((int)nk, m->lim.max_kf_points);
  UploadBlock B;
  const auto pnobs = B.take<int32_t>(np); const auto pidx = B.take<int2>(np); const auto ipool = B.take<int32_t>(m->idx.mirror.size());
  const auto koct = B.take<int2>(nk), kdep = B.take<int2>(nk); const auto opool = B.take<int32_t>(m->koct.mirror.size()), dpool = B.take<int32_t>(m->kdep.mirror.size());
  const auto kthd = B.take<float>(nk);
  char* d = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d), B.size) != hipSuccess) return LLD_ERR_ALLOC;
  if (hipMemsetAsync(d, 0, B.size, m->ctx->stream) != hipSuccess) { (void)hipFree(d); return LLD_ERR_HIP; }
  m->d_ext = d; m->ext_bytes = B.size;
  B.bind(nullptr, d);
  MapExt& X = m->X;
  X.p_nobs = B.dev(pnobs); X.p_idx = B.dev(pidx); X.idx_pool = B.dev(ipool); X.k_oct = B.dev(koct); X.k_dep = B.dev(kdep); X.oct_pool = B.dev(opool);
  X.dep_pool = B.dev(dpool); X.k_thd = B.dev(kthd);
  m->idx.d_row = X.p_idx; m->idx.d_pool = X.idx_pool; m->koct.d_row = X.k_oct; m->koct.d_pool = X.oct_pool; m->kdep.d_row = X.k_dep; m->kdep.d_pool = X.dep_pool;
  return LLD_OK;
}

// The bundle-adjustment tables and their pools, on the first call that fills them.  A failure leaves the map as it was.
int ba_ensure(lld_map* m) {
  if (m->d_ba) return LLD_OK;
  if (m->lim.max_kf_points > (1 << 28) || m->lim.max_kf_lines > (1 << 26)) return LLD_ERR_UNSUPPORTED;      // twice the pools' totals stay int32 offsets
  const size_t nk = m->lim.max_keyframes, nl = std::max(m->lim.max_lines, 1);
  m->kuvr.init((int)nk, 3 * (int64_t)m->lim.max_kf_points); m->kkl.init((int)nk, 10 * (int64_t)m->lim.max_kf_lines);
  m->lobs.init((int)nl, m->lim.max_kf_lines); m->lidx.init((int)nl, m->lim.max_kf_lines);
  m->kf_feat.assign(nk, 0);
  UploadBlock B;
  const auto kid = B.take<u64>(nk); const auto kqt = B.take<double>(nk, 7); const auto kow = B.take<float>(nk, 3); const auto kfeat = B.take<uint8_t>(nk); const auto kuvr = B.take<int2>(nk), kkl = B.take<int2>(nk);
  const auto upool = B.take<int32_t>(m->kuvr.mirror.size()), kpool = B.take<int32_t>(m->kkl.mirror.size());
  const auto lobs = B.take<int2>(nl), lidx = B.take<int2>(nl); const auto opool = B.take<int32_t>(m->lobs.mirror.size()), ipool = B.take<int32_t>(m->lidx.mirror.size());
  const auto lnobs = B.take<int32_t>(nl);
  const auto kmark = B.take<u64>(nk); const auto kcam = B.take<int32_t>(nk), fixed = B.take<int32_t>(nk), fixed_bad = B.take<int32_t>(nk);
  char* d = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d), B.size) != hipSuccess) return LLD_ERR_ALLOC;
  B.bind(nullptr, d);
  if (hipMemsetAsync(d, 0, B.size, m->ctx->stream) != hipSuccess || hipMemsetAsync(B.dev(lnobs), 0xff, nl * 4, m->ctx->stream) != hipSuccess) { (void)hipFree(d); return LLD_ERR_HIP; }
  m->d_ba = d; m->ba_bytes = B.size; m->mark_off = kmark.off; m->mark_bytes = nk * sizeof(u64);
  MapBa& Y = m->Y;
  Y.k_id = B.dev(kid); Y.k_qt = B.dev(kqt); Y.k_ow = B.dev(kow); Y.k_feat = B.dev(kfeat); Y.k_uvr = B.dev(kuvr); Y.k_kl = B.dev(kkl); Y.uvr_pool = B.dev(upool); Y.kl_pool = B.dev(kpool);
  Y.l_obs = B.dev(lobs); Y.l_idx = B.dev(lidx); Y.lobs_pool = B.dev(opool); Y.lidx_pool = B.dev(ipool); Y.l_nobs = B.dev(lnobs);
  Y.k_mark = B.dev(kmark); Y.k_cam = B.dev(kcam); Y.fixed = B.dev(fixed); Y.fixed_bad = B.dev(fixed_bad);
  m->kuvr.d_row = Y.k_uvr; m->kuvr.d_pool = Y.uvr_pool; m->kkl.d_row = Y.k_kl; m->kkl.d_pool = Y.kl_pool;
  m->lobs.d_row = Y.l_obs; m->lobs.d_pool = Y.lobs_pool; m->lidx.d_row = Y.l_idx; m->lidx.d_pool = Y.lidx_pool;
  return LLD_OK;
}

// The keyframes' descriptor rows and their two pools, on the first call that fills one of them.  A failure leaves the map as it was.
int desc_ensure(lld_map* m) {
  if (m->d_desc) return LLD_OK;
  const int64_t lim_p = 8 * (int64_t)m->lim.max_kf_points, lim_l = (int64_t)m->lim.line_dim * m->lim.max_kf_lines;
  if (2 * lim_p > INT32_MAX || 2 * lim_l > INT32_MAX) return LLD_ERR_UNSUPPORTED;                    // twice the pools' totals stay int32 offsets
  const size_t nk = m->lim.max_keyframes;
  m->kdesc.init((int)nk, lim_p); m->kldesc.init((int)nk, lim_l);
  UploadBlock B;
  const auto kd = B.take<int2>(nk), kl = B.take<int2>(nk); const auto dpool = B.take<int32_t>(m->kdesc.mirror.size()), lpool = B.take<int32_t>(m->kldesc.mirror.size());
  char* d = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d), B.size) != hipSuccess) return LLD_ERR_ALLOC;
  if (hipMemsetAsync(d, 0, B.size, m->ctx->stream) != hipSuccess) { (void)hipFree(d); return LLD_ERR_HIP; }
  m->d_desc = d; m->desc_bytes = B.size;
  B.bind(nullptr, d);
  lld_map_dev::MapDesc& Z = m->Z;
  Z.k_desc = B.dev(kd); Z.kdesc_pool = B.dev(dpool); Z.k_ldesc = B.dev(kl); Z.kldesc_pool = B.dev(lpool);
  m->kdesc.d_row = Z.k_desc; m->kdesc.d_pool = Z.kdesc_pool; m->kldesc.d_row = Z.k_ldesc; m->kldesc.d_pool = Z.kldesc_pool;
  return LLD_OK;
}

// lld_map_set_keyframe_descriptors / _line_descriptors: `per` words per feature of the keyframe's row `feat` (its point or line row), into `pool`
int set_kf_desc_rows(lld_map* m, RowPool lld_map::*pool, const RowPool& feat, int per, int32_t n, const int32_t* slot, const int32_t* start, const int32_t* desc) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !starts_ok(n, start) || (start[n] > 0 && !desc)) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_kf, m->epoch, n, slot)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (!m->kf_set[slot[i]] || start[i + 1] - start[i] != feat.len[slot[i]]) return LLD_ERR_INVALID;   // one row per feature of a keyframe the map holds
  const int64_t limit = pool == &lld_map::kdesc ? 8 * (int64_t)m->lim.max_kf_points : (int64_t)m->lim.line_dim * m->lim.max_kf_lines;
  if (2 * limit > INT32_MAX || (int64_t)per * start[n] > limit) return LLD_ERR_UNSUPPORTED;           // (what desc_ensure refuses, before the scaled starts are formed)
  std::vector<int32_t> ws((size_t)n + 1);
  for (int i = 0; i <= n; i++) ws[i] = per * start[i];
  PoolPlan P;
  // the limits first, the allocation behind them: a fresh pool is empty, so the call's own words are its live total
  if (m->d_desc && !(m->*pool).plan(n, slot, ws.data(), P)) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  const bool fresh = !m->d_desc;
  int st = desc_ensure(m); if (st) return st;
  RowPool& R = m->*pool;
  if (fresh && !R.plan(n, slot, ws.data(), P)) return LLD_ERR_UNSUPPORTED;                            // (cannot happen: checked above)
  UploadBlock B;
  R.reserve(B, P);
  st = up_begin(m, B); if (st) return st;
  m->mutations++;
  R.commit(B, P, n, slot, ws.data(), desc);
  st = up_submit(m, B);
  if (!st) st = R.launch(m->ctx->stream, B, P);
  if (st) m->poisoned = true;                                          // the host's rows are ahead of the device's
  return st;
}

}  // namespace

namespace lld_map_dev {
Limits limits(const lld_map* m) { return {m->ctx, m->lim.max_local_points, m->lim.max_local_lines, m->lim.line_dim, m->poisoned, m->serial}; }
int gather_launch(hipStream_t st, const lld_map* m, const GatherDst& G) {
  const MapDev& M = m->D;
  const long long n = std::max(std::max((long long)M.max_lp * 8, (long long)M.max_ll * std::max(M.dim, 16)), (long long)std::max(std::max(G.nt, G.nl), 1));
  hipLaunchKernelGGL(map_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, M, G);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}
int restore_launch(hipStream_t st, const lld_map* m, const GatherDst& G) {
  const int n = std::max(std::max(G.nt, G.nl), std::max(G.n_rec2, 1));
  hipLaunchKernelGGL(map_restore_kernel, dim3((n + 255) / 256), dim3(256), 0, st, m->D, G);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}
}  // namespace lld_map_dev

extern "C" {

int lld_map_create(lld_ctx* ctx, const lld_map_limits* L, lld_map** out) {
  if (!ctx || !L || !out) return LLD_ERR_INVALID;
  *out = nullptr;
  if (L->max_keyframes < 1 || L->max_points < 1 || L->max_lines < 0 || L->line_dim < 1 || L->max_observations < 0 || L->max_kf_points < 0 || L->max_kf_lines < 0 ||
      L->max_children < 0 || L->max_local_points < 1 || L->max_local_lines < 0) return LLD_ERR_INVALID;
  if (L->line_dim > 128 || L->max_keyframes > kMaxKeyframes || L->max_local_points > (1 << 20) || L->max_local_lines > (1 << 20)) return LLD_ERR_UNSUPPORTED;
  const int64_t big = (int64_t)1 << 29;                               // twice a total stays an int32 offset
  if (L->max_observations > big || L->max_kf_points > big || L->max_kf_lines > big || L->max_children > big) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  lld_map* m = new lld_map();
  m->ctx = ctx; m->lim = *L;
  const size_t nk = L->max_keyframes, np = L->max_points, nl = std::max(L->max_lines, 1), dim = L->line_dim, nlp = L->max_local_points, nll = std::max(L->max_local_lines, 1);
  m->obs.init((int)np, L->max_observations); m->child.init((int)nk, L->max_children); m->kpt.init((int)nk, L->max_kf_points); m->kln.init((int)nk, L->max_kf_lines);
  m->stamp_pt.assign(np, 0); m->stamp_kf.assign(nk, 0); m->stamp_ln.assign(L->max_lines, 0); m->kf_set.assign(nk, 0); m->kf_key.assign(nk, 0);
  UploadBlock B;
  const auto ppos = B.take<float>(np, 3), pnrm = B.take<float>(np, 3), pmind = B.take<float>(np), pmaxd = B.take<float>(np); const auto pdesc = B.take<uint32_t>(np, 8);
  const auto pstate = B.take<uint8_t>(np); const auto pobs = B.take<int2>(np); const auto opool = B.take<int32_t>(m->obs.mirror.size());
  const auto lx0 = B.take<double>(nl, 3), ldir = B.take<double>(nl, 3), lx1 = B.take<double>(nl, 3), lx2 = B.take<double>(nl, 3); const auto ldesc = B.take<float>(nl, dim);
  const auto lbad = B.take<uint8_t>(nl);
  const auto kkey = B.take<u64>(nk); const auto kbad = B.take<uint8_t>(nk); const auto kpar = B.take<int32_t>(nk), kcov = B.take<int32_t>(nk, 10), kncov = B.take<int32_t>(nk);
  const auto kch = B.take<int2>(nk), kp = B.take<int2>(nk), kl = B.take<int2>(nk);
  const auto cpool = B.take<int32_t>(m->child.mirror.size()), ppool = B.take<int32_t>(m->kpt.mirror.size()), lpool = B.take<int32_t>(m->kln.mirror.size());
  const auto cnt = B.take<int32_t>(nk), touched = B.take<int32_t>(nk), fc = B.take<int32_t>(FC_WORDS);
  m->first_off = B.size;
  const auto pfirst = B.take<u64>(np), lfirst = B.take<u64>(nl);
  m->first_bytes = B.size - m->first_off;
  const auto knp = B.take<int32_t>(kLkfCap), knl = B.take<int32_t>(kLkfCap);
  m->down_off = B.size;
  const auto st = B.take<int32_t>(ST_WORDS), lkf = B.take<int32_t>(kLkfCap), lpts = B.take<int32_t>(nlp), llns = B.take<int32_t>(nll);
  m->down_bytes = B.size - m->down_off; m->o_lkf = lkf.off - m->down_off; m->o_lpts = lpts.off - m->down_off; m->o_llns = llns.off - m->down_off;
  m->tables_bytes = B.size;
  m->lkf_lds = kLkfLdsFixed + (((size_t)nk + 31) / 32) * 4;
  int status = LLD_OK;
  if (hipMalloc(reinterpret_cast<void**>(&m->d_tables), B.size) != hipSuccess) { m->d_tables = nullptr; status = LLD_ERR_ALLOC; }
  if (!status && hipHostMalloc(reinterpret_cast<void**>(&m->h_down), m->down_bytes, hipHostMallocDefault) != hipSuccess) { m->h_down = nullptr; status = LLD_ERR_ALLOC; }
  if (!status && hipEventCreateWithFlags(&m->uploaded, hipEventDisableTiming) != hipSuccess) { m->uploaded = nullptr; status = LLD_ERR_HIP; }
  if (!status && hipFuncSetAttribute(reinterpret_cast<const void*>(&map_local_keyframes_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(kLkfLdsFixed + kMaxKeyframes / 8)) != hipSuccess) status = LLD_ERR_HIP;
  if (status) { lld_map_destroy(m); return status; }
  B.bind(nullptr, m->d_tables);
  MapDev& D = m->D;
  D.max_kf = (int)nk; D.max_pt = (int)np; D.max_ln = L->max_lines; D.dim = (int)dim; D.max_lp = L->max_local_points; D.max_ll = L->max_local_lines;
  D.p_pos = B.dev(ppos); D.p_nrm = B.dev(pnrm); D.p_mind = B.dev(pmind); D.p_maxd = B.dev(pmaxd); D.p_desc = B.dev(pdesc); D.p_state = B.dev(pstate); D.p_obs = B.dev(pobs);
  D.obs_pool = B.dev(opool);
  D.l_x0 = B.dev(lx0); D.l_dir = B.dev(ldir); D.l_x1 = B.dev(lx1); D.l_x2 = B.dev(lx2); D.l_desc = B.dev(ldesc); D.l_bad = B.dev(lbad);
  D.k_key = B.dev(kkey); D.k_bad = B.dev(kbad); D.k_parent = B.dev(kpar); D.k_cov = B.dev(kcov); D.k_ncov = B.dev(kncov); D.k_child = B.dev(kch); D.k_pt = B.dev(kp); D.k_ln = B.dev(kl);
  D.child_pool = B.dev(cpool); D.kpt_pool = B.dev(ppool); D.kln_pool = B.dev(lpool);
  D.cnt = B.dev(cnt); D.touched = B.dev(touched); D.fc = B.dev(fc); D.p_first = B.dev(pfirst); D.l_first = B.dev(lfirst);
  D.lkf = B.dev(lkf); D.lkf_np = B.dev(knp); D.lkf_nl = B.dev(knl); D.lpts = B.dev(lpts); D.llns = B.dev(llns); D.st = B.dev(st);
  m->obs.d_row = D.p_obs; m->obs.d_pool = D.obs_pool; m->child.d_row = D.k_child; m->child.d_pool = D.child_pool;
  m->kpt.d_row = D.k_pt; m->kpt.d_pool = D.kpt_pool; m->kln.d_row = D.k_ln; m->kln.d_pool = D.kln_pool;
  status = tables_reset(m);
  if (status) { lld_map_destroy(m); return status; }
  *out = m;
  return LLD_OK;
}

void lld_map_destroy(lld_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  if (m->d_tables) (void)hipFree(m->d_tables);
  if (m->d_ext) (void)hipFree(m->d_ext);
  if (m->d_ba) (void)hipFree(m->d_ba);
  if (m->d_ref) (void)hipFree(m->d_ref);
  if (m->d_desc) (void)hipFree(m->d_desc);
  m->ba.release(); m->ap.release(); m->rf.release(); m->fu.release(); m->up.release();
  if (m->h_down) (void)hipHostFree(m->h_down);
  if (m->uploaded) (void)hipEventDestroy(m->uploaded);
  delete m;
}

int lld_map_clear(lld_map* m) {
  if (!m) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  const int st = tables_reset(m);
  if (!st) m->poisoned = false;                                      // host rows and device tables are empty together again
  return st;
}

int lld_map_set_points(lld_map* m, int32_t n, const int32_t* slot, const float* world_pos, const float* normal, const float* min_distance, const float* max_distance,
                       const uint32_t* desc, const uint8_t* bad) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !world_pos || !normal || !min_distance || !max_distance || !desc || !bad) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_pt, m->epoch, n, slot)) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  UploadBlock B;
  const auto s = B.take<int32_t>(n); const auto pos = B.take<float>(n, 3), nrm = B.take<float>(n, 3), mind = B.take<float>(n), maxd = B.take<float>(n);
  const auto d = B.take<uint32_t>(n, 8); const auto b = B.take<uint8_t>(n);
  int st = up_begin(m, B); if (st) return st;
  m->mutations++;
  B.stage(s, slot); B.stage(pos, world_pos); B.stage(nrm, normal); B.stage(mind, min_distance); B.stage(maxd, max_distance); B.stage(d, desc); B.stage(b, bad);
  st = up_submit(m, B); if (st) return st;
  hipLaunchKernelGGL(map_set_points_kernel, dim3((n + 255) / 256), dim3(256), 0, m->ctx->stream, m->D, n, B.dev(s), B.dev(pos), B.dev(nrm), B.dev(mind), B.dev(maxd), B.dev(d), B.dev(b));
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

int lld_map_set_observations(lld_map* m, int32_t n, const int32_t* slot, const int32_t* start, const int32_t* kf_slot) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !starts_ok(n, start) || (start[n] > 0 && !kf_slot)) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_pt, m->epoch, n, slot) || !entries_in(kf_slot, start[n], 0, m->lim.max_keyframes)) return LLD_ERR_INVALID;
  PoolPlan P;
  if (!m->obs.plan(n, slot, start, P)) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  UploadBlock B;
  m->obs.reserve(B, P);
  const auto drop = B.take<int32_t>(m->d_ext ? n : 0);              // with the culling tables: these rows carry no keypoint indices any more
  int st = up_begin(m, B); if (st) return st;
  m->mutations++;
  m->obs.commit(B, P, n, slot, start, kf_slot);
  if (m->d_ext) {
    B.stage(drop, slot);
    for (int i = 0; i < n; i++) { m->idx.live -= m->idx.len[slot[i]]; m->idx.len[slot[i]] = 0; }
  }
  st = up_submit(m, B);
  if (!st) st = m->obs.launch(m->ctx->stream, B, P);
  if (!st && m->d_ext) {
    hipLaunchKernelGGL(map_drop_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, m->ctx->stream, n, B.dev(drop), m->X.p_idx);
    if (hipGetLastError() != hipSuccess) st = LLD_ERR_HIP;
  }
  if (st) m->poisoned = true;                                        // the host's rows are ahead of the device's
  return st;
}

int lld_map_set_observations_indexed(lld_map* m, int32_t n, const int32_t* slot, const int32_t* start, const int32_t* kf_slot, const int32_t* kp_index,
                                     const int32_t* n_obs) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !n_obs || !starts_ok(n, start) || (start[n] > 0 && (!kf_slot || !kp_index))) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_pt, m->epoch, n, slot) || !entries_in(kf_slot, start[n], 0, m->lim.max_keyframes)) return LLD_ERR_INVALID;
  for (int i = 0; i < start[n]; i++) if (kp_index[i] < 0) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (n_obs[i] < 0) return LLD_ERR_INVALID;
  PoolPlan P, Pi;
  if (!m->obs.plan(n, slot, start, P)) return LLD_ERR_UNSUPPORTED;
  // every limit is held before anything is allocated: a fresh index pool is empty, so the call's own entries are its live total
  if (m->d_ext ? !m->idx.plan(n, slot, start, Pi) : start[n] > m->lim.max_observations) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  const bool fresh = !m->d_ext;
  int st = ext_ensure(m); if (st) return st;
  if (fresh && !m->idx.plan(n, slot, start, Pi)) return LLD_ERR_UNSUPPORTED;     // (cannot happen: checked above)
  UploadBlock B;
  m->obs.reserve(B, P); m->idx.reserve(B, Pi);
  const auto s = B.take<int32_t>(n), no = B.take<int32_t>(n);
  st = up_begin(m, B); if (st) return st;
  m->mutations++;
  m->obs.commit(B, P, n, slot, start, kf_slot); m->idx.commit(B, Pi, n, slot, start, kp_index);
  B.stage(s, slot); B.stage(no, n_obs);
  st = up_submit(m, B);
  hipStream_t stream = m->ctx->stream;
  if (!st) st = m->obs.launch(stream, B, P);
  if (!st) st = m->idx.launch(stream, B, Pi);
  if (!st) {
    hipLaunchKernelGGL(map_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, B.dev(s), B.dev(no), m->X.p_nobs);
    if (hipGetLastError() != hipSuccess) st = LLD_ERR_HIP;
  }
  if (st) m->poisoned = true;                                        // the host's rows are ahead of the device's
  return st;
}

int lld_map_set_keyframe_keypoints(lld_map* m, int32_t n, const int32_t* slot, const int32_t* start, const int32_t* octave, const float* depth, const float* th_depth) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !th_depth || !starts_ok(n, start) || (start[n] > 0 && (!octave || !depth))) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_kf, m->epoch, n, slot)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (!m->kf_set[slot[i]] || start[i + 1] - start[i] != m->kpt.len[slot[i]]) return LLD_ERR_INVALID;   // one entry per keypoint of a keyframe the map holds
  PoolPlan Po, Pd;
  // as above: the limits first, the allocation behind them
  if (m->d_ext ? (!m->koct.plan(n, slot, start, Po) || !m->kdep.plan(n, slot, start, Pd)) : start[n] > m->lim.max_kf_points) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  const bool fresh = !m->d_ext;
  int st = ext_ensure(m); if (st) return st;
  if (fresh && (!m->koct.plan(n, slot, start, Po) || !m->kdep.plan(n, slot, start, Pd))) return LLD_ERR_UNSUPPORTED;      // (cannot happen: checked above)
  UploadBlock B;
  m->koct.reserve(B, Po); m->kdep.reserve(B, Pd);
  const auto s = B.take<int32_t>(n); const auto thd = B.take<float>(n);
  st = up_begin(m, B); if (st) return st;
  m->mutations++;
  m->koct.commit(B, Po, n, slot, start, octave); m->kdep.commit(B, Pd, n, slot, start, reinterpret_cast<const int32_t*>(depth));    // a float travels as its bit pattern
  B.stage(s, slot); B.stage(thd, th_depth);
  st = up_submit(m, B);
  hipStream_t stream = m->ctx->stream;
  if (!st) st = m->koct.launch(stream, B, Po);
  if (!st) st = m->kdep.launch(stream, B, Pd);
  if (!st) {
    hipLaunchKernelGGL(map_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, B.dev(s), reinterpret_cast<const int32_t*>(B.dev(thd)),
                       reinterpret_cast<int32_t*>(m->X.k_thd));
    if (hipGetLastError() != hipSuccess) st = LLD_ERR_HIP;
  }
  if (st) m->poisoned = true;
  return st;
}

int lld_map_set_covisibles(lld_map* m, int32_t n, const int32_t* slot, const int32_t* cov_start, const int32_t* cov) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !starts_ok(n, cov_start) || (cov_start[n] > 0 && !cov)) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_kf, m->epoch, n, slot) || !entries_in(cov, cov_start[n], 0, m->lim.max_keyframes)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (!m->kf_set[slot[i]]) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  UploadBlock B;
  const auto s = B.take<int32_t>(n), cs = B.take<int32_t>((size_t)n + 1), cv = B.take<int32_t>(cov_start[n]);
  int st = up_begin(m, B); if (st) return st;
  m->mutations++;
  B.stage(s, slot); B.stage(cs, cov_start); B.stage(cv, cov);
  st = up_submit(m, B); if (st) return st;
  hipLaunchKernelGGL(map_set_cov_kernel, dim3((n + 255) / 256), dim3(256), 0, m->ctx->stream, m->D, n, B.dev(s), B.dev(cs), B.dev(cv));
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

int lld_map_set_keyframes(lld_map* m, int32_t n, const int32_t* slot, const uint64_t* order_key, const uint8_t* bad, const int32_t* parent, const int32_t* cov_start,
                          const int32_t* cov, const int32_t* child_start, const int32_t* child, const int32_t* point_start, const int32_t* point,
                          const int32_t* line_start, const int32_t* line) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !order_key || !bad || !parent) return LLD_ERR_INVALID;
  if (!starts_ok(n, cov_start) || !starts_ok(n, child_start) || !starts_ok(n, point_start) || !starts_ok(n, line_start)) return LLD_ERR_INVALID;
  if ((cov_start[n] > 0 && !cov) || (child_start[n] > 0 && !child) || (point_start[n] > 0 && !point) || (line_start[n] > 0 && !line)) return LLD_ERR_INVALID;
  const int nk = m->lim.max_keyframes;
  if (!slots_ok(m->stamp_kf, m->epoch, n, slot)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (parent[i] < -1 || parent[i] >= nk || order_key[i] == ~0ull) return LLD_ERR_INVALID;
  if (!entries_in(cov, cov_start[n], 0, nk) || !entries_in(child, child_start[n], 0, nk) || !entries_in(point, point_start[n], -1, m->lim.max_points) ||
      !entries_in(line, line_start[n], -1, m->lim.max_lines)) return LLD_ERR_INVALID;
  PoolPlan Pc, Pp, Pl;
  if (!m->child.plan(n, slot, child_start, Pc) || !m->kpt.plan(n, slot, point_start, Pp) || !m->kln.plan(n, slot, line_start, Pl)) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  UploadBlock B;
  const auto s = B.take<int32_t>(n); const auto key = B.take<u64>(n); const auto b = B.take<uint8_t>(n); const auto par = B.take<int32_t>(n), cs = B.take<int32_t>((size_t)n + 1),
             cv = B.take<int32_t>(cov_start[n]);
  m->child.reserve(B, Pc); m->kpt.reserve(B, Pp); m->kln.reserve(B, Pl);
  int st = up_begin(m, B); if (st) return st;
  m->mutations++;
  B.stage(s, slot); B.stage(key, reinterpret_cast<const u64*>(order_key)); B.stage(b, bad); B.stage(par, parent); B.stage(cs, cov_start); B.stage(cv, cov);
  m->child.commit(B, Pc, n, slot, child_start, child); m->kpt.commit(B, Pp, n, slot, point_start, point); m->kln.commit(B, Pl, n, slot, line_start, line);
  for (int i = 0; i < n; i++) { m->kf_set[slot[i]] = 1; m->kf_key[slot[i]] = order_key[i]; }
  st = up_submit(m, B);
  hipStream_t stream = m->ctx->stream;
  if (!st) {
    hipLaunchKernelGGL(map_set_keyframes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, m->D, n, B.dev(s), B.dev(key), B.dev(b), B.dev(par), B.dev(cs), B.dev(cv));
    if (hipGetLastError() != hipSuccess) st = LLD_ERR_HIP;
  }
  if (!st) st = m->child.launch(stream, B, Pc);
  if (!st) st = m->kpt.launch(stream, B, Pp);
  if (!st) st = m->kln.launch(stream, B, Pl);
  if (st) m->poisoned = true;                                        // the host's rows are ahead of the device's
  return st;
}

int lld_map_set_lines(lld_map* m, int32_t n, const int32_t* slot, const double* x0, const double* dir, const double* x1, const double* x2, const float* desc, const uint8_t* bad) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !x0 || !dir || !x1 || !x2 || !desc || !bad) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_ln, m->epoch, n, slot)) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  const int dim = m->lim.line_dim, W = std::max(dim, 16);
  UploadBlock B;
  const auto s = B.take<int32_t>(n); const auto a0 = B.take<double>(n, 3), ad = B.take<double>(n, 3), a1 = B.take<double>(n, 3), a2 = B.take<double>(n, 3);
  const auto d = B.take<float>(n, dim); const auto b = B.take<uint8_t>(n);
  int st = up_begin(m, B); if (st) return st;
  m->mutations++;
  B.stage(s, slot); B.stage(a0, x0); B.stage(ad, dir); B.stage(a1, x1); B.stage(a2, x2); B.stage(d, desc); B.stage(b, bad);
  st = up_submit(m, B); if (st) return st;
  const long long total = (long long)n * W;
  hipLaunchKernelGGL(map_set_lines_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, m->ctx->stream, m->D, n, W, B.dev(s), B.dev(a0), B.dev(ad), B.dev(a1), B.dev(a2),
                     B.dev(d), B.dev(b));
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

int lld_map_set_keyframe_features(lld_map* m, int32_t n, const int32_t* slot, const uint64_t* mn_id, const float* Tcw, const int32_t* kp_start, const float* kp_uvr,
                                  const int32_t* kl_start, const float* kl_left, const float* kl_right, const int32_t* kl_octave) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !mn_id || !Tcw || !starts_ok(n, kp_start) || !starts_ok(n, kl_start)) return LLD_ERR_INVALID;
  if ((kp_start[n] > 0 && !kp_uvr) || (kl_start[n] > 0 && (!kl_left || !kl_right || !kl_octave))) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_kf, m->epoch, n, slot)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++)                                         // one entry per keypoint and per keyline of a keyframe the map holds
    if (!m->kf_set[slot[i]] || kp_start[i + 1] - kp_start[i] != m->kpt.len[slot[i]] || kl_start[i + 1] - kl_start[i] != m->kln.len[slot[i]]) return LLD_ERR_INVALID;
  // the rows as the pools hold them: three words per keypoint, ten per keyline (the totals are the point and line rows', so they fit)
  std::vector<int32_t> us((size_t)n + 1), ks((size_t)n + 1), kl((size_t)kl_start[n] * 10);
  for (int i = 0; i <= n; i++) { us[i] = 3 * kp_start[i]; ks[i] = 10 * kl_start[i]; }
  for (int k = 0; k < kl_start[n]; k++) {
    std::memcpy(&kl[10 * (size_t)k], kl_left + 4 * (size_t)k, 16); std::memcpy(&kl[10 * (size_t)k + 4], kl_right + 4 * (size_t)k, 16);
    kl[10 * (size_t)k + 8] = kl_octave[2 * (size_t)k]; kl[10 * (size_t)k + 9] = kl_octave[2 * (size_t)k + 1];
  }
  PoolPlan Pu, Pk;
  // the limits first, the allocation behind them: fresh pools are empty, and the rows' totals are bounded by the point and line rows' limits
  if (m->d_ba && (!m->kuvr.plan(n, slot, us.data(), Pu) || !m->kkl.plan(n, slot, ks.data(), Pk))) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  const bool fresh = !m->d_ba;
  int st = ba_ensure(m); if (st) return st;
  if (fresh && (!m->kuvr.plan(n, slot, us.data(), Pu) || !m->kkl.plan(n, slot, ks.data(), Pk))) return LLD_ERR_UNSUPPORTED;      // (cannot happen)
  UploadBlock B;
  m->kuvr.reserve(B, Pu); m->kkl.reserve(B, Pk);
  const auto s = B.take<int32_t>(n); const auto id = B.take<u64>(n); const auto qt = B.take<double>(n, 7); const auto ow = B.take<float>(n, 3);
  st = up_begin(m, B); if (st) return st;
  m->mutations++;
  m->kuvr.commit(B, Pu, n, slot, us.data(), reinterpret_cast<const int32_t*>(kp_uvr));          // a float travels as its bit pattern
  m->kkl.commit(B, Pk, n, slot, ks.data(), kl.data());
  B.stage(s, slot); B.stage(id, reinterpret_cast<const u64*>(mn_id));
  for (int i = 0; i < n; i++) {
    lld_se3_from_tcw_f32(Tcw + 16 * (size_t)i, B.host(qt) + 7 * (size_t)i); lld::camera_centre(Tcw + 16 * (size_t)i, B.host(ow) + 3 * (size_t)i);
    m->kf_feat[slot[i]] = 1;
  }
  st = up_submit(m, B);
  hipStream_t stream = m->ctx->stream;
  if (!st) st = m->kuvr.launch(stream, B, Pu);
  if (!st) st = m->kkl.launch(stream, B, Pk);
  if (!st) {
    hipLaunchKernelGGL(map_set_kf_pose_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, m->Y, n, B.dev(s), B.dev(id), B.dev(qt), B.dev(ow));
    if (hipGetLastError() != hipSuccess) st = LLD_ERR_HIP;
  }
  if (st) m->poisoned = true;                                        // the host's rows are ahead of the device's
  return st;
}

int lld_map_set_keyframe_poses(lld_map* m, int32_t n, const int32_t* slot, const float* Tcw) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !Tcw) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_kf, m->epoch, n, slot)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (!m->d_ba || !m->kf_feat[slot[i]]) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  UploadBlock B;
  const auto s = B.take<int32_t>(n); const auto qt = B.take<double>(n, 7); const auto ow = B.take<float>(n, 3);
  int st = up_begin(m, B); if (st) return st;
  m->mutations++;
  B.stage(s, slot);
  for (int i = 0; i < n; i++) { lld_se3_from_tcw_f32(Tcw + 16 * (size_t)i, B.host(qt) + 7 * (size_t)i); lld::camera_centre(Tcw + 16 * (size_t)i, B.host(ow) + 3 * (size_t)i); }
  st = up_submit(m, B); if (st) return st;
  hipLaunchKernelGGL(map_set_kf_pose_kernel, dim3((n + 255) / 256), dim3(256), 0, m->ctx->stream, m->Y, n, B.dev(s), (const u64*)nullptr, B.dev(qt), B.dev(ow));
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

int lld_map_set_line_observations(lld_map* m, int32_t n, const int32_t* slot, const int32_t* start, const int32_t* kf_slot, const int32_t* line_index,
                                  const int32_t* n_obs) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !n_obs || !starts_ok(n, start) || (start[n] > 0 && (!kf_slot || !line_index))) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_ln, m->epoch, n, slot) || !entries_in(kf_slot, start[n], 0, m->lim.max_keyframes)) return LLD_ERR_INVALID;
  for (int i = 0; i < start[n]; i++) if (line_index[i] < 0) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (n_obs[i] < 0) return LLD_ERR_INVALID;
  PoolPlan Po, Pi;
  if (m->d_ba ? (!m->lobs.plan(n, slot, start, Po) || !m->lidx.plan(n, slot, start, Pi)) : start[n] > m->lim.max_kf_lines) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  const bool fresh = !m->d_ba;
  int st = ba_ensure(m); if (st) return st;
  if (fresh && (!m->lobs.plan(n, slot, start, Po) || !m->lidx.plan(n, slot, start, Pi))) return LLD_ERR_UNSUPPORTED;      // (cannot happen: checked above)
  UploadBlock B;
  m->lobs.reserve(B, Po); m->lidx.reserve(B, Pi);
  const auto s = B.take<int32_t>(n), no = B.take<int32_t>(n);
  st = up_begin(m, B); if (st) return st;
  m->mutations++;
  m->lobs.commit(B, Po, n, slot, start, kf_slot); m->lidx.commit(B, Pi, n, slot, start, line_index);
  B.stage(s, slot); B.stage(no, n_obs);
  st = up_submit(m, B);
  hipStream_t stream = m->ctx->stream;
  if (!st) st = m->lobs.launch(stream, B, Po);
  if (!st) st = m->lidx.launch(stream, B, Pi);
  if (!st) {
    hipLaunchKernelGGL(map_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, n, B.dev(s), B.dev(no), m->Y.l_nobs);
    if (hipGetLastError() != hipSuccess) st = LLD_ERR_HIP;
  }
  if (st) m->poisoned = true;                                        // the host's rows are ahead of the device's
  return st;
}

int lld_map_set_point_refs(lld_map* m, int32_t n, const int32_t* slot, const int32_t* ref_kf) {
  if (!m || n < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !ref_kf) return LLD_ERR_INVALID;
  if (!slots_ok(m->stamp_pt, m->epoch, n, slot) || !entries_in(ref_kf, n, -1, m->lim.max_keyframes)) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  if (!m->d_ref) {                                                    // the first call: every slot unknown.  A failure leaves the map as it was.
    int32_t* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), (size_t)m->lim.max_points * 4) != hipSuccess) return LLD_ERR_ALLOC;
    if (hipMemsetAsync(d, 0xff, (size_t)m->lim.max_points * 4, m->ctx->stream) != hipSuccess) { (void)hipFree(d); return LLD_ERR_HIP; }
    m->d_ref = d;
  }
  UploadBlock B;
  const auto s = B.take<int32_t>(n), r = B.take<int32_t>(n);
  int st = up_begin(m, B); if (st) return st;
  m->mutations++;
  B.stage(s, slot); B.stage(r, ref_kf);
  st = up_submit(m, B); if (st) return st;
  hipLaunchKernelGGL(map_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, m->ctx->stream, n, B.dev(s), B.dev(r), m->d_ref);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

int lld_map_set_keyframe_descriptors(lld_map* m, int32_t n, const int32_t* slot, const int32_t* start, const uint32_t* desc) {
  if (!m) return LLD_ERR_INVALID;
  return set_kf_desc_rows(m, &lld_map::kdesc, m->kpt, 8, n, slot, start, reinterpret_cast<const int32_t*>(desc));
}

int lld_map_set_keyframe_line_descriptors(lld_map* m, int32_t n, const int32_t* slot, const int32_t* start, const float* desc) {
  if (!m) return LLD_ERR_INVALID;
  return set_kf_desc_rows(m, &lld_map::kldesc, m->kln, m->lim.line_dim, n, slot, start, reinterpret_cast<const int32_t*>(desc));    // a float travels as its bit pattern
}

int lld_frame_track_update_local_map(lld_frame* f, lld_map* m) {
  if (!f || !m || f->ctx != m->ctx) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  lld_frame_track_state* S = f->track;
  if (!S || !S->stage1_queued) return LLD_ERR_INVALID;               // the frame's MapPoints come from a stage 1
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  hipStream_t st = m->ctx->stream;
  const MapDev& M = m->D;
  LLD_HIP_TRY(hipMemsetAsync(M.fc, 0, FC_WORDS * 4, st));
  LLD_HIP_TRY(hipMemsetAsync(m->d_tables + m->first_off, 0xff, m->first_bytes, st));
  if (f->nt > 0) hipLaunchKernelGGL(map_vote_kernel, dim3((f->nt + 255) / 256), dim3(256), 0, st, M, S->D);
  hipLaunchKernelGGL(map_local_keyframes_kernel, dim3(1), dim3(kLkfThreads), m->lkf_lds, st, M, (M.max_kf + 31) / 32);
  hipLaunchKernelGGL(map_first_kernel, dim3(kLkfCap), dim3(256), 0, st, M);
  hipLaunchKernelGGL(map_count_kernel, dim3(kLkfCap), dim3(256), 0, st, M);
  hipLaunchKernelGGL(map_write_kernel, dim3(kLkfCap), dim3(256), 0, st, M);
  LLD_HIP_TRY(hipGetLastError());
  S->local_map_of = m; S->local_map_serial = ++m->serial;
  return LLD_OK;
}

int lld_frame_local_map_download(lld_frame* f, lld_map* m, lld_local_map_result* r) {
  if (!f || !m || !r || f->ctx != m->ctx) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(m->ctx->device));
  const bool lists = r->local_keyframes || r->local_points || r->local_lines;
  LLD_HIP_TRY(hipMemcpyAsync(m->h_down, m->d_tables + m->down_off, lists ? m->down_bytes : (size_t)ST_WORDS * 4, hipMemcpyDeviceToHost, m->ctx->stream));
  lld_frame_track_state* S = f->track;
  if (S && S->stage1_queued) {
    lld_track_result s2; lld_track_result* p2 = r->stage2;
    // mp_in_view holds max_local_points bytes: it is filled when the frame's last stage 2 was sized by this map (not by a longer host list)
    if (p2 && S->stage2_queued) { s2 = *p2; s2.mp_in_view = S->n_in_view <= m->lim.max_local_points ? r->mp_in_view : nullptr; p2 = &s2; }
    const int st = lld_frame_track_download(f, r->stage1, S->stage2_queued ? p2 : nullptr); if (st) return st;
    if (r->stage2 && S->stage2_queued) { s2.mp_in_view = r->stage2->mp_in_view; *r->stage2 = s2; }
  } else {
    LLD_HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  }
  const int32_t* st = reinterpret_cast<const int32_t*>(m->h_down);
  r->status = st[ST_STATUS]; r->n_voted = st[ST_VOTED]; r->n_local_keyframes = st[ST_NKF]; r->n_local_points = st[ST_NPTS]; r->n_local_lines = st[ST_NLNS];
  r->n_bad_cleared = st[ST_CLEARED]; r->ref_keyframe = st[ST_REF]; r->vote_empty = st[ST_EMPTY];
  r->stage2_ran = (S && S->stage2_queued) ? st[ST_STAGE2] : 0;
  const bool kf_ok = !(r->status & LLD_LOCAL_MAP_KEYFRAME_OVERFLOW);
  if (r->local_keyframes) std::memcpy(r->local_keyframes, m->h_down + m->o_lkf, (size_t)std::min(std::max(r->n_local_keyframes, 0), kLkfCap) * 4);
  if (r->local_points && kf_ok && r->n_local_points <= m->lim.max_local_points) std::memcpy(r->local_points, m->h_down + m->o_lpts, (size_t)r->n_local_points * 4);
  if (r->local_lines && kf_ok && r->n_local_lines <= m->lim.max_local_lines) std::memcpy(r->local_lines, m->h_down + m->o_llns, (size_t)r->n_local_lines * 4);
  return LLD_OK;
}

int lld_map_download_links(lld_map* m, int32_t n, const int32_t* slot, int32_t* parent, int32_t* n_cov, int32_t* cov, int32_t* child_start, int32_t child_capacity,
                           int32_t* child) {
  if (!m || n < 0 || child_capacity < 0) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !parent || !n_cov || !cov || !child_start || (child_capacity > 0 && !child)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (slot[i] < 0 || slot[i] >= m->lim.max_keyframes || !m->kf_set[slot[i]]) return LLD_ERR_INVALID;
  // the child rows' lengths are the host's (every update before this call is queued before its kernel); the contents come from the device
  std::vector<int32_t> start((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) start[i + 1] = start[i] + m->child.len[slot[i]];
  std::memcpy(child_start, start.data(), ((size_t)n + 1) * 4);
  if (start[n] > child_capacity) return LLD_ERR_INVALID;              // only child_start is written
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  UploadBlock B;
  const auto i_s = B.take<int32_t>(n), i_st = B.take<int32_t>((size_t)n + 1);
  B.end_upload();
  const size_t out_off = B.size;
  const auto r_par = B.take<int32_t>(n), r_nc = B.take<int32_t>(n), r_cov = B.take<int32_t>(n, 10), r_nch = B.take<int32_t>(n), r_ch = B.take<int32_t>((size_t)start[n]);
  int st;
  void* hb; st = lld_ctx_pinned(ctx, B.size, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind((char*)hb, (char*)db);
  B.stage(i_s, slot); B.stage(i_st, start.data());
  hipStream_t sm = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, sm));
  hipLaunchKernelGGL(map_links_kernel, dim3(n), dim3(64), 0, sm, m->D, n, B.dev(i_s), B.dev(i_st), B.dev(r_par), B.dev(r_nc), B.dev(r_cov), B.dev(r_nch), B.dev(r_ch));
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(B.h + out_off, B.d + out_off, B.size - out_off, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  const int32_t* nch = B.host(r_nch);
  for (int i = 0; i < n; i++) if (nch[i] != start[i + 1] - start[i]) return LLD_ERR_HIP;       // the device's rows are not the host's: never with a sound map
  std::memcpy(parent, B.host(r_par), (size_t)n * 4); std::memcpy(n_cov, B.host(r_nc), (size_t)n * 4); std::memcpy(cov, B.host(r_cov), (size_t)n * 40);
  if (start[n]) std::memcpy(child, B.host(r_ch), (size_t)start[n] * 4);
  return LLD_OK;
}

}  // extern "C"
