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
// Covisibility on the same tables (lld_map_covisibility: KeyFrame::UpdateConnections, src/KeyFrame.cc:312-402, and the redundancy count of
// LocalMapping::KeyFrameCulling, src/LocalMapping.cc:646-694): map_covis_query_kernel, one workgroup per query, and map_covis_pack_kernel.
// The culling part reads four members more (MapExt: keypoint index per observation, nObs per point, octave / depth / mThDepth per keyframe);
// their tables and pools are allocated by the first lld_map_set_observations_indexed / lld_map_set_keyframe_keypoints, never by lld_map_create.
#include "lld_common.h"
#include "lld_frame_track_state.h"
#include "lld_map_internal.h"
#include "lld_track_internal.h"
#include "lld_upload_block.h"
#include "lld_wave.h"

namespace {

using lld_track::Span;
using lld_track::TrackDev;
using lld_track::UploadBlock;
typedef unsigned long long u64;

constexpr int kMaxVoted = 1024;                    // voted keyframes one workgroup sorts in LDS
constexpr int kLkfCap = LLD_MAP_MAX_LOCAL_KEYFRAMES;
static_assert(kLkfCap >= kMaxVoted + 3 * 81, "list capacity");    // the list: the voted ones, and at most three more per entry visited while it holds <= 80
constexpr int kMaxKeyframes = 1 << 18;             // the marks are a bit set in LDS: 32 KB at this size
enum { ST_STATUS = 0, ST_VOTED, ST_NKF, ST_NPTS, ST_NLNS, ST_CLEARED, ST_REF, ST_EMPTY, ST_STAGE2, ST_WORDS = 16 };
enum { FC_TOUCHED = 0, FC_CLEARED, FC_WORDS = 4 };

struct MapDev {
  int max_kf, max_pt, max_ln, dim, max_lp, max_ll;
  float* p_pos; float* p_nrm; float* p_mind; float* p_maxd; uint32_t* p_desc; uint8_t* p_state; int2* p_obs; int32_t* obs_pool;
  double* l_x0; double* l_dir; double* l_x1; double* l_x2; float* l_desc; uint8_t* l_bad;
  u64* k_key; uint8_t* k_bad; int32_t* k_parent; int32_t* k_cov; int32_t* k_ncov; int2* k_child; int2* k_pt; int2* k_ln;
  int32_t* child_pool; int32_t* kpt_pool; int32_t* kln_pool;
  // per call: vote counters (zero between calls), the slots that got a first vote, first occurrences, the lists
  int32_t* cnt; int32_t* touched; int32_t* fc; u64* p_first; u64* l_first;
  int32_t* lkf; int32_t* lkf_np; int32_t* lkf_nl; int32_t* lpts; int32_t* llns; int32_t* st;
};

// The culling tables.  All null until the first lld_map_set_observations_indexed / lld_map_set_keyframe_keypoints.
//   point slot s     p_nobs = MapPoint::Observations(), p_idx = (offset, length) in idx_pool of the keypoint indices, parallel to the p_obs row
//   keyframe slot s  k_oct / k_dep = (offset, length) in oct_pool / dep_pool of mvKeysUn[i].octave / the bits of mvDepth[i], k_thd = mThDepth
struct MapExt {
  int32_t* p_nobs; int2* p_idx; int32_t* idx_pool; int2* k_oct; int2* k_dep; int32_t* oct_pool; int32_t* dep_pool; float* k_thd;
};

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
// map_covis_pack_kernel: one workgroup per query, exclusive sums of the per-query counts, then the staged lists to their packed places.
// No workgroup reads what another workgroup of the same kernel writes, so a query's result cannot depend on the batch.
constexpr int kCovThreads = 256, kCovGroup = 16, kCovGroups = kCovThreads / kCovGroup;
constexpr int kCovMax = LLD_MAP_COVIS_MAX_CONNECTED, kCovCells = 2 * kCovMax;
static_assert((kCovCells & (kCovCells - 1)) == 0 && kCovMax + 2 * kCovThreads < kCovCells, "the table keeps empty cells behind an overflow");
constexpr size_t kCovLds = (size_t)kCovCells * 8;
enum { CS_CLAIMED = 0, CS_NO_KP, CS_MPS, CS_RED, CS_WORDS };

struct CovArgs {
  const int32_t* query; const int32_t* stage_off;
  int32_t n_queries, monocular, th, th_obs, has_ext; uint32_t flags; double ratio;
  int32_t* st_slot; int32_t* st_cnt;         // staging: the table's cells in use, in cell order
  int32_t* st_kf; int32_t* st_w; u64* st_key;     // ... the same in map order; the ordered list as weight << 32 | rank
  int32_t* cnt_conn; int32_t* cnt_ord;
  int32_t* n_max; int32_t* kf_max; uint8_t* updated; uint8_t* status; int32_t* n_mps; int32_t* n_red; uint8_t* redundant;
  int32_t cap_conn, cap_ord;
  int32_t* conn_start; int32_t* ord_start; int32_t* totals; int32_t* conn_kf; int32_t* conn_w; int32_t* ord_kf; int32_t* ord_w;
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
          if (A.monocular || !(depth > th_depth || depth < 0.f)) {
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
    if (t == 0) {
      const int nm = no_kp ? 0 : s_st[CS_MPS], nr = no_kp ? 0 : s_st[CS_RED];
      A.n_mps[q] = nm; A.n_red[q] = nr;
      A.redundant[q] = ((double)nr > A.ratio * (double)nm) ? 1 : 0;    // nRedundantObservations > 0.9*nMPs: int against double
    }
  }
  if (!conn) { if (t == 0) A.status[q] = (uint8_t)status; return; }
  const int claimed = s_st[CS_CLAIMED];
  if (claimed == 0 || claimed > kCovMax) {
    // keyframeCounter.empty() (:346-347), or more keyframes than the table answers for: no entries, the cov row stays
    if (t == 0) {
      A.cnt_conn[q] = 0; A.cnt_ord[q] = 0; A.n_max[q] = 0; A.kf_max[q] = -1; A.updated[q] = 0;
      A.status[q] = (uint8_t)(status | (claimed ? LLD_MAP_COVIS_CONN_OVERFLOW : 0));
    }
    return;
  }
  // ---- the cells in use, to the staging
  const size_t off = (size_t)A.stage_off[q];
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
      A.st_kf[off + r] = slot; A.st_w[off + r] = w;
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
  for (int i = t; i < n_sel; i += kCovThreads) A.st_key[off + i] = keys[npad - 1 - i];
  if (t == 0) {
    if (!n_sel) A.st_key[off] = ((u64)(uint32_t)nmax << 32) | (uint32_t)rmax;
    A.cnt_conn[q] = n; A.cnt_ord[q] = n_ord; A.n_max[q] = nmax; A.kf_max[q] = A.st_kf[off + rmax]; A.updated[q] = 1;
    A.status[q] = (uint8_t)status;
  }
  if ((A.flags & LLD_MAP_COVIS_WRITE_COV) && status == 0) {
    // mvpOrderedConnectedKeyFrames' first ten: what Tracking::UpdateLocalMap reads as GetBestCovisibilityKeyFrames(10)
    const int nc = min(n_ord, 10);
    if (t < nc) M.k_cov[10 * own + t] = A.st_kf[off + (n_sel ? (uint32_t)keys[npad - 1 - t] : (uint32_t)rmax)];
    if (t == 0) M.k_ncov[own] = nc;
  }
}

__global__ __launch_bounds__(kCovThreads) void map_covis_pack_kernel(CovArgs A) {
  __shared__ int s_sum[4];
  const int q = blockIdx.x, t = threadIdx.x;
  int a = 0, b = 0, ta = 0, tb = 0;                                    // conn before q, ordered before q, the totals
  for (int j = t; j < A.n_queries; j += kCovThreads) {
    const int c = A.cnt_conn[j], d = A.cnt_ord[j];
    if (j < q) { a += c; b += d; }
    ta += c; tb += d;
  }
  a = lld_wave::block_sum(a, s_sum); b = lld_wave::block_sum(b, s_sum); ta = lld_wave::block_sum(ta, s_sum); tb = lld_wave::block_sum(tb, s_sum);
  if (t == 0) {
    A.conn_start[q] = a; A.ord_start[q] = b;
    if (q == A.n_queries - 1) { A.conn_start[A.n_queries] = ta; A.ord_start[A.n_queries] = tb; A.totals[0] = ta; A.totals[1] = tb; }
  }
  if (ta > A.cap_conn || tb > A.cap_ord) return;                       // a short capacity: only the totals go back
  const size_t off = (size_t)A.stage_off[q];
  const int nc = A.cnt_conn[q], no = A.cnt_ord[q];
  for (int i = t; i < nc; i += kCovThreads) { A.conn_kf[a + i] = A.st_kf[off + i]; A.conn_w[a + i] = A.st_w[off + i]; }
  for (int i = t; i < no; i += kCovThreads) {
    const u64 key = A.st_key[off + i];
    A.ord_kf[b + i] = A.st_kf[off + (uint32_t)key]; A.ord_w[b + i] = (int32_t)(key >> 32);
  }
}

// ------------------------------------------------------------------------------------------------ host: the pools
struct PoolPlan { bool repack = false; int n_up = 0; size_t n_data = 0; int64_t live_after = 0; Span<int32_t> slot, src, data; Span<int2> row; };

struct RowPool {
  int rows = 0; int64_t limit = 0, cap = 0, tail = 0, live = 0;
  std::vector<int32_t> off, len, rcap, mirror;
  int2* d_row = nullptr; int32_t* d_pool = nullptr;
  void init(int rows_, int64_t limit_) {
    rows = rows_; limit = limit_; cap = 2 * limit_; tail = live = 0;
    off.assign(rows, 0); len.assign(rows, 0); rcap.assign(rows, 0); mirror.assign((size_t)std::max<int64_t>(cap, 1), 0);
  }
  void reset() { tail = live = 0; std::fill(off.begin(), off.end(), 0); std::fill(len.begin(), len.end(), 0); std::fill(rcap.begin(), rcap.end(), 0); }
  // false: the live total would pass the limit.  Nothing is changed.
  bool plan(int n, const int32_t* slot, const int32_t* start, PoolPlan& P) const {
    int64_t lv = live, t = tail; size_t nd = 0;
    for (int i = 0; i < n; i++) {
      const int nl = start[i + 1] - start[i], s = slot[i];
      lv += nl - len[s]; nd += nl;
      if (nl > rcap[s]) t += nl;
    }
    if (lv > limit) return false;
    P.live_after = lv; P.repack = t > cap;
    P.n_up = P.repack ? rows : n; P.n_data = P.repack ? (size_t)lv : nd;
    return true;
  }
  void reserve(UploadBlock& B, PoolPlan& P) const {
    P.slot = B.take<int32_t>(P.n_up); P.src = B.take<int32_t>(P.n_up); P.row = B.take<int2>(P.n_up); P.data = B.take<int32_t>(P.n_data);
  }
  void commit(const UploadBlock& B, const PoolPlan& P, int n, const int32_t* slot, const int32_t* start, const int32_t* data) {
    int32_t* hs = B.host(P.slot); int32_t* hsrc = B.host(P.src); int2* hrow = B.host(P.row); int32_t* hd = B.host(P.data);
    if (!P.repack) {
      int32_t run = 0;
      for (int i = 0; i < n; i++) {
        const int nl = start[i + 1] - start[i], s = slot[i];
        if (nl > rcap[s]) { off[s] = (int32_t)tail; rcap[s] = nl; tail += nl; }
        len[s] = nl;
        if (nl) { std::memcpy(&mirror[off[s]], data + start[i], (size_t)nl * 4); std::memcpy(hd + run, data + start[i], (size_t)nl * 4); }
        hs[i] = s; hsrc[i] = run; hrow[i] = make_int2(off[s], nl); run += nl;
      }
    } else {
      // every row, packed tightly in slot order: the rows of this call from the caller's arrays, the others from the host copy
      std::vector<int32_t> upd(rows, -1), packed((size_t)std::max<int64_t>(cap, 1));
      for (int i = 0; i < n; i++) upd[slot[i]] = i;
      int32_t run = 0;
      for (int r = 0; r < rows; r++) {
        const int i = upd[r];
        const int nl = i >= 0 ? start[i + 1] - start[i] : len[r];
        const int32_t* from = i >= 0 ? data + start[i] : mirror.data() + off[r];
        if (nl) std::memcpy(&packed[run], from, (size_t)nl * 4);
        off[r] = run; len[r] = nl; rcap[r] = nl;
        hs[r] = r; hsrc[r] = run; hrow[r] = make_int2(run, nl); run += nl;
      }
      mirror.swap(packed); tail = run;
      if (run) std::memcpy(hd, mirror.data(), (size_t)run * 4);
    }
    live = P.live_after;
  }
  int launch(hipStream_t st, const UploadBlock& B, const PoolPlan& P) const {
    if (P.n_up <= 0) return LLD_OK;
    hipLaunchKernelGGL(map_rows_kernel, dim3(std::min(P.n_up, 4096)), dim3(64), 0, st, P.n_up, B.dev(P.slot), B.dev(P.row), B.dev(P.src), B.dev(P.data), d_row, d_pool);
    LLD_HIP_TRY(hipGetLastError());
    return LLD_OK;
  }
};

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

struct lld_map {
  lld_ctx* ctx = nullptr;
  lld_map_limits lim{};
  MapDev D{};
  char* d_tables = nullptr; size_t first_off = 0, first_bytes = 0, down_off = 0, down_bytes = 0, tables_bytes = 0;
  size_t o_lkf = 0, o_lpts = 0, o_llns = 0;                         // inside the downloaded span, which starts with st
  RowPool obs, child, kpt, kln;
  // the culling tables (MapExt): allocated by the first setter that fills them
  MapExt X{}; char* d_ext = nullptr; size_t ext_bytes = 0; RowPool idx, koct, kdep;
  std::vector<uint8_t> kf_set;              // lld_map_set_keyframes named the slot since the last clear
  bool cov_lds_set = false;                 // map_covis_query_kernel was granted its 64 KB of dynamic LDS
  std::vector<uint32_t> stamp_pt, stamp_kf, stamp_ln; uint32_t epoch = 0;
  // the staging of lld_map_set_*: pinned block, device block, the event of the last copy
  char* h_up = nullptr; size_t h_up_bytes = 0; char* d_up = nullptr; size_t d_up_bytes = 0; hipEvent_t uploaded = nullptr; bool upload_pending = false;
  char* h_down = nullptr;
  unsigned long long serial = 0;            // counts lld_frame_track_update_local_map calls: the lists in the tables are the last one's
  bool poisoned = false;                    // a HIP failure after the host bookkeeping of a set call moved: host copy and device tables may differ
  size_t lkf_lds = 0;
};

namespace {

// slots in range and no slot twice in one call
bool slots_ok(std::vector<uint32_t>& stamp, uint32_t& epoch, int n, const int32_t* slot) {
  if (++epoch == 0) { std::fill(stamp.begin(), stamp.end(), 0u); epoch = 1; }
  for (int i = 0; i < n; i++) {
    if (slot[i] < 0 || (size_t)slot[i] >= stamp.size() || stamp[slot[i]] == epoch) return false;
    stamp[slot[i]] = epoch;
  }
  return true;
}

int up_begin(lld_map* m, UploadBlock& B) {
  B.end_upload();
  if (m->upload_pending) { LLD_HIP_TRY(hipEventSynchronize(m->uploaded)); m->upload_pending = false; }
  if (B.size > m->h_up_bytes) {
    if (m->h_up) LLD_HIP_TRY(hipHostFree(m->h_up));
    m->h_up = nullptr; m->h_up_bytes = 0;
    const size_t want = B.size + (B.size >> 2) + 4096;
    if (hipHostMalloc(reinterpret_cast<void**>(&m->h_up), want, hipHostMallocDefault) != hipSuccess) { m->h_up = nullptr; return LLD_ERR_ALLOC; }
    m->h_up_bytes = want;
  }
  if (B.size > m->d_up_bytes) {
    LLD_HIP_TRY(hipStreamSynchronize(m->ctx->stream));                // the scatter kernels of an earlier call may still read the old block
    if (m->d_up) LLD_HIP_TRY(hipFree(m->d_up));
    m->d_up = nullptr; m->d_up_bytes = 0;
    const size_t want = B.size + (B.size >> 2) + 4096;
    if (hipMalloc(reinterpret_cast<void**>(&m->d_up), want) != hipSuccess) { m->d_up = nullptr; return LLD_ERR_ALLOC; }
    m->d_up_bytes = want;
  }
  B.bind(m->h_up, m->d_up);
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
  std::fill(m->kf_set.begin(), m->kf_set.end(), (uint8_t)0);
  if (m->d_ext) {
    LLD_HIP_TRY(hipMemsetAsync(m->d_ext, 0, m->ext_bytes, st));
    m->idx.reset(); m->koct.reset(); m->kdep.reset();
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
  m->stamp_pt.assign(np, 0); m->stamp_kf.assign(nk, 0); m->stamp_ln.assign(L->max_lines, 0); m->kf_set.assign(nk, 0);
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
  if (m->d_up) (void)hipFree(m->d_up);
  if (m->h_up) (void)hipHostFree(m->h_up);
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
  B.stage(s, slot); B.stage(key, reinterpret_cast<const u64*>(order_key)); B.stage(b, bad); B.stage(par, parent); B.stage(cs, cov_start); B.stage(cv, cov);
  m->child.commit(B, Pc, n, slot, child_start, child); m->kpt.commit(B, Pp, n, slot, point_start, point); m->kln.commit(B, Pl, n, slot, line_start, line);
  for (int i = 0; i < n; i++) m->kf_set[slot[i]] = 1;
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
  B.stage(s, slot); B.stage(a0, x0); B.stage(ad, dir); B.stage(a1, x1); B.stage(a2, x2); B.stage(d, desc); B.stage(b, bad);
  st = up_submit(m, B); if (st) return st;
  const long long total = (long long)n * W;
  hipLaunchKernelGGL(map_set_lines_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, m->ctx->stream, m->D, n, W, B.dev(s), B.dev(a0), B.dev(ad), B.dev(a1), B.dev(a2),
                     B.dev(d), B.dev(b));
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
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

int lld_map_covisibility(lld_map* m, const lld_map_covisibility_in* in, lld_map_covisibility_out* out) {
  if (!m || !in || !out) return LLD_ERR_INVALID;
  lld_covisibility_out* L = &out->lists;
  const int32_t nq = in->n_queries;
  const bool conn = (in->flags & LLD_COVIS_CONNECTIONS) != 0, cull = (in->flags & LLD_COVIS_CULLING) != 0;
  if (nq < 0) return LLD_ERR_INVALID;
  if ((in->flags & ~(uint32_t)(LLD_COVIS_CONNECTIONS | LLD_COVIS_CULLING | LLD_MAP_COVIS_WRITE_COV)) || !(conn || cull)) return LLD_ERR_INVALID;
  if ((in->flags & LLD_MAP_COVIS_WRITE_COV) && !conn) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (nq == 0) return LLD_OK;
  if (!in->kf_slot || !out->status) return LLD_ERR_INVALID;
  if (cull && (!L->n_mps || !L->n_redundant || !L->redundant)) return LLD_ERR_INVALID;
  if (conn) {
    if (L->conn_capacity < 0 || L->ordered_capacity < 0) return LLD_ERR_INVALID;
    if (!L->conn_start || !L->ordered_start || !L->n_max || !L->kf_max || !L->updated) return LLD_ERR_INVALID;
    if (L->conn_capacity > 0 && (!L->conn_kf || !L->conn_weight)) return LLD_ERR_INVALID;
    if (L->ordered_capacity > 0 && (!L->ordered_kf || !L->ordered_weight)) return LLD_ERR_INVALID;
  }
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
  const int32_t cap_conn = conn ? (int32_t)std::min<long long>(L->conn_capacity, stage_total) : 0;
  const int32_t cap_ord = conn ? (int32_t)std::min<long long>(L->ordered_capacity, stage_total) : 0;

  UploadBlock B;
  const auto i_q = B.take<int32_t>(nq), i_so = B.take<int32_t>(conn ? (size_t)nq + 1 : 0);
  B.end_upload();
  const size_t out_off = B.size;
  const auto r_cs = B.take<int32_t>(conn ? (size_t)nq + 1 : 0), r_rs = B.take<int32_t>(conn ? (size_t)nq + 1 : 0), r_tot = B.take<int32_t>(conn ? 2 : 0);
  const auto r_nm = B.take<int32_t>(conn ? nq : 0), r_km = B.take<int32_t>(conn ? nq : 0); const auto r_up = B.take<uint8_t>(conn ? nq : 0), r_st = B.take<uint8_t>(nq);
  const auto r_mp = B.take<int32_t>(cull ? nq : 0), r_rd = B.take<int32_t>(cull ? nq : 0); const auto r_rf = B.take<uint8_t>(cull ? nq : 0);
  const auto r_ck = B.take<int32_t>(cap_conn), r_cw = B.take<int32_t>(cap_conn), r_rk = B.take<int32_t>(cap_ord), r_rw = B.take<int32_t>(cap_ord);
  const size_t out_bytes = B.size - out_off;
  const auto t_cc = B.take<int32_t>(conn ? nq : 0), t_co = B.take<int32_t>(conn ? nq : 0);
  const auto t_sl = B.take<int32_t>((size_t)stage_total), t_sc = B.take<int32_t>((size_t)stage_total), t_kf = B.take<int32_t>((size_t)stage_total),
             t_w = B.take<int32_t>((size_t)stage_total);
  const auto t_key = B.take<u64>((size_t)stage_total);
  int st;
  void* hb; st = lld_ctx_pinned(ctx, out_off + out_bytes, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind((char*)hb, (char*)db);
  B.stage(i_q, in->kf_slot);
  if (conn) B.stage(i_so, stage_off.data());

  CovArgs A;
  A.query = B.dev(i_q); A.stage_off = B.dev(i_so);
  A.n_queries = nq; A.monocular = in->monocular ? 1 : 0; A.th = in->params.th; A.th_obs = in->params.th_obs; A.has_ext = m->d_ext ? 1 : 0;
  A.flags = in->flags; A.ratio = in->params.redundant_ratio;
  A.st_slot = B.dev(t_sl); A.st_cnt = B.dev(t_sc); A.st_kf = B.dev(t_kf); A.st_w = B.dev(t_w); A.st_key = B.dev(t_key);
  A.cnt_conn = B.dev(t_cc); A.cnt_ord = B.dev(t_co);
  A.n_max = B.dev(r_nm); A.kf_max = B.dev(r_km); A.updated = B.dev(r_up); A.status = B.dev(r_st);
  A.n_mps = B.dev(r_mp); A.n_red = B.dev(r_rd); A.redundant = B.dev(r_rf);
  A.cap_conn = cap_conn; A.cap_ord = cap_ord;
  A.conn_start = B.dev(r_cs); A.ord_start = B.dev(r_rs); A.totals = B.dev(r_tot);
  A.conn_kf = B.dev(r_ck); A.conn_w = B.dev(r_cw); A.ord_kf = B.dev(r_rk); A.ord_w = B.dev(r_rw);

  if (conn && !m->cov_lds_set) {
    LLD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&map_covis_query_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCovLds));
    m->cov_lds_set = true;
  }
  hipStream_t sm = ctx->stream;
  struct Events {                                                      // destroyed on every way out
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Events() { for (int k = 0; k < 4; ++k) if (e[k]) (void)hipEventDestroy(e[k]); }
  } events;
  hipEvent_t* ev = events.e;
  const bool timed = L->phase_ms != nullptr;
  if (timed) for (int k = 0; k < 4; ++k) LLD_HIP_TRY(hipEventCreate(&ev[k]));
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[0], sm));
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, sm));
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[1], sm));
  hipLaunchKernelGGL(map_covis_query_kernel, dim3(nq), dim3(kCovThreads), conn ? kCovLds : 0, sm, m->D, m->X, A);
  if (conn) hipLaunchKernelGGL(map_covis_pack_kernel, dim3(nq), dim3(kCovThreads), 0, sm, A);
  LLD_HIP_TRY(hipGetLastError());
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[2], sm));
  LLD_HIP_TRY(hipMemcpyAsync(B.h + out_off, B.d + out_off, out_bytes, hipMemcpyDeviceToHost, sm));
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[3], sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  if (timed) {
    for (int k = 0; k < 3; ++k) LLD_HIP_TRY(hipEventElapsedTime(&L->phase_ms[k], ev[k], ev[k + 1]));
  }

  if (conn) {
    const int32_t* tot = B.host(r_tot);
    L->n_conn = tot[0]; L->n_ordered = tot[1];
    if (tot[0] > L->conn_capacity || tot[1] > L->ordered_capacity) return LLD_ERR_INVALID;
    std::memcpy(L->conn_start, B.host(r_cs), (size_t)(nq + 1) * 4); std::memcpy(L->ordered_start, B.host(r_rs), (size_t)(nq + 1) * 4);
    std::memcpy(L->n_max, B.host(r_nm), (size_t)nq * 4); std::memcpy(L->kf_max, B.host(r_km), (size_t)nq * 4); std::memcpy(L->updated, B.host(r_up), (size_t)nq);
    if (tot[0]) { std::memcpy(L->conn_kf, B.host(r_ck), (size_t)tot[0] * 4); std::memcpy(L->conn_weight, B.host(r_cw), (size_t)tot[0] * 4); }
    if (tot[1]) { std::memcpy(L->ordered_kf, B.host(r_rk), (size_t)tot[1] * 4); std::memcpy(L->ordered_weight, B.host(r_rw), (size_t)tot[1] * 4); }
  }
  if (cull) {
    std::memcpy(L->n_mps, B.host(r_mp), (size_t)nq * 4); std::memcpy(L->n_redundant, B.host(r_rd), (size_t)nq * 4); std::memcpy(L->redundant, B.host(r_rf), (size_t)nq);
  }
  std::memcpy(out->status, B.host(r_st), (size_t)nq);
  return LLD_OK;
}

}  // extern "C"
