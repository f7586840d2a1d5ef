// lld_map_tables.h — the resident map's tables as the files that run on them see them: the device pointers (MapDev, MapExt), the host's
// bookkeeping of the variable-length rows (RowPool) and the handle that owns both (struct lld_map).  lld_map.hip creates, fills and frees
// them; lld_map_covis.hip and lld_map_ba.hip walk them; lld_map_apply.hip changes rows on the device and makes the RowPools follow;
// lld_map_refresh.hip rewrites the landmarks' descriptor, normal and distance rows from them; lld_map_fuse.hip searches a keyframe's rows for
// duplicates of listed points and moves observation rows between the landmarks it fuses.  The grow-only staging pair each of these
// call families keeps on the handle is one struct (Staging); how a call travels through it is lld_round_trip.h's.
// lld_map_internal.h stays the narrow face lld_frame_track.hip sees.  Nothing here is exported.
#ifndef LLD_MAP_TABLES_H
#define LLD_MAP_TABLES_H

#include "lld_common.h"
#include "lld_upload_block.h"

namespace lld_map_dev {

using lld_track::Span;
using lld_track::UploadBlock;
typedef unsigned long long u64;

// The layout of a slot's rows is described at the top of lld_map.hip.
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

// The bundle-adjustment tables (lld_map_ba.hip).  All null until the first lld_map_set_keyframe_features / _poses / lld_map_set_line_observations.
//   keyframe slot s  k_id = mnId, k_qt[7] = the pose as SE3Quat, k_ow[3] = the camera centre of that pose (KeyFrame::SetPose, float),
//                    k_feat (1: features were set), k_uvr = (offset, length) in uvr_pool of the
//                    keypoints' (u, v, uR) float bits, three words per keypoint, k_kl = (offset, length) in kl_pool of the keylines, ten words
//                    each: left[4], right[4] float bits, octave[2]
//   line slot s      l_obs / l_idx = (offset, length) in lobs_pool / lidx_pool of mObservations: keyframe slot, keyline index; l_nobs =
//                    MapLine::Observations(), -1: no observation row was ever set
//   per call         k_mark (~0 unmarked, 0 local, 1 + (landmark ordinal << 32 | row position) of the first visit: fixed), k_cam = the
//                    keyframe's camera index in the window, fixed / fixed_bad = the non-bad / bad keyframes marked fixed, in no order
struct MapBa {
  u64* k_id; double* k_qt; float* k_ow; uint8_t* k_feat; int2* k_uvr; int2* k_kl; int32_t* uvr_pool; int32_t* kl_pool;
  int2* l_obs; int2* l_idx; int32_t* lobs_pool; int32_t* lidx_pool; int32_t* l_nobs;
  u64* k_mark; int32_t* k_cam; int32_t* fixed; int32_t* fixed_bad;
};

// The keyframes' descriptor rows (lld_map_refresh.hip reads them).  All null until the first lld_map_set_keyframe_descriptors /
// lld_map_set_keyframe_line_descriptors.
//   keyframe slot s  k_desc = (offset, length) in kdesc_pool of mDescriptors, eight words per keypoint; k_ldesc = (offset, length) in
//                    kldesc_pool of mDescriptorsLines, `dim` float bit patterns per keyline
struct MapDesc { int2* k_desc; int32_t* kdesc_pool; int2* k_ldesc; int32_t* kldesc_pool; };

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
  int launch(hipStream_t st, const UploadBlock& B, const PoolPlan& P) const;      // defined in lld_map.hip: it names map_rows_kernel
};

// A pinned block and a device block that a call family reuses from call to call and that only grow: a quarter and a page more than asked
// for, so a slowly growing map does not allocate on every call.
struct Staging {
  char* h = nullptr; size_t h_bytes = 0; char* d = nullptr; size_t d_bytes = 0;
  // LLD_ERR_ALLOC leaves the block that could not grow null.  `stream` is waited for before the device block is freed: the kernels of an
  // earlier call may still read it.
  int grow(hipStream_t stream, size_t pinned, size_t device) {
    if (pinned > h_bytes) {
      if (h) LLD_HIP_TRY(hipHostFree(h));
      h = nullptr; h_bytes = 0;
      const size_t want = pinned + (pinned >> 2) + 4096;
      if (hipHostMalloc(reinterpret_cast<void**>(&h), want, hipHostMallocDefault) != hipSuccess) { h = nullptr; return LLD_ERR_ALLOC; }
      h_bytes = want;
    }
    if (device > d_bytes) {
      LLD_HIP_TRY(hipStreamSynchronize(stream));
      if (d) LLD_HIP_TRY(hipFree(d));
      d = nullptr; d_bytes = 0;
      const size_t want = device + (device >> 2) + 4096;
      if (hipMalloc(reinterpret_cast<void**>(&d), want) != hipSuccess) { d = nullptr; return LLD_ERR_ALLOC; }
      d_bytes = want;
    }
    return LLD_OK;
  }
  void release() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    h = d = nullptr; h_bytes = d_bytes = 0;
  }
};

// slots in range and no slot twice in one call (stamp / epoch: lld_map::stamp_* and lld_map::epoch)
inline bool slots_ok(std::vector<uint32_t>& stamp, uint32_t& epoch, int n, const int32_t* slot) {
  if (++epoch == 0) { std::fill(stamp.begin(), stamp.end(), 0u); epoch = 1; }
  for (int i = 0; i < n; i++) {
    if (slot[i] < 0 || (size_t)slot[i] >= stamp.size() || stamp[slot[i]] == epoch) return false;
    stamp[slot[i]] = epoch;
  }
  return true;
}

// ComputeDistinctiveDescriptors of n point slots, queued on `sm` behind whatever changed their rows (lld_map_refresh.hip: rf_check_kernel,
// rf_point_wave, rf_point_block).  slot [n] and list [n] (the queries with a stored row of at most 64 first, n_wave of them) are device
// arrays the caller uploaded; the others are device scratch of n elements each.  A slot is named at most once.
struct DescRefresh { int32_t n, n_wave; const int32_t* slot; const int32_t* list; uint8_t* verdict; int32_t* t_ref; int32_t* t_level; int32_t* o_best; int32_t* o_med; uint8_t* o_upd; };

}  // namespace lld_map_dev

struct lld_map {
  lld_ctx* ctx = nullptr;
  lld_map_limits lim{};
  lld_map_dev::MapDev D{};
  char* d_tables = nullptr; size_t first_off = 0, first_bytes = 0, down_off = 0, down_bytes = 0, tables_bytes = 0;
  size_t o_lkf = 0, o_lpts = 0, o_llns = 0;                         // inside the downloaded span, which starts with st
  lld_map_dev::RowPool obs, child, kpt, kln;
  // the culling tables (MapExt): allocated by the first setter that fills them
  lld_map_dev::MapExt X{}; char* d_ext = nullptr; size_t ext_bytes = 0; lld_map_dev::RowPool idx, koct, kdep;
  // the bundle-adjustment tables (MapBa): allocated by the first setter that fills them; mark_off / mark_bytes: k_mark inside d_ba
  lld_map_dev::MapBa Y{}; char* d_ba = nullptr; size_t ba_bytes = 0, mark_off = 0, mark_bytes = 0; lld_map_dev::RowPool kuvr, kkl, lobs, lidx;
  std::vector<uint8_t> kf_feat;             // lld_map_set_keyframe_features named the slot since the last clear
  // lld_map_ba_window's staging; lld_map_local_ba's result arrays and the capacities of its last call
  lld_map_dev::Staging ba;
  std::vector<double> ba_res_f; std::vector<uint8_t> ba_res_b; int32_t ba_cap[6] = {0, 0, 0, 0, 0, 0};
  std::vector<uint8_t> kf_set;              // lld_map_set_keyframes named the slot since the last clear
  std::vector<unsigned long long> kf_key;   // ... and the order key it gave it (0: never set): where lld_map_fuse puts a new observation in a row
  // MapPoint::mpRefKF per point slot (lld_map_set_point_refs), -1 unknown: a pool of its own, allocated by the first call
  int32_t* d_ref = nullptr;
  // The window lld_map_ba_window / lld_map_local_ba assembled last, for lld_map_ba_apply: its index arrays are still in ba.h / ba.d at these
  // byte offsets.  valid: the status was 0 and every capacity held; at: `mutations` when it was assembled.  mutations counts every call that
  // changes a table: lld_map_set_*, lld_map_clear, LLD_MAP_COVIS_WRITE_COV, lld_map_ba_apply, lld_map_refresh_* and lld_map_fuse when they wrote.
  struct BaStaged {
    bool valid = false; unsigned long long at = 0;
    int32_t n_cams = 0, n_local = 0, n_pts = 0, n_ptobs = 0, n_lns = 0, n_lnobs = 0;
    size_t cam_slot = 0, point_slot = 0, pt_start = 0, pt_cam = 0, line_slot = 0, ln_start = 0, ln_cam = 0;
  } win;
  unsigned long long mutations = 0;
  lld_map_dev::Staging ap;                  // lld_map_ba_apply's staging
  // the keyframes' descriptor rows (MapDesc): allocated by the first setter that fills them; lld_map_refresh_*'s staging
  lld_map_dev::MapDesc Z{}; char* d_desc = nullptr; size_t desc_bytes = 0; lld_map_dev::RowPool kdesc, kldesc;
  lld_map_dev::Staging rf;
  lld_map_dev::Staging fu;                  // lld_map_fuse's staging
  bool cov_lds_set = false;                 // map_covis_query_kernel was granted its 64 KB of dynamic LDS
  std::vector<uint32_t> stamp_pt, stamp_kf, stamp_ln; uint32_t epoch = 0;
  // the staging of lld_map_set_*, the event of the last copy out of its pinned block
  lld_map_dev::Staging up; hipEvent_t uploaded = nullptr; bool upload_pending = false;
  char* h_down = nullptr;
  unsigned long long serial = 0;            // counts lld_frame_track_update_local_map calls: the lists in the tables are the last one's
  bool poisoned = false;                    // a HIP failure after the host bookkeeping of a set call moved: host copy and device tables may differ
  size_t lkf_lds = 0;
};

namespace lld_map_dev {
int refresh_descriptors_queue(hipStream_t sm, const lld_map* m, const DescRefresh& R);      // lld_map_refresh.hip
}

#endif
