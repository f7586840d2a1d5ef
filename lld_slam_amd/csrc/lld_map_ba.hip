// lld_map_ba.hip — the local bundle adjustment window assembled on the resident map's tables (lld_map.hip, lld_map_tables.h):
// lld_map_ba_window, which is the first third of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:938-1018 and the edge loops :1093-1218),
// and lld_map_local_ba, which hands that window to lld_local_ba_stopflag.
//
// The reference walks objects and stamps them (mnBALocalForKF, mnBAFixedForKF); here a stamp is a 64-bit key that records WHERE the walk would
// have met the object first, so that the order of the walk can be restored after a parallel visit:
//   ba_mark_kernel        k_mark = 0 for every slot of the list (local, bad ones included); listed = first entry or not bad
//   ba_first_kernel       one workgroup per listed keyframe: atomicMin of (list position, entry position) per point and line slot
//   ba_count_kernel       first occurrences per keyframe
//   ba_write_kernel       ordered compaction: the local points and lines, in list order and then keypoint order
//   ba_visit_kernel       sixteen lanes per landmark: non-bad observers counted, each index held to the observer's rows, and
//                         atomicMin of 1 + (landmark ordinal, row position) per observer - whoever finds the slot unmarked lists it as fixed
//   ba_local_cams_kernel  one workgroup: the listed local keyframes ranked by (mn_id, list position), the mn_id == 0 ones behind them
//   ba_fixed_rank_kernel  the fixed cameras ranked by their keys: first-marked order
//   ba_cams_kernel        a camera's feature rows held to its point and line rows; the pose goes out
//   ba_scan_kernel        the two *_obs_start arrays: tiles of 256, every tile sums the counts before it
//   ba_fill_kernel        sixteen lanes per landmark: a point's run in stored order, a line's run by ascending mn_id, widened
// A row's order inside a run is a rank by counting (how many kept entries come before this one), not a sort in LDS: rows are short, and no
// row length is a limit.  Nothing is written to the window unless the status is 0 and every count is inside its capacity; both are decided
// on the device before ba_fill_kernel, from row lengths alone.  Plain vector loads and stores only.  On the host the window is laid out on an
// UploadBlock in the map's staging pair (lld_map_tables.h's Staging) and travels through lld_round_trip.h; the downloaded range starts behind
// the scratch, at the header.
#include "lld_common.h"
#include "lld_map_tables.h"
#include "lld_round_trip.h"
#include "lld_wave.h"

namespace {

using lld_map_dev::MapBa;
using lld_map_dev::MapDev;
using lld_map_dev::MapExt;
using lld_map_dev::u64;
using lld_rt::copy_out;
using lld_track::Span;
using lld_track::UploadBlock;

constexpr int kMaxLocal = LLD_MAP_BA_MAX_LOCAL;        // ba_local_cams_kernel ranks them in one workgroup
constexpr int kThreads = 256;
constexpr int kScanTile = kThreads;                     // ba_scan_kernel: one entry per lane
constexpr int kGroup = 16, kGroups = kThreads / kGroup; // lanes per landmark in ba_visit_kernel / ba_fill_kernel
constexpr int kGrid = 512;                              // grid-stride kernels: the counts they run over are known on the device only
enum { H_NCAMS = 0, H_NFREE, H_NLOCAL, H_NPTS, H_NPTOBS, H_NLNS, H_NLNOBS, H_STATUS, H_NFIXED, H_NBAD, H_WORDS = 16 };

struct BaArgs {
  int32_t n, n_levels, has_ext, bound_p, bound_l;
  const int32_t* slot; const float* sig;
  int32_t* listed; int32_t* cnt_p; int32_t* cnt_l; int32_t* lp; int32_t* pcnt; int32_t* ll; int32_t* lcnt;
  int32_t* hdr;
  int32_t cap_c, cap_p, cap_po, cap_l, cap_lo, cap_b;
  int32_t* cam_slot; double* cam_qt; int32_t* bad_slot;
  int32_t* point_slot; double* pt_xyz; int32_t* pt_start; int32_t* pt_cam; double* pt_uvr; double* pt_sig;
  int32_t* line_slot; double* ln_x0; double* ln_dir; int32_t* ln_start; int32_t* ln_cam; double* ln_left; double* ln_right; int32_t* ln_oct;
};

__device__ __forceinline__ void no_data(const BaArgs& A) { atomicOr(&A.hdr[H_STATUS], LLD_MAP_BA_NO_FEATURE_DATA); }
__device__ __forceinline__ u64 first_key(int p, int j) { return ((u64)(unsigned)p << 32) | (unsigned)j; }

// ------------------------------------------------------------------------------------------------ :940-950 local keyframes
__global__ void ba_mark_kernel(MapDev M, MapBa Y, BaArgs A) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const int s = A.slot[i];
  Y.k_mark[s] = 0;                                                     // mnBALocalForKF, whatever the bad flag
  A.listed[i] = (i == 0 || !M.k_bad[s]) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ :955-984 local points and lines
// a line counts when it is not bad and has four observations; one that is not bad and has no observation row cannot be judged
__device__ __forceinline__ bool line_counts(const MapDev& M, const MapBa& Y, const BaArgs& A, int s, bool report) {
  if (s < 0 || M.l_bad[s]) return false;
  const int nobs = Y.l_nobs[s];
  if (nobs < 0) { if (report) no_data(A); return false; }
  return nobs >= 4;
}
__global__ __launch_bounds__(kThreads) void ba_first_kernel(MapDev M, MapBa Y, BaArgs A) {
  const int p = blockIdx.x;
  if (!A.listed[p]) return;
  const int kf = A.slot[p];
  const int2 rp = M.k_pt[kf], rl = M.k_ln[kf];
  for (int j = threadIdx.x; j < rp.y; j += kThreads) {
    const int s = M.kpt_pool[rp.x + j];
    if (s >= 0 && M.p_state[s] == 1) atomicMin(&M.p_first[s], first_key(p, j));
  }
  for (int j = threadIdx.x; j < rl.y; j += kThreads) {
    const int s = M.kln_pool[rl.x + j];
    if (line_counts(M, Y, A, s, true)) atomicMin(&M.l_first[s], first_key(p, j));
  }
}
__global__ __launch_bounds__(kThreads) void ba_count_kernel(MapDev M, MapBa Y, BaArgs A) {
  __shared__ int lds[kThreads / 64];
  const int p = blockIdx.x;
  int np = 0, nl = 0;
  if (A.listed[p]) {                                                   // (uniform over the workgroup)
    const int kf = A.slot[p];
    const int2 rp = M.k_pt[kf], rl = M.k_ln[kf];
    for (int j = threadIdx.x; j < rp.y; j += kThreads) {
      const int s = M.kpt_pool[rp.x + j];
      if (s >= 0 && M.p_state[s] == 1 && M.p_first[s] == first_key(p, j)) np++;
    }
    for (int j = threadIdx.x; j < rl.y; j += kThreads) {
      const int s = M.kln_pool[rl.x + j];
      if (line_counts(M, Y, A, s, false) && M.l_first[s] == first_key(p, j)) nl++;
    }
  }
  np = lld_wave::block_sum(np, lds); nl = lld_wave::block_sum(nl, lds);
  if (threadIdx.x == 0) { A.cnt_p[p] = np; A.cnt_l[p] = nl; }
}
// every workgroup sums the counts of the keyframes before its own, then writes its keyframe's first occurrences in entry order
__global__ __launch_bounds__(kThreads) void ba_write_kernel(MapDev M, MapBa Y, BaArgs A) {
  __shared__ int lds[kThreads / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  int a = 0, b = 0, ta = 0, tb = 0;
  for (int q = tid; q < A.n; q += kThreads) { const int c = A.cnt_p[q], d = A.cnt_l[q]; ta += c; tb += d; if (q < p) { a += c; b += d; } }
  a = lld_wave::block_sum(a, lds); b = lld_wave::block_sum(b, lds); ta = lld_wave::block_sum(ta, lds); tb = lld_wave::block_sum(tb, lds);
  if (p == 0 && tid == 0) { A.hdr[H_NPTS] = ta; A.hdr[H_NLNS] = tb; }
  if (!A.listed[p] || ta > A.bound_p || tb > A.bound_l) return;        // (the bounds hold by construction: a slot is listed once)
  const int kf = A.slot[p];
  const int2 rp = M.k_pt[kf], rl = M.k_ln[kf];
  for (int j0 = 0, run = a; j0 < rp.y; j0 += kThreads) {
    const int j = j0 + tid;
    int s = -1; bool w = false;
    if (j < rp.y) { s = M.kpt_pool[rp.x + j]; w = s >= 0 && M.p_state[s] == 1 && M.p_first[s] == first_key(p, j); }
    int tot; const int r = lld_wave::block_excl_scan<kThreads>(w ? 1 : 0, lds, tot);
    if (w) A.lp[run + r] = s;
    run += tot;
  }
  for (int j0 = 0, run = b; j0 < rl.y; j0 += kThreads) {
    const int j = j0 + tid;
    int s = -1; bool w = false;
    if (j < rl.y) { s = M.kln_pool[rl.x + j]; w = line_counts(M, Y, A, s, false) && M.l_first[s] == first_key(p, j); }
    int tot; const int r = lld_wave::block_excl_scan<kThreads>(w ? 1 : 0, lds, tot);
    if (w) A.ll[run + r] = s;
    run += tot;
  }
}

// ------------------------------------------------------------------------------------------------ :990-1018 fixed cameras, and the runs' lengths
// Landmark ordinal q: the local points, then the local lines.  A bad observer is marked like any other (mnBAFixedForKF) but neither listed
// as fixed nor part of a run: it goes to a list of its own, in no order, for a caller that mirrors the marks.  Of the others the stored
// index is held to the rows the fill will read - before anything of those rows is read.
__device__ __forceinline__ void visit(const MapBa& Y, const BaArgs& A, int kf, bool bad, int q, int j) {
  const u64 old = atomicMin(&Y.k_mark[kf], 1ull + first_key(q, j));
  if (old != ~0ull) return;                                            // (only the one visit that found it unmarked goes on)
  if (bad) Y.fixed_bad[atomicAdd(&A.hdr[H_NBAD], 1)] = kf;
  else Y.fixed[atomicAdd(&A.hdr[H_NFIXED], 1)] = kf;
}
__global__ __launch_bounds__(kThreads) void ba_visit_kernel(MapDev M, MapExt X, MapBa Y, BaArgs A) {
  const int np = A.hdr[H_NPTS], nl = A.hdr[H_NLNS], total = np + nl;
  const int g = threadIdx.x / kGroup, gl = threadIdx.x % kGroup;
  for (int base = blockIdx.x * kGroups; base < total; base += gridDim.x * kGroups) {      // uniform over the workgroup: the shuffles below are safe
    const int q = base + g;
    int c = 0;
    if (q < np) {
      const int s = A.lp[q];
      const int2 row = M.p_obs[s];
      int2 ir = make_int2(0, 0);
      if (A.has_ext) ir = X.p_idx[s];
      if (ir.y != row.y) { if (gl == 0) no_data(A); }                  // the row came through lld_map_set_observations: no indices
      else
        for (int j = gl; j < row.y; j += kGroup) {
          const int kf = M.obs_pool[row.x + j];
          const bool bad = M.k_bad[kf] != 0;
          visit(Y, A, kf, bad, q, j);
          if (bad) continue;
          c++;
          const int idx = X.idx_pool[ir.x + j];
          const int2 orow = X.k_oct[kf];
          if (idx < 0 || idx >= orow.y || idx >= M.k_pt[kf].y) no_data(A);
          else { const int oct = X.oct_pool[orow.x + idx]; if (oct < 0 || oct >= A.n_levels) no_data(A); }
        }
    } else if (q < total) {
      const int s = A.ll[q - np];
      const int2 row = Y.l_obs[s], ir = Y.l_idx[s];
      if (ir.y != row.y) { if (gl == 0) no_data(A); }
      else
        for (int j = gl; j < row.y; j += kGroup) {
          const int kf = Y.lobs_pool[row.x + j];
          const bool bad = M.k_bad[kf] != 0;
          visit(Y, A, kf, bad, q, j);
          if (bad) continue;
          c++;
          const int idx = Y.lidx_pool[ir.x + j];
          if (idx < 0 || idx >= M.k_ln[kf].y) no_data(A);
        }
    }
    c = lld_wave::sum<kGroup>(c);
    if (gl == 0 && q < np) A.pcnt[q] = c;
    if (gl == 0 && q >= np && q < total) A.lcnt[q - np] = c;
  }
}

// ------------------------------------------------------------------------------------------------ the cameras (lld_optimizer_adapter.cc:83-87)
__global__ __launch_bounds__(kMaxLocal) void ba_local_cams_kernel(MapBa Y, BaArgs A) {
  __shared__ u64 s_id[kMaxLocal];
  __shared__ uint8_t s_on[kMaxLocal];
  const int i = threadIdx.x;
  int s = -1; bool on = false; u64 id = 0;
  if (i < A.n) { s = A.slot[i]; on = A.listed[i] != 0; if (on && Y.k_feat[s]) id = Y.k_id[s]; }    // (without features the status says so: ba_cams_kernel)
  s_id[i] = id; s_on[i] = on ? 1 : 0;
  __syncthreads();
  int rank = 0, n_free = 0, zero_before = 0, n_zero = 0;
  for (int j = 0; j < A.n; j++) {
    if (!s_on[j]) continue;
    const u64 o = s_id[j];
    if (o) { n_free++; if (o < id || (o == id && j < i)) rank++; }
    else { n_zero++; if (j < i) zero_before++; }
  }
  if (on) {
    const int cam = id ? rank : n_free + zero_before;
    Y.k_cam[s] = cam;
    if (cam < A.cap_c) A.cam_slot[cam] = s;
  }
  if (i == 0) { A.hdr[H_NFREE] = n_free; A.hdr[H_NLOCAL] = n_free + n_zero; }
}
__global__ __launch_bounds__(kThreads) void ba_fixed_rank_kernel(MapBa Y, BaArgs A) {
  const int nf = A.hdr[H_NFIXED], nloc = A.hdr[H_NLOCAL];
  if (blockIdx.x == 0 && threadIdx.x == 0) A.hdr[H_NCAMS] = nloc + nf;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < nf; i += gridDim.x * kThreads) {
    const int kf = Y.fixed[i];
    const u64 key = Y.k_mark[kf];
    int r = 0;
    for (int j = 0; j < nf; j++) r += Y.k_mark[Y.fixed[j]] < key;      // the keys are distinct: one (landmark, position) each
    const int cam = nloc + r;
    Y.k_cam[kf] = cam;
    if (cam < A.cap_c) A.cam_slot[cam] = kf;
  }
}
__global__ __launch_bounds__(kThreads) void ba_cams_kernel(MapDev M, MapExt X, MapBa Y, BaArgs A) {
  const int nc = min(A.hdr[H_NCAMS], A.cap_c);                         // (a short capacity is refused on the host whatever this finds)
  const int nb = A.hdr[H_NBAD] <= A.cap_b ? A.hdr[H_NBAD] : 0;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < nb; i += gridDim.x * kThreads) A.bad_slot[i] = Y.fixed_bad[i];
  for (int c = blockIdx.x * kThreads + threadIdx.x; c < nc; c += gridDim.x * kThreads) {
    const int s = A.cam_slot[c];
    const int np = M.k_pt[s].y, nl = M.k_ln[s].y;
    if (!Y.k_feat[s] || Y.k_uvr[s].y != 3 * np || Y.k_kl[s].y != 10 * nl || !A.has_ext || X.k_oct[s].y != np) { no_data(A); continue; }
    for (int k = 0; k < 7; k++) A.cam_qt[7 * (size_t)c + k] = Y.k_qt[7 * (size_t)s + k];
  }
}

// ------------------------------------------------------------------------------------------------ the runs' starts
// Exclusive scan of cnt[0, n) into start[0, n]: entry n counts as 0, so start[n] is the total, which also goes to *total.  Only entries
// inside the capacity are stored.
__device__ void scan_starts(const int32_t* cnt, int n, int32_t* start, int cap, int32_t* total, int* lds) {
  const int tid = threadIdx.x;
  for (int tile = blockIdx.x; tile * kScanTile <= n; tile += gridDim.x) {
    const int lo = tile * kScanTile;
    int before = 0;
    for (int q = tid; q < lo; q += kThreads) before += cnt[q];
    before = lld_wave::block_sum(before, lds);
    const int i = lo + tid;
    int tot; const int r = lld_wave::block_excl_scan<kThreads>(i < n ? cnt[i] : 0, lds, tot);
    if (i <= n && i <= cap) start[i] = before + r;
    if (i == n) *total = before + r;
  }
}
__global__ __launch_bounds__(kThreads) void ba_scan_kernel(BaArgs A) {
  __shared__ int lds[kThreads / 64];
  scan_starts(A.pcnt, A.hdr[H_NPTS], A.pt_start, A.cap_p, &A.hdr[H_NPTOBS], lds);
  scan_starts(A.lcnt, A.hdr[H_NLNS], A.ln_start, A.cap_l, &A.hdr[H_NLNOBS], lds);
}

// ------------------------------------------------------------------------------------------------ :1093-1218 the window
__device__ __forceinline__ double wide(int32_t bits) { return (double)__int_as_float(bits); }
__global__ __launch_bounds__(kThreads) void ba_fill_kernel(MapDev M, MapExt X, MapBa Y, BaArgs A) {
  const int* h = A.hdr;
  const int np = h[H_NPTS], nl = h[H_NLNS];
  if (h[H_STATUS] || h[H_NCAMS] > A.cap_c || np > A.cap_p || h[H_NPTOBS] > A.cap_po || nl > A.cap_l || h[H_NLNOBS] > A.cap_lo) return;
  const int total = np + nl;
  const int g = threadIdx.x / kGroup, gl = threadIdx.x % kGroup;
  for (int q = blockIdx.x * kGroups + g; q < total; q += gridDim.x * kGroups) {
    if (q < np) {
      const int s = A.lp[q];
      if (gl == 0) A.point_slot[q] = s;
      if (gl < 3) A.pt_xyz[3 * (size_t)q + gl] = (double)M.p_pos[3 * (size_t)s + gl];
      const int2 row = M.p_obs[s];
      const int to_idx = X.p_idx[s].x - row.x;
      const size_t base = (size_t)A.pt_start[q];
      for (int j = gl; j < row.y; j += kGroup) {
        const int kf = M.obs_pool[row.x + j];
        if (M.k_bad[kf]) continue;
        int r = 0;
        for (int k = 0; k < j; k++) r += M.k_bad[M.obs_pool[row.x + k]] == 0;          // stored order
        const int idx = X.idx_pool[row.x + j + to_idx];
        const int32_t* f = Y.uvr_pool + Y.k_uvr[kf].x + 3 * (size_t)idx;
        const size_t e = base + r;
        A.pt_cam[e] = Y.k_cam[kf];
        A.pt_uvr[3 * e] = wide(f[0]); A.pt_uvr[3 * e + 1] = wide(f[1]); A.pt_uvr[3 * e + 2] = wide(f[2]);
        A.pt_sig[e] = (double)A.sig[X.oct_pool[X.k_oct[kf].x + idx]];
      }
    } else {
      const int l = q - np, s = A.ll[l];
      if (gl == 0) A.line_slot[l] = s;
      if (gl < 3) { A.ln_x0[3 * (size_t)l + gl] = M.l_x0[3 * (size_t)s + gl]; A.ln_dir[3 * (size_t)l + gl] = M.l_dir[3 * (size_t)s + gl]; }
      const int2 row = Y.l_obs[s];
      const int to_idx = Y.l_idx[s].x - row.x;
      const size_t base = (size_t)A.ln_start[l];
      for (int j = gl; j < row.y; j += kGroup) {
        const int kf = Y.lobs_pool[row.x + j];
        if (M.k_bad[kf]) continue;
        const u64 id = Y.k_id[kf];
        int r = 0;
        for (int k = 0; k < row.y; k++) {                              // proj_map is keyed by mnId
          const int ko = Y.lobs_pool[row.x + k];
          if (M.k_bad[ko]) continue;
          const u64 o = Y.k_id[ko];
          r += o < id || (o == id && k < j);
        }
        const int idx = Y.lidx_pool[row.x + j + to_idx];
        const int32_t* f = Y.kl_pool + Y.k_kl[kf].x + 10 * (size_t)idx;
        const size_t e = base + r;
        A.ln_cam[e] = Y.k_cam[kf];
        for (int k = 0; k < 4; k++) { A.ln_left[4 * e + k] = wide(f[k]); A.ln_right[4 * e + k] = wide(f[4 + k]); }
        A.ln_oct[2 * e] = f[8]; A.ln_oct[2 * e + 1] = f[9];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
struct Layout {                                  // the downloaded span of one call, in the map's pinned block
  Span<int32_t> hdr, cam_slot, bad_slot, point_slot, pt_start, pt_cam, line_slot, ln_start, ln_cam, ln_oct;
  Span<double> cam_qt, pt_xyz, pt_uvr, pt_sig, ln_x0, ln_dir, ln_left, ln_right;
};

int check_in(const lld_map* m, const lld_map_ba_in* in) {
  if (!m || !in) return LLD_ERR_INVALID;
  if (in->n_keyframes < 1 || in->n_keyframes > kMaxLocal || !in->kf_slot || in->n_levels < 1 || !in->inv_level_sigma2) return LLD_ERR_INVALID;
  return LLD_OK;
}

// The assembly into the map's pinned block: B and L describe where.  cap: cameras, points, point observations, lines, line observations,
// keyframes marked fixed although they are bad.
// LLD_OK also when the status is set or a capacity was short: the header says which.
int run_window(lld_map* m, const lld_map_ba_in* in, const int32_t* cap, UploadBlock& B, Layout& L, float* phase_ms) {
  if (m->poisoned) return LLD_ERR_HIP;
  const int n = in->n_keyframes;
  if (++m->epoch == 0) { std::fill(m->stamp_kf.begin(), m->stamp_kf.end(), 0u); m->epoch = 1; }
  for (int i = 0; i < n; i++) {
    const int s = in->kf_slot[i];
    if (s < 0 || s >= m->lim.max_keyframes || !m->kf_set[s] || m->stamp_kf[s] == m->epoch) return LLD_ERR_INVALID;
    m->stamp_kf[s] = m->epoch;
  }
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  // what the lists can hold at most: every entry of the listed keyframes' rows (the host's rows are the device's: every update before this
  // call is queued before its kernels)
  long long bp = 0, bl = 0;
  for (int i = 0; i < n; i++) { bp += m->kpt.len[in->kf_slot[i]]; bl += m->kln.len[in->kf_slot[i]]; }
  const int bound_p = (int)std::min<long long>(bp, m->lim.max_points), bound_l = (int)std::min<long long>(bl, m->lim.max_lines);
  const size_t cc = cap[0], cp = cap[1], cpo = cap[2], cl = cap[3], clo = cap[4], cb = cap[5];

  B = UploadBlock();
  const auto i_slot = B.take<int32_t>(n); const auto i_sig = B.take<float>(in->n_levels);
  B.end_upload();
  const auto t_listed = B.take<int32_t>(n), t_cp = B.take<int32_t>(n), t_cl = B.take<int32_t>(n);
  const auto t_lp = B.take<int32_t>(bound_p), t_pc = B.take<int32_t>(bound_p), t_ll = B.take<int32_t>(bound_l), t_lc = B.take<int32_t>(bound_l);
  const size_t out_off = B.size;
  L.hdr = B.take<int32_t>(H_WORDS);
  L.cam_slot = B.take<int32_t>(cc); L.cam_qt = B.take<double>(cc, 7); L.bad_slot = B.take<int32_t>(cb);
  L.point_slot = B.take<int32_t>(cp); L.pt_xyz = B.take<double>(cp, 3); L.pt_start = B.take<int32_t>(cp + 1);
  L.pt_cam = B.take<int32_t>(cpo); L.pt_uvr = B.take<double>(cpo, 3); L.pt_sig = B.take<double>(cpo);
  L.line_slot = B.take<int32_t>(cl); L.ln_x0 = B.take<double>(cl, 3); L.ln_dir = B.take<double>(cl, 3); L.ln_start = B.take<int32_t>(cl + 1);
  L.ln_cam = B.take<int32_t>(clo); L.ln_left = B.take<double>(clo, 4); L.ln_right = B.take<double>(clo, 4); L.ln_oct = B.take<int32_t>(clo, 2);
  m->win.valid = false;                                                // the staging is about to be overwritten
  int st = m->ba.grow(ctx->stream, B.size, B.size); if (st) return st;
  B.bind(m->ba.h, m->ba.d);
  B.stage(i_slot, in->kf_slot); B.stage(i_sig, in->inv_level_sigma2);
  std::memset(B.host(L.hdr), 0, H_WORDS * 4);

  BaArgs A{};
  A.n = n; A.n_levels = in->n_levels; A.has_ext = m->d_ext ? 1 : 0; A.bound_p = bound_p; A.bound_l = bound_l;
  A.slot = B.dev(i_slot); A.sig = B.dev(i_sig);
  A.listed = B.dev(t_listed); A.cnt_p = B.dev(t_cp); A.cnt_l = B.dev(t_cl); A.lp = B.dev(t_lp); A.pcnt = B.dev(t_pc); A.ll = B.dev(t_ll); A.lcnt = B.dev(t_lc);
  A.hdr = B.dev(L.hdr);
  A.cap_c = cap[0]; A.cap_p = cap[1]; A.cap_po = cap[2]; A.cap_l = cap[3]; A.cap_lo = cap[4]; A.cap_b = cap[5];
  A.cam_slot = B.dev(L.cam_slot); A.cam_qt = B.dev(L.cam_qt); A.bad_slot = B.dev(L.bad_slot);
  A.point_slot = B.dev(L.point_slot); A.pt_xyz = B.dev(L.pt_xyz); A.pt_start = B.dev(L.pt_start); A.pt_cam = B.dev(L.pt_cam); A.pt_uvr = B.dev(L.pt_uvr); A.pt_sig = B.dev(L.pt_sig);
  A.line_slot = B.dev(L.line_slot); A.ln_x0 = B.dev(L.ln_x0); A.ln_dir = B.dev(L.ln_dir); A.ln_start = B.dev(L.ln_start); A.ln_cam = B.dev(L.ln_cam);
  A.ln_left = B.dev(L.ln_left); A.ln_right = B.dev(L.ln_right); A.ln_oct = B.dev(L.ln_oct);

  return lld_rt::round_trip(ctx->stream, B, out_off, B.size - out_off, phase_ms, [&](hipStream_t sm) {
    const MapDev& M = m->D;
    LLD_HIP_TRY(hipMemsetAsync(B.dev(L.hdr), 0, H_WORDS * 4, sm));
    LLD_HIP_TRY(hipMemsetAsync(m->d_tables + m->first_off, 0xff, m->first_bytes, sm));       // p_first / l_first: scratch of a call, as in UpdateLocalMap
    LLD_HIP_TRY(hipMemsetAsync(m->d_ba + m->mark_off, 0xff, m->mark_bytes, sm));
    hipLaunchKernelGGL(ba_mark_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, sm, M, m->Y, A);
    hipLaunchKernelGGL(ba_first_kernel, dim3(n), dim3(kThreads), 0, sm, M, m->Y, A);
    hipLaunchKernelGGL(ba_count_kernel, dim3(n), dim3(kThreads), 0, sm, M, m->Y, A);
    hipLaunchKernelGGL(ba_write_kernel, dim3(n), dim3(kThreads), 0, sm, M, m->Y, A);
    hipLaunchKernelGGL(ba_visit_kernel, dim3(kGrid), dim3(kThreads), 0, sm, M, m->X, m->Y, A);
    hipLaunchKernelGGL(ba_local_cams_kernel, dim3(1), dim3(kMaxLocal), 0, sm, m->Y, A);
    hipLaunchKernelGGL(ba_fixed_rank_kernel, dim3(kGrid), dim3(kThreads), 0, sm, m->Y, A);
    hipLaunchKernelGGL(ba_cams_kernel, dim3(kGrid), dim3(kThreads), 0, sm, M, m->X, m->Y, A);
    hipLaunchKernelGGL(ba_scan_kernel, dim3(kGrid), dim3(kThreads), 0, sm, A);
    hipLaunchKernelGGL(ba_fill_kernel, dim3(kGrid), dim3(kThreads), 0, sm, M, m->X, m->Y, A);
    return LLD_OK;
  });
}

bool fits(const int32_t* h, const int32_t* cap, bool with_bad = false) {
  return h[H_NCAMS] <= cap[0] && h[H_NPTS] <= cap[1] && h[H_NPTOBS] <= cap[2] && h[H_NLNS] <= cap[3] && h[H_NLNOBS] <= cap[4] && (!with_bad || h[H_NBAD] <= cap[5]);
}

// A complete window (status 0, every capacity held) stays in the staging: lld_map_ba_apply scatters a result through its index arrays.
void keep_for_apply(lld_map* m, const Layout& L, const int32_t* h) {
  lld_map::BaStaged& W = m->win;
  W.valid = true; W.at = m->mutations;
  W.n_cams = h[H_NCAMS]; W.n_local = h[H_NLOCAL]; W.n_pts = h[H_NPTS]; W.n_ptobs = h[H_NPTOBS]; W.n_lns = h[H_NLNS]; W.n_lnobs = h[H_NLNOBS];
  W.cam_slot = L.cam_slot.off; W.point_slot = L.point_slot.off; W.pt_start = L.pt_start.off; W.pt_cam = L.pt_cam.off;
  W.line_slot = L.line_slot.off; W.ln_start = L.ln_start.off; W.ln_cam = L.ln_cam.off;
}

}  // namespace

extern "C" {

int lld_map_ba_window(lld_map* m, const lld_map_ba_in* in, lld_map_ba_window_out* out) {
  if (!out) return LLD_ERR_INVALID;
  int st = check_in(m, in); if (st) return st;
  const int32_t cap[6] = {out->cam_capacity, out->point_capacity, out->pt_obs_capacity, out->line_capacity, out->ln_obs_capacity, 0};
  for (int k = 0; k < 5; k++) if (cap[k] < 0) return LLD_ERR_INVALID;
  if ((cap[0] > 0 && (!out->cam_slot || !out->cam_qt)) || (cap[1] > 0 && (!out->point_slot || !out->pt_xyz)) || !out->pt_obs_start ||
      (cap[2] > 0 && (!out->pt_obs_cam || !out->pt_obs_uvr || !out->pt_obs_inv_sigma2)) || (cap[3] > 0 && (!out->line_slot || !out->line_x0 || !out->line_dir)) ||
      !out->ln_obs_start || (cap[4] > 0 && (!out->ln_obs_cam || !out->ln_obs_left || !out->ln_obs_right || !out->ln_obs_octave))) return LLD_ERR_INVALID;
  if (!m->d_ba) {                                                     // no feature was ever set: nothing is queued
    if (m->poisoned) return LLD_ERR_HIP;
    for (int i = 0; i < in->n_keyframes; i++) {
      const int s = in->kf_slot[i];
      if (s < 0 || s >= m->lim.max_keyframes || !m->kf_set[s]) return LLD_ERR_INVALID;
      for (int k = 0; k < i; k++) if (in->kf_slot[k] == s) return LLD_ERR_INVALID;
    }
    out->n_cams = out->n_free_cams = out->n_local_cams = out->n_points = out->n_pt_obs = out->n_lines = out->n_ln_obs = 0;
    out->status = LLD_MAP_BA_NO_FEATURE_DATA;
    return LLD_OK;
  }
  UploadBlock B; Layout L;
  st = run_window(m, in, cap, B, L, out->phase_ms); if (st) return st;
  const int32_t* h = B.host(L.hdr);
  out->status = h[H_STATUS];
  if (out->status) {
    out->n_cams = out->n_free_cams = out->n_local_cams = out->n_points = out->n_pt_obs = out->n_lines = out->n_ln_obs = 0;
    return LLD_OK;
  }
  out->n_cams = h[H_NCAMS]; out->n_free_cams = h[H_NFREE]; out->n_local_cams = h[H_NLOCAL]; out->n_points = h[H_NPTS]; out->n_pt_obs = h[H_NPTOBS];
  out->n_lines = h[H_NLNS]; out->n_ln_obs = h[H_NLNOBS];
  if (!fits(h, cap)) return LLD_ERR_INVALID;                           // only the counts are written
  keep_for_apply(m, L, h);
  const size_t nc = h[H_NCAMS], np = h[H_NPTS], npo = h[H_NPTOBS], nl = h[H_NLNS], nlo = h[H_NLNOBS];
  copy_out(out->cam_slot, B, L.cam_slot, nc); copy_out(out->cam_qt, B, L.cam_qt, 7 * nc);
  copy_out(out->point_slot, B, L.point_slot, np); copy_out(out->pt_xyz, B, L.pt_xyz, 3 * np); copy_out(out->pt_obs_start, B, L.pt_start, np + 1);
  copy_out(out->pt_obs_cam, B, L.pt_cam, npo); copy_out(out->pt_obs_uvr, B, L.pt_uvr, 3 * npo); copy_out(out->pt_obs_inv_sigma2, B, L.pt_sig, npo);
  copy_out(out->line_slot, B, L.line_slot, nl); copy_out(out->line_x0, B, L.ln_x0, 3 * nl); copy_out(out->line_dir, B, L.ln_dir, 3 * nl);
  copy_out(out->ln_obs_start, B, L.ln_start, nl + 1);
  copy_out(out->ln_obs_cam, B, L.ln_cam, nlo); copy_out(out->ln_obs_left, B, L.ln_left, 4 * nlo); copy_out(out->ln_obs_right, B, L.ln_right, 4 * nlo);
  copy_out(out->ln_obs_octave, B, L.ln_oct, 2 * nlo);
  return LLD_OK;
}

int lld_map_local_ba(lld_map* m, const lld_map_ba_in* in, const lld_ba_params* params, volatile const unsigned char* stop_flag, lld_ba_result* result,
                     lld_map_ba_ids* ids) {
  if (!result || !ids) return LLD_ERR_INVALID;
  int st = check_in(m, in); if (st) return st;
  *ids = lld_map_ba_ids{};
  *result = lld_ba_result{};
  if (!m->d_ba) {
    lld_map_ba_window_out none{};
    int32_t zero[2] = {0, 0};
    none.pt_obs_start = zero; none.ln_obs_start = zero + 1;
    st = lld_map_ba_window(m, in, &none);
    ids->status = none.status;
    return st;
  }
  UploadBlock B; Layout L;
  const int32_t* h = nullptr;
  for (int attempt = 0; attempt < 2; attempt++) {                      // the capacities of the last call; a window that outgrew them is assembled again
    st = run_window(m, in, m->ba_cap, B, L, nullptr); if (st) return st;
    h = B.host(L.hdr);
    if (h[H_STATUS]) { ids->status = h[H_STATUS]; return LLD_OK; }
    if (fits(h, m->ba_cap, true)) break;
    if (attempt) return LLD_ERR_HIP;                                   // the counts moved between two runs on the same tables: never with a sound map
    const int32_t need[6] = {h[H_NCAMS], h[H_NPTS], h[H_NPTOBS], h[H_NLNS], h[H_NLNOBS], h[H_NBAD]};
    for (int k = 0; k < 6; k++) if (need[k] > m->ba_cap[k]) m->ba_cap[k] = need[k] + need[k] / 4 + 16;
  }
  keep_for_apply(m, L, h);
  lld_ba_window& w = ids->window;
  w.cam = in->cam;
  w.n_cams = h[H_NCAMS]; w.n_free_cams = h[H_NFREE]; w.cam_qt = B.host(L.cam_qt);
  w.n_points = h[H_NPTS]; w.pt_xyz = B.host(L.pt_xyz); w.pt_obs_start = B.host(L.pt_start); w.n_pt_obs = h[H_NPTOBS];
  w.pt_obs_cam = B.host(L.pt_cam); w.pt_obs_uvr = B.host(L.pt_uvr); w.pt_obs_inv_sigma2 = B.host(L.pt_sig);
  w.n_lines = h[H_NLNS]; w.line_x0 = B.host(L.ln_x0); w.line_dir = B.host(L.ln_dir); w.ln_obs_start = B.host(L.ln_start); w.n_ln_obs = h[H_NLNOBS];
  w.ln_obs_cam = B.host(L.ln_cam); w.ln_obs_left = B.host(L.ln_left); w.ln_obs_right = B.host(L.ln_right); w.ln_obs_octave = B.host(L.ln_oct);
  ids->n_local_cams = h[H_NLOCAL]; ids->cam_slot = B.host(L.cam_slot); ids->point_slot = B.host(L.point_slot); ids->line_slot = B.host(L.line_slot);
  ids->n_marked_bad = h[H_NBAD]; ids->marked_bad_slot = B.host(L.bad_slot);
  const size_t nc = w.n_cams, np = w.n_points, nl = w.n_lines;
  m->ba_res_f.assign(7 * nc + 3 * np + 6 * nl + 1, 0.0);
  m->ba_res_b.assign((size_t)w.n_pt_obs + 2 * (size_t)w.n_ln_obs + nl + 1, 0);
  result->cam_qt = m->ba_res_f.data(); result->pt_xyz = result->cam_qt + 7 * nc; result->line_x0 = result->pt_xyz + 3 * np; result->line_dir = result->line_x0 + 3 * nl;
  result->pt_obs_outlier = m->ba_res_b.data(); result->ln_edge_outlier = result->pt_obs_outlier + w.n_pt_obs; result->line_removed = result->ln_edge_outlier + 2 * (size_t)w.n_ln_obs;
  lld_ba_params def;
  if (!params) { lld_ba_params_default(&def); params = &def; }
  return lld_local_ba_stopflag(m->ctx, &w, params, stop_flag, result);
}

}  // extern "C"
