// lld_map_apply.hip — the last third of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1334-1386, the part under mMutexMapUpdate) on the
// resident map's tables: lld_map_ba_apply scatters a local BA's result through the index arrays of the window the map assembled last
// (lld_map_ba.hip left them in the map's device staging), and lld_map_download_rows reads any row pool back for an audit.
//
// The rules (erase lists, bad cascades, mpRefKF, UpdateNormalAndDepth, the MapLine::SetBadFlag quirk) are stated in include/lld_amd.h.
// Every point and every line of the window is independent of every other: what two landmarks can both write is a -1 into an observer's
// row, and every such write stores the same value.
//   ap_cams_kernel     one lane per local camera: the stored pose and its centre into k_qt / k_ow
//   ap_mark_kernel     sixteen lanes per window point: which stored entries the result erases (era: 0 kept, 1 a mono erasure, 2 a stereo
//                      one), the -1 writes into the observers' point rows, and by one lane the walk of n_obs in the reference's order
//   ap_lines_kernel    one lane per window line: its erasures one after the other (their order decides which entries a line that goes
//                      bad still clears), the minimal position, and the line's outputs
//   ap_refresh_kernel  sixteen lanes per window point: mpRefKF, the position, UpdateNormalAndDepth on the entries that stay - each lane
//                      forms terms, every lane adds them in row order; the sum and the level lookup are lld_normal_depth.h's
//   ap_rows_kernel     one lane per window point: the kept entries moved to the front of both rows (or both rows emptied), then the
//                      point's outputs read back from the tables
// The kernels follow each other on the stream, so none reads a row while another kernel rewrites it.  No index is followed before it is
// held to the row it points into.  The host then repeats the removals on its copies of the rows (RowPool), from the flags it sent and the
// verdicts it got back, and holds the lengths it arrives at to the device's.  The staging pair is lld_map_tables.h's Staging, the timed
// upload / launches / download lld_round_trip.h's.
#pragma clang fp contract(off)

#include "lld_common.h"
#include "lld_device_math.h"
#include "lld_map_tables.h"
#include "lld_normal_depth.h"
#include "lld_round_trip.h"
#include "lld_wave.h"

namespace {

using lld_map_dev::MapBa;
using lld_map_dev::MapDev;
using lld_map_dev::MapExt;
using lld_map_dev::RowPool;
using lld_rt::blocks;
using lld_rt::copy_out;
using lld_track::Span;
using lld_track::UploadBlock;

constexpr int kThreads = 256;
constexpr int kGroup = 16, kGroups = kThreads / kGroup;
enum { C_PT_ERASED = 0, C_LN_ERASED, C_PT_BAD, C_LN_BAD, C_SKIPPED, C_WORDS = 8 };
constexpr uint8_t kBad = LLD_MAP_APPLY_WENT_BAD, kRefreshed = LLD_MAP_APPLY_REFRESHED, kNoRef = LLD_MAP_APPLY_NO_REFERENCE, kSkipped = LLD_MAP_APPLY_INDEX_SKIPPED;
constexpr int32_t kMinusOneF = (int32_t)0xBF800000u;         // the bits of -1.0f: a keyline without a right partner stores it four times

struct ApArgs {
  int32_t n_local, n_pts, n_lns, n_levels, has_ext;
  // the window, in the staging lld_map_ba.hip filled
  const int32_t* cam_slot; const int32_t* point_slot; const int32_t* pt_start; const int32_t* pt_cam;
  const int32_t* line_slot; const int32_t* ln_start; const int32_t* ln_cam;
  // the result
  const double* cam_qt; const float* cam_ow; const float* pt_pos; const double* ln_x0; const double* ln_dir;
  const uint8_t* pt_out; const uint8_t* ln_out; const uint8_t* ln_removed; const float* level_scale;
  const int32_t* era_start;                   // [n_pts + 1] where a point's stored entries sit in era
  uint8_t* era;
  int32_t* p_ref;                             // null: lld_map_set_point_refs was never called
  // outputs
  int32_t* cnt; float* o_ow; float* o_pos; float* o_nrm; float* o_mind; float* o_maxd; int32_t* o_nobs; int32_t* o_ref; int32_t* o_len; uint8_t* o_flags;
  uint8_t* o_lbad; int32_t* o_lnobs; int32_t* o_llen; int32_t* o_lapplied;
};

__global__ void ap_cams_kernel(MapBa Y, ApArgs A) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.n_local) return;
  const int s = A.cam_slot[c];
  for (int k = 0; k < 7; k++) Y.k_qt[7 * (size_t)s + k] = A.cam_qt[7 * (size_t)c + k];
  for (int k = 0; k < 3; k++) Y.k_ow[3 * (size_t)s + k] = A.cam_ow[3 * (size_t)c + k];
}
__global__ void ap_cams_out_kernel(MapBa Y, ApArgs A) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= A.n_local) return;
  const int s = A.cam_slot[c];
  for (int k = 0; k < 3; k++) A.o_ow[3 * (size_t)c + k] = Y.k_ow[3 * (size_t)s + k];
}

// ------------------------------------------------------------------------------------------------ points: what goes (MapPoint.cc:111-168)
__global__ __launch_bounds__(kThreads) void ap_mark_kernel(MapDev M, MapExt X, MapBa Y, ApArgs A) {
  const int g = threadIdx.x / kGroup, gl = threadIdx.x % kGroup;
  for (int base = blockIdx.x * kGroups; base < A.n_pts; base += gridDim.x * kGroups) {     // uniform over the workgroup: the shuffles below are safe
    const int q = base + g;
    int nm = 0, ns = 0, skipped = 0;
    int s = -1; int2 row = make_int2(0, 0), ir = make_int2(0, 0); int e0 = 0, e1 = 0, at = 0;
    if (q < A.n_pts) {
      s = A.point_slot[q]; row = M.p_obs[s]; ir = X.p_idx[s]; e0 = A.pt_start[q]; e1 = A.pt_start[q + 1]; at = A.era_start[q];
      for (int j = gl; j < row.y; j += kGroup) {
        const int kf = M.obs_pool[row.x + j];
        bool hit = false;
        for (int e = e0; e < e1; e++) hit = hit || (A.pt_out[e] && A.cam_slot[A.pt_cam[e]] == kf);
        uint8_t code = 0;
        if (hit) {
          const int idx = X.idx_pool[ir.x + j];
          const int2 ur = Y.k_uvr[kf];
          code = 1;
          if (3 * (long long)idx + 2 < ur.y && __int_as_float(Y.uvr_pool[ur.x + 3 * idx + 2]) >= 0.f) code = 2;     // mvuRight[idx] >= 0
        }
        A.era[at + j] = code;
        nm += code == 1; ns += code == 2;
      }
    }
    lld_wave::sum_each<kGroup>(nm, ns);
    // EraseObservation after EraseObservation, the mono edges' first (:1282-1310): the first one that leaves n_obs <= 2 ends the walk
    int n = 0, applied = 0; bool bad = false;
    if (q < A.n_pts) {
      n = X.p_nobs[s];
      for (int t = 0; t < nm && !bad; t++) { n -= 1; applied++; bad = n <= 2; }
      for (int t = 0; t < ns && !bad; t++) { n -= 2; applied++; bad = n <= 2; }
      // KeyFrame::EraseMapPointMatch of the erased entries - of every entry when the point goes bad (SetBadFlag walks what is left)
      for (int j = gl; j < row.y; j += kGroup) {
        if (!bad && !A.era[at + j]) continue;
        const int kf = M.obs_pool[row.x + j], idx = X.idx_pool[ir.x + j];
        const int2 pr = M.k_pt[kf];
        if (idx < pr.y) M.kpt_pool[pr.x + idx] = -1; else skipped++;
      }
    }
    skipped = lld_wave::sum<kGroup>(skipped);
    if (gl == 0 && q < A.n_pts) {
      X.p_nobs[s] = n;
      if (bad) M.p_state[s] = 2;
      A.o_flags[q] = (uint8_t)((bad ? kBad : 0) | (skipped ? kSkipped : 0));
      if (applied) atomicAdd(&A.cnt[C_PT_ERASED], applied);
      if (bad) atomicAdd(&A.cnt[C_PT_BAD], 1);
      if (skipped) atomicAdd(&A.cnt[C_SKIPPED], skipped);
    }
  }
}

// ------------------------------------------------------------------------------------------------ lines (MapLine.cc:77-123)
__global__ void ap_lines_kernel(MapDev M, MapBa Y, ApArgs A) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= A.n_lns) return;
  const int s = A.line_slot[l];
  const int2 row = Y.l_obs[s], ir = Y.l_idx[s];
  int n = Y.l_nobs[s], len = min(row.y, ir.y), applied = 0, skipped = 0;
  bool bad = false;
  if (!A.ln_removed[l]) {                                              // GetLineData failed: the line is skipped whole (:1320-1323)
    for (int e = A.ln_start[l]; e < A.ln_start[l + 1] && !bad; e++) {
      if (!A.ln_out[2 * (size_t)e] && !A.ln_out[2 * (size_t)e + 1]) continue;
      const int kf = A.cam_slot[A.ln_cam[e]];
      int j = 0;
      while (j < len && Y.lobs_pool[row.x + j] != kf) j++;
      if (j == len) continue;                                          // mObservations.count(pKF) == 0
      const int idx = Y.lidx_pool[ir.x + j];
      const int2 lr = M.k_ln[kf], kl = Y.k_kl[kf];
      if (idx < lr.y) M.kln_pool[lr.x + idx] = -1; else skipped++;     // EraseMapLineMatch
      bool partner = false;                                            // line_matches[idx] >= 0
      if (10 * (long long)idx + 9 < kl.y) {
        const int32_t* f = Y.kl_pool + kl.x + 10 * (size_t)idx + 4;
        partner = !(f[0] == kMinusOneF && f[1] == kMinusOneF && f[2] == kMinusOneF && f[3] == kMinusOneF);
      }
      n -= partner ? 2 : 1;
      for (int k = j; k + 1 < len; k++) { Y.lobs_pool[row.x + k] = Y.lobs_pool[row.x + k + 1]; Y.lidx_pool[ir.x + k] = Y.lidx_pool[ir.x + k + 1]; }
      len--; applied++;
      bad = n <= 4;
    }
    // SetBadFlag clears mObservations before EraseMapLineMatch(this) looks the index up: the observers' entries stay
    if (bad) { len = 0; M.l_bad[s] = 1; }
    if (applied) { Y.l_nobs[s] = n; Y.l_obs[s] = make_int2(row.x, len); Y.l_idx[s] = make_int2(ir.x, len); }
    for (int k = 0; k < 3; k++) { M.l_x0[3 * (size_t)s + k] = A.ln_x0[3 * (size_t)l + k]; M.l_dir[3 * (size_t)s + k] = A.ln_dir[3 * (size_t)l + k]; }
    if (applied) atomicAdd(&A.cnt[C_LN_ERASED], applied);
    if (bad) atomicAdd(&A.cnt[C_LN_BAD], 1);
    if (skipped) atomicAdd(&A.cnt[C_SKIPPED], skipped);
  }
  A.o_lbad[l] = M.l_bad[s]; A.o_lnobs[l] = Y.l_nobs[s]; A.o_llen[l] = Y.l_obs[s].y; A.o_lapplied[l] = applied;
}

// ------------------------------------------------------------------------------------------------ points: mpRefKF, SetWorldPos, UpdateNormalAndDepth
__global__ __launch_bounds__(kThreads) void ap_refresh_kernel(MapDev M, MapExt X, MapBa Y, ApArgs A) {
  const int g = threadIdx.x / kGroup, gl = threadIdx.x % kGroup;
  for (int base = blockIdx.x * kGroups; base < A.n_pts; base += gridDim.x * kGroups) {     // uniform over the workgroup
    const int q = base + g;
    const bool on = q < A.n_pts;
    int s = 0; int2 row = make_int2(0, 0), ir = make_int2(0, 0); int at = 0; bool bad = false; int ref = -1;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (on) {
      s = A.point_slot[q]; row = M.p_obs[s]; ir = X.p_idx[s]; at = A.era_start[q]; bad = (A.o_flags[q] & kBad) != 0;
      if (A.p_ref) ref = A.p_ref[s];
      px = A.pt_pos[3 * (size_t)q]; py = A.pt_pos[3 * (size_t)q + 1]; pz = A.pt_pos[3 * (size_t)q + 2];
      if (gl < 3) M.p_pos[3 * (size_t)s + gl] = gl == 0 ? px : gl == 1 ? py : pz;           // SetWorldPos: bad or not
    }
    const int len = (on && !bad) ? row.y : 0;
    // the first entry that stays, whether the reference keyframe is erased, where it is, and whether every observer has a centre
    int first = 0x7fffffff, ref_at = 0x7fffffff, ref_gone = 0, no_centre = 0, kept = 0;
    for (int j = gl; j < len; j += kGroup) {
      const int kf = M.obs_pool[row.x + j];
      if (A.era[at + j]) { if (kf == ref) ref_gone = 1; continue; }
      kept++;
      first = min(first, j);
      if (kf == ref) ref_at = min(ref_at, j);
      if (!Y.k_feat[kf]) no_centre = 1;
    }
    first = lld_wave::min<kGroup>(first); ref_at = lld_wave::min<kGroup>(ref_at);
    lld_wave::sum_each<kGroup>(ref_gone, no_centre, kept);
    if (on && bad && ref != -1) { ref = -1; if (gl == 0) A.p_ref[s] = -1; }
    if (on && !bad && ref_gone && kept) {                              // mpRefKF = mObservations.begin()->first
      ref = M.obs_pool[row.x + first]; ref_at = first;
      if (gl == 0) A.p_ref[s] = ref;
    }
    if (!kept) continue;                                               // bad, or observations.empty(): the routine returns  (group-uniform)
    int level = -1;                                                    // of the reference keyframe's own observation
    if (ref >= 0 && !no_centre && A.has_ext) level = lld_nd::ref_level(ref, ref_at, len, X.idx_pool + ir.x, X.k_oct, X.oct_pool, Y.k_feat, A.n_levels);
    if (level < 0) { if (gl == 0) A.o_flags[q] |= kNoRef; continue; }       // (group-uniform)
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int j0 = 0; j0 < len; j0 += kGroup) {
      const int j = j0 + gl;
      float tx = 0.f, ty = 0.f, tz = 0.f; int keep = 0;
      if (j < len && !A.era[at + j]) { keep = 1; lld_nd::term(px, py, pz, Y.k_ow + 3 * (size_t)M.obs_pool[row.x + j], tx, ty, tz); }
      lld_nd::add_in_order<kGroup>(keep, tx, ty, tz, nx, ny, nz);
    }
    if (gl == 0) {
      lld_nd::finish(lld_nd::Out{M.p_nrm, M.p_mind, M.p_maxd}, s, px, py, pz, nx, ny, nz, kept, Y.k_ow + 3 * (size_t)ref, A.level_scale, level, A.n_levels);
      A.o_flags[q] |= kRefreshed;
    }
  }
}

// ------------------------------------------------------------------------------------------------ points: the rows, and what the tables hold now
__global__ void ap_rows_kernel(MapDev M, MapExt X, ApArgs A) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= A.n_pts) return;
  const int s = A.point_slot[q], at = A.era_start[q];
  const int2 row = M.p_obs[s], ir = X.p_idx[s];
  const uint8_t flags = A.o_flags[q];
  int w = 0;
  if (!(flags & kBad))
    for (int j = 0; j < row.y; j++) {
      if (A.era[at + j]) continue;
      if (w != j) { M.obs_pool[row.x + w] = M.obs_pool[row.x + j]; X.idx_pool[ir.x + w] = X.idx_pool[ir.x + j]; }
      w++;
    }
  if (w != row.y) { M.p_obs[s] = make_int2(row.x, w); X.p_idx[s] = make_int2(ir.x, w); }
  for (int k = 0; k < 3; k++) { A.o_pos[3 * (size_t)q + k] = M.p_pos[3 * (size_t)s + k]; A.o_nrm[3 * (size_t)q + k] = M.p_nrm[3 * (size_t)s + k]; }
  A.o_mind[q] = M.p_mind[s]; A.o_maxd[q] = M.p_maxd[s]; A.o_nobs[q] = X.p_nobs[s]; A.o_ref[q] = A.p_ref ? A.p_ref[s] : -1; A.o_len[q] = M.p_obs[s].y;
}

// ------------------------------------------------------------------------------------------------ lld_map_download_rows
__global__ void ap_download_rows_kernel(int n, const int32_t* slot, const int32_t* start, const int2* d_row, const int32_t* pool, int32_t* len, int32_t* data) {
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    const int2 w = d_row[slot[r]];
    const int room = start[r + 1] - start[r];
    if (threadIdx.x == 0) len[r] = w.y;
    for (int j = threadIdx.x; j < min(w.y, room); j += blockDim.x) data[start[r] + j] = pool[w.x + j];
  }
}

// entry `at` leaves rows a and b (parallel rows of one landmark): the entries behind it move up, the rows' places stay
void drop_entry(RowPool& a, RowPool& b, int s, int at) {
  int32_t* ra = a.mirror.data() + a.off[s]; int32_t* rb = b.mirror.data() + b.off[s];
  const int len = a.len[s];
  for (int k = at; k + 1 < len; k++) { ra[k] = ra[k + 1]; rb[k] = rb[k + 1]; }
  a.len[s] = b.len[s] = len - 1; a.live--; b.live--;
}
void drop_row(RowPool& a, RowPool& b, int s) { a.live -= a.len[s]; b.live -= b.len[s]; a.len[s] = b.len[s] = 0; }
void clear_match(RowPool& rows, int kf, int idx) { if (idx < rows.len[kf]) rows.mirror[rows.off[kf] + idx] = -1; }

RowPool* pool_of(lld_map* m, int kind, bool& allocated) {
  allocated = true;
  switch (kind) {
    case LLD_MAP_ROWS_POINT_OBS: return &m->obs;
    case LLD_MAP_ROWS_KF_POINTS: return &m->kpt;
    case LLD_MAP_ROWS_KF_LINES: return &m->kln;
    case LLD_MAP_ROWS_POINT_IDX: allocated = m->d_ext != nullptr; return &m->idx;
    case LLD_MAP_ROWS_LINE_OBS: allocated = m->d_ba != nullptr; return &m->lobs;
    case LLD_MAP_ROWS_LINE_IDX: allocated = m->d_ba != nullptr; return &m->lidx;
  }
  return nullptr;
}

}  // namespace

extern "C" {

int lld_map_ba_apply(lld_map* m, const lld_map_ba_apply_in* in, lld_map_ba_apply_out* out) {
  if (!m || !in || !out) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  const lld_map::BaStaged W = m->win;
  if (!W.valid || W.at != m->mutations || !m->d_ba || !m->d_ext) return LLD_ERR_INVALID;
  if (in->n_cams != W.n_cams || in->n_points != W.n_pts || in->n_pt_obs != W.n_ptobs || in->n_lines != W.n_lns || in->n_ln_obs != W.n_lnobs) return LLD_ERR_INVALID;
  if (in->n_levels < 1 || !in->level_scale) return LLD_ERR_INVALID;
  const size_t nloc = W.n_local, np = W.n_pts, npo = W.n_ptobs, nl = W.n_lns, nlo = W.n_lnobs;
  if ((W.n_cams > 0 && !in->cam_qt) || (np && !in->pt_xyz) || (npo && !in->pt_obs_outlier) || (nl && (!in->line_x0 || !in->line_dir || !in->line_removed)) ||
      (nlo && !in->ln_edge_outlier)) return LLD_ERR_INVALID;
  if ((nloc && (!out->tcw || !out->ow)) || (np && (!out->pt_pos || !out->pt_normal || !out->pt_min_distance || !out->pt_max_distance || !out->pt_n_obs || !out->pt_ref_kf ||
                                                  !out->pt_row_len || !out->pt_flags)) || (nl && (!out->ln_bad || !out->ln_n_obs || !out->ln_row_len))) return LLD_ERR_INVALID;
  // the window as the host received it; the rows of its points as the host keeps them (they are the device's: the map has not changed)
  const int32_t* w_cam_slot = reinterpret_cast<const int32_t*>(m->ba.h + W.cam_slot);
  const int32_t* w_point = reinterpret_cast<const int32_t*>(m->ba.h + W.point_slot);
  const int32_t* w_pt_start = reinterpret_cast<const int32_t*>(m->ba.h + W.pt_start);
  const int32_t* w_pt_cam = reinterpret_cast<const int32_t*>(m->ba.h + W.pt_cam);
  const int32_t* w_line = reinterpret_cast<const int32_t*>(m->ba.h + W.line_slot);
  const int32_t* w_ln_start = reinterpret_cast<const int32_t*>(m->ba.h + W.ln_start);
  const int32_t* w_ln_cam = reinterpret_cast<const int32_t*>(m->ba.h + W.ln_cam);
  long long era_total = 0;
  for (size_t q = 0; q < np; q++) {
    const int s = w_point[q];
    if (m->idx.len[s] != m->obs.len[s]) return LLD_ERR_INVALID;        // (a window with status 0 has an index row for every point)
    era_total += m->obs.len[s];
  }
  for (size_t l = 0; l < nl; l++) if (m->lidx.len[w_line[l]] != m->lobs.len[w_line[l]]) return LLD_ERR_INVALID;
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  UploadBlock B;
  const auto u_qt = B.take<double>(nloc, 7); const auto u_ow = B.take<float>(nloc, 3), u_pos = B.take<float>(np, 3); const auto u_x0 = B.take<double>(nl, 3), u_dir = B.take<double>(nl, 3);
  const auto u_po = B.take<uint8_t>(npo), u_lo = B.take<uint8_t>(nlo, 2), u_rm = B.take<uint8_t>(nl); const auto u_ls = B.take<float>(in->n_levels);
  const auto u_es = B.take<int32_t>(np + 1);
  B.end_upload();
  const auto r_cnt = B.take<int32_t>(C_WORDS); const auto r_ow = B.take<float>(nloc, 3), r_pos = B.take<float>(np, 3), r_nrm = B.take<float>(np, 3), r_min = B.take<float>(np), r_max = B.take<float>(np);
  const auto r_nobs = B.take<int32_t>(np), r_ref = B.take<int32_t>(np), r_len = B.take<int32_t>(np); const auto r_fl = B.take<uint8_t>(np), r_lbad = B.take<uint8_t>(nl);
  const auto r_lnobs = B.take<int32_t>(nl), r_llen = B.take<int32_t>(nl), r_lapp = B.take<int32_t>(nl);
  B.end_download();
  const auto t_era = B.take<uint8_t>((size_t)era_total);
  int st = m->ap.grow(ctx->stream, B.travel_bytes(), B.size); if (st) return st;
  B.bind(m->ap.h, m->ap.d);

  float* tcw = out->tcw;
  for (size_t c = 0; c < nloc; c++) {                                  // SetPose(Converter::toCvMat(SE3quat)) (:1369): the float matrix is what the keyframe keeps
    lld_se3_to_tcw_f32(in->cam_qt + 7 * c, tcw + 16 * c);
    lld_se3_from_tcw_f32(tcw + 16 * c, B.host(u_qt) + 7 * c);
    lld::camera_centre(tcw + 16 * c, B.host(u_ow) + 3 * c);
  }
  for (size_t k = 0; k < 3 * np; k++) B.host(u_pos)[k] = (float)in->pt_xyz[k];
  B.stage(u_x0, in->line_x0); B.stage(u_dir, in->line_dir); B.stage(u_po, in->pt_obs_outlier); B.stage(u_lo, in->ln_edge_outlier); B.stage(u_rm, in->line_removed);
  B.stage(u_ls, in->level_scale);
  { int32_t* es = B.host(u_es); es[0] = 0; for (size_t q = 0; q < np; q++) es[q + 1] = es[q] + m->obs.len[w_point[q]]; }

  ApArgs A{};
  A.n_local = W.n_local; A.n_pts = W.n_pts; A.n_lns = W.n_lns; A.n_levels = in->n_levels; A.has_ext = 1;
  const char* dw = m->ba.d;
  A.cam_slot = reinterpret_cast<const int32_t*>(dw + W.cam_slot); A.point_slot = reinterpret_cast<const int32_t*>(dw + W.point_slot);
  A.pt_start = reinterpret_cast<const int32_t*>(dw + W.pt_start); A.pt_cam = reinterpret_cast<const int32_t*>(dw + W.pt_cam);
  A.line_slot = reinterpret_cast<const int32_t*>(dw + W.line_slot); A.ln_start = reinterpret_cast<const int32_t*>(dw + W.ln_start);
  A.ln_cam = reinterpret_cast<const int32_t*>(dw + W.ln_cam);
  A.cam_qt = B.dev(u_qt); A.cam_ow = B.dev(u_ow); A.pt_pos = B.dev(u_pos); A.ln_x0 = B.dev(u_x0); A.ln_dir = B.dev(u_dir);
  A.pt_out = B.dev(u_po); A.ln_out = B.dev(u_lo); A.ln_removed = B.dev(u_rm); A.level_scale = B.dev(u_ls); A.era_start = B.dev(u_es); A.era = B.dev(t_era);
  A.p_ref = m->d_ref;
  A.cnt = B.dev(r_cnt); A.o_ow = B.dev(r_ow); A.o_pos = B.dev(r_pos); A.o_nrm = B.dev(r_nrm); A.o_mind = B.dev(r_min); A.o_maxd = B.dev(r_max);
  A.o_nobs = B.dev(r_nobs); A.o_ref = B.dev(r_ref); A.o_len = B.dev(r_len); A.o_flags = B.dev(r_fl);
  A.o_lbad = B.dev(r_lbad); A.o_lnobs = B.dev(r_lnobs); A.o_llen = B.dev(r_llen); A.o_lapplied = B.dev(r_lapp);

  // from here on the tables move: the window is spent, and a HIP failure leaves host rows and device rows apart
  m->mutations++; m->win.valid = false;
  st = lld_rt::round_trip(ctx->stream, B, out->phase_ms, [&](hipStream_t sm) {
    LLD_HIP_TRY(hipMemsetAsync(B.dev(r_cnt), 0, C_WORDS * 4, sm));
    const dim3 grouped((unsigned)std::min<size_t>(std::max<size_t>((np + kGroups - 1) / kGroups, 1), 2048));
    if (nloc) hipLaunchKernelGGL(ap_cams_kernel, blocks(nloc, kThreads), dim3(kThreads), 0, sm, m->Y, A);
    if (np) hipLaunchKernelGGL(ap_mark_kernel, grouped, dim3(kThreads), 0, sm, m->D, m->X, m->Y, A);
    if (nl) hipLaunchKernelGGL(ap_lines_kernel, blocks(nl, 64), dim3(64), 0, sm, m->D, m->Y, A);
    if (np) hipLaunchKernelGGL(ap_refresh_kernel, grouped, dim3(kThreads), 0, sm, m->D, m->X, m->Y, A);
    if (np) hipLaunchKernelGGL(ap_rows_kernel, blocks(np, 64), dim3(64), 0, sm, m->D, m->X, A);
    if (nloc) hipLaunchKernelGGL(ap_cams_out_kernel, blocks(nloc, kThreads), dim3(kThreads), 0, sm, m->Y, A);
    return LLD_OK;
  });
  if (st) { m->poisoned = true; return st; }

  // The host's rows follow: the same removals, from the flags that went up and the verdicts that came down.
  const uint8_t* fl = B.host(r_fl); const int32_t* dev_len = B.host(r_len);
  bool same = true;
  for (size_t q = 0; q < np; q++) {
    const int s = w_point[q];
    const int32_t* kfs = m->obs.mirror.data() + m->obs.off[s]; const int32_t* ids = m->idx.mirror.data() + m->idx.off[s];
    if (fl[q] & kBad) {
      for (int j = 0; j < m->obs.len[s]; j++) clear_match(m->kpt, kfs[j], ids[j]);
      drop_row(m->obs, m->idx, s);
    } else {
      for (int e = w_pt_start[q]; e < w_pt_start[q + 1]; e++) {
        if (!in->pt_obs_outlier[e]) continue;
        const int kf = w_cam_slot[w_pt_cam[e]];
        int j = 0;
        while (j < m->obs.len[s] && kfs[j] != kf) j++;
        if (j == m->obs.len[s]) continue;
        clear_match(m->kpt, kf, ids[j]);
        drop_entry(m->obs, m->idx, s, j);
      }
    }
    same = same && m->obs.len[s] == dev_len[q];
  }
  const uint8_t* lbad = B.host(r_lbad); const int32_t* lapp = B.host(r_lapp); const int32_t* dev_llen = B.host(r_llen);
  for (size_t l = 0; l < nl; l++) {
    const int s = w_line[l];
    if (!in->line_removed[l]) {
      const int32_t* kfs = m->lobs.mirror.data() + m->lobs.off[s]; const int32_t* ids = m->lidx.mirror.data() + m->lidx.off[s];
      int applied = 0;
      for (int e = w_ln_start[l]; e < w_ln_start[l + 1] && applied < lapp[l]; e++) {
        if (!in->ln_edge_outlier[2 * (size_t)e] && !in->ln_edge_outlier[2 * (size_t)e + 1]) continue;
        const int kf = w_cam_slot[w_ln_cam[e]];
        int j = 0;
        while (j < m->lobs.len[s] && kfs[j] != kf) j++;
        if (j == m->lobs.len[s]) continue;
        clear_match(m->kln, kf, ids[j]);
        drop_entry(m->lobs, m->lidx, s, j);
        applied++;
      }
      if (applied && lbad[l]) drop_row(m->lobs, m->lidx, s);
    }
    same = same && m->lobs.len[s] == dev_llen[l];
  }
  if (!same) { m->poisoned = true; return LLD_ERR_HIP; }               // the device's rows are not the host's: never with a sound map

  const int32_t* cnt = B.host(r_cnt);
  out->n_local_cams = W.n_local; out->n_pt_obs_erased = cnt[C_PT_ERASED]; out->n_ln_obs_erased = cnt[C_LN_ERASED]; out->n_points_bad = cnt[C_PT_BAD];
  out->n_lines_bad = cnt[C_LN_BAD]; out->n_index_skipped = cnt[C_SKIPPED];
  copy_out(out->ow, B, r_ow, 3 * nloc);
  copy_out(out->pt_pos, B, r_pos, 3 * np); copy_out(out->pt_normal, B, r_nrm, 3 * np); copy_out(out->pt_min_distance, B, r_min, np); copy_out(out->pt_max_distance, B, r_max, np);
  copy_out(out->pt_n_obs, B, r_nobs, np); copy_out(out->pt_ref_kf, B, r_ref, np); copy_out(out->pt_row_len, B, r_len, np); copy_out(out->pt_flags, B, r_fl, np);
  copy_out(out->ln_bad, B, r_lbad, nl); copy_out(out->ln_n_obs, B, r_lnobs, nl); copy_out(out->ln_row_len, B, r_llen, nl);
  return LLD_OK;
}

int lld_map_download_rows(lld_map* m, int32_t kind, int32_t n, const int32_t* slot, int32_t* start, int32_t capacity, int32_t* data) {
  if (!m || n < 0 || capacity < 0) return LLD_ERR_INVALID;
  bool allocated = false;
  RowPool* P = pool_of(m, kind, allocated);
  if (!P) return LLD_ERR_INVALID;
  if (m->poisoned) return LLD_ERR_HIP;
  if (n == 0) return LLD_OK;
  if (!slot || !start || (capacity > 0 && !data)) return LLD_ERR_INVALID;
  const int rows = kind == LLD_MAP_ROWS_KF_POINTS || kind == LLD_MAP_ROWS_KF_LINES ? m->lim.max_keyframes
                 : kind == LLD_MAP_ROWS_POINT_OBS || kind == LLD_MAP_ROWS_POINT_IDX ? m->lim.max_points : m->lim.max_lines;
  for (int i = 0; i < n; i++) if (slot[i] < 0 || slot[i] >= rows) return LLD_ERR_INVALID;
  // the lengths are the host's (every update before this call is queued before its kernel); the contents come from the device
  std::vector<int32_t> st((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) st[i + 1] = st[i] + (allocated ? P->len[slot[i]] : 0);
  std::memcpy(start, st.data(), ((size_t)n + 1) * 4);
  if (st[n] > capacity) return LLD_ERR_INVALID;                        // only start is written
  if (!allocated) return LLD_OK;
  lld_ctx* ctx = m->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  UploadBlock B;
  const auto i_s = B.take<int32_t>(n), i_st = B.take<int32_t>((size_t)n + 1);
  B.end_upload();
  const auto r_len = B.take<int32_t>(n), r_data = B.take<int32_t>((size_t)st[n]);
  B.end_download();
  int rc;
  void* hb; rc = lld_ctx_pinned(ctx, B.size, &hb); if (rc) return rc;
  void* db; rc = lld_ctx_scratch(ctx, B.size + 256, &db); if (rc) return rc;
  B.bind((char*)hb, (char*)db);
  B.stage(i_s, slot); B.stage(i_st, st.data());
  rc = lld_rt::round_trip(ctx->stream, B, nullptr, [&](hipStream_t sm) {
    hipLaunchKernelGGL(ap_download_rows_kernel, dim3(std::min(n, 4096)), dim3(64), 0, sm, n, B.dev(i_s), B.dev(i_st), P->d_row, P->d_pool, B.dev(r_len), B.dev(r_data));
    return LLD_OK;
  });
  if (rc) return rc;
  const int32_t* len = B.host(r_len);
  for (int i = 0; i < n; i++) if (len[i] != st[i + 1] - st[i]) return LLD_ERR_HIP;         // the device's rows are not the host's: never with a sound map
  if (st[n]) std::memcpy(data, B.host(r_data), (size_t)st[n] * 4);
  return LLD_OK;
}

}  // extern "C"
