// lld_map_correct.hip — the three places where the loop-closing thread MOVES the map, each as one call:
//   lld_loop_correct            LoopClosing::CorrectLoop, src/LoopClosing.cc:440-518 (Sim3 propagation, point correction, UpdateNormalAndDepth, SetPose)
//   lld_essential_graph_apply   the write-back of Optimizer::OptimizeEssentialGraph, src/Optimizer.cc:1601-1653
//   lld_global_ba_apply         the map update of LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:678-739
// The rules restated and the limits are written out in include/lld_amd.h; tests/loopcorr_ref.py restates them in numpy, sequentially in the
// reference's loop order.  One call = one upload (lld_upload_block.h), its kernels on the context's stream, one download, one wait.
//
// The whole file is compiled without FMA contraction: every operation is the one IEEE operation the reference's host code performs.
//
// Kernels (no LDS, no scratch; the only atomic is the integer atomicMin of the owner pass):
//   mc_centres        one thread per keyframe: Ow = -Rcw^T tcw of the poses on entry (KeyFrame::SetPose, src/KeyFrame.cc:82-85).
//   mc_loop_poses     one thread per connected keyframe, in double: Tic = Tiw*Twc, the two Sim3, the corrected SE3 pose and its centre.
//   mc_owner          one thread per (connected keyframe, point) entry: atomicMin of the keyframe's rank on the point's word.  The minimum of
//                     integers does not depend on the order in which the entries arrive.
//   mc_points_loop / mc_points_graph   one thread per point, grid-stride: CorrectedSwi.map(Siw.map(P)) in double, rounded to float once.
//   mc_graph_poses    one thread per keyframe: Sim3 -> SE3 of the optimised essential graph, its centre, and the inverse the points use.
//   mc_normal<W>      UpdateNormalAndDepth for whole maps: a group of W lanes per point (W = 8: eight points per wavefront, for the points
//                     with at most 8 observations, the bulk of a map; W = 64: one point per wavefront, longer lists in chunks of 64).  Lane i of
//                     a group forms term i; every lane of the group then adds the terms in observation order through group broadcasts, so
//                     the float sum is lm_normal_wave's, bit for bit.  The host bins the points by observation count while it stages them.
//   mc_gba_chain      one workgroup: the poses of the keyframes Global BA did not optimise, composed down the spanning tree one depth at a
//                     time (the float roundings are ordered).  The host derives the depths and refuses a cycle, so the loop is bounded.
//   mc_gba_centres / mc_points_gba    one thread per keyframe / per point: all float cv::Mat arithmetic.
// No kernel follows an index the host has not range-checked.
#pragma clang fp contract(off)

#include <climits>
#include <cmath>
#include <vector>

#include "lld_common.h"
#include "lld_normal_depth.h"
#include "lld_sim3_math.h"
#include "lld_upload_block.h"
#include "lld_wave.h"

namespace {

using lld_track::Span;
using lld_track::UploadBlock;

constexpr int kBlock = 256;
constexpr int kNoOwner = 0x7f7f7f7f;         // the staged fill of the owner words: above every rank

// ------------------------------------------------------------------------------------------------------------------ float cv::Mat forms
// A pose is Tcw[12], the rows of [R|t]; the fourth row of the cv::Mat is (0, 0, 0, 1).

// Ow = -Rwc*tcw with Rwc = Rcw.t() (KeyFrame.cc:84-85): one gemm, double accumulation, one rounding
__device__ __forceinline__ void centre_of(const float* T, float* ow) { lld::camera_centre(T, ow); }
// Twc = [Rcw^T | Ow] (KeyFrame.cc:87-89)
__device__ __forceinline__ void inverse_of(const float* T, float* Twc) {
  float ow[3];
  centre_of(T, ow);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Twc[4 * i + j] = T[4 * j + i];
    Twc[4 * i + 3] = ow[i];
  }
}
// C = A*B of two 4x4 float matrices: every entry the four-term double sum in index order, rounded once - the translation column included
__device__ __forceinline__ void mul44(const float* A, const float* B, float* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = (double)A[4 * i] * (double)B[j];
      s += (double)A[4 * i + 1] * (double)B[4 + j];
      s += (double)A[4 * i + 2] * (double)B[8 + j];
      s += (double)A[4 * i + 3] * (j == 3 ? 1.0 : 0.0);
      C[4 * i + j] = (float)s;
    }
}
// Sim3(toMatrix3d(R), toVector3d(t), 1.0) of a float pose
__device__ __forceinline__ Sim3 sim3_of_pose(const float* T) {
  Mat3 R;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R.m[i][j] = (double)T[4 * i + j];
  Sim3 S; S.r = quat_from_rotation(R); S.t = vec3((double)T[3], (double)T[7], (double)T[11]); S.s = 1.0;
  return S;
}
// toCvSE3(R(q), t*(1./s)): a reciprocal and then a product (LoopClosing.cc:506-512, Optimizer.cc:1611-1617)
__device__ __forceinline__ void se3_of_sim3(const Sim3& S, float* T) {
  const Mat3 R = quat_rotation(S.r);
  const Vec3 t = (1. / S.s) * S.t;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R.m[i][j];
  T[3] = (float)t.x; T[7] = (float)t.y; T[11] = (float)t.z;
}

// ------------------------------------------------------------------------------------------------------------------ keyframe kernels
// grid: n_kf threads
__global__ __launch_bounds__(kBlock) void mc_centres(int n_kf, const float* __restrict__ tcw, float* __restrict__ ow) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k < n_kf) centre_of(tcw + 12 * (size_t)k, ow + 3 * (size_t)k);
}

struct LoopPoseArgs {
  int n_conn, cur;
  const int32_t* conn; const float* tcw; const double* scw;
  double* corrected; double* non_corrected; double* swi;     // [n_conn][8] each; swi = CorrectedSiw.inverse()
  float* tiw; float* ow; float* scw_f32;                     // per rank
  float* ow_new;                                             // [n_kf][3], written at the connected slots only
};

// grid: n_conn threads
__global__ __launch_bounds__(kBlock) void mc_loop_poses(LoopPoseArgs A) {
  const int r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= A.n_conn) return;
  const int kf = A.conn[r];
  const float* Tiw = A.tcw + 12 * (size_t)kf;
  const Sim3 Scw = sim3_load(A.scw);
  Sim3 corr = Scw;                                           // CorrectedSim3[mpCurrentKF] = mg2oScw (:441)
  if (r != A.cur) {
    float Twc[12], Tic[12];
    inverse_of(A.tcw + 12 * (size_t)A.conn[A.cur], Twc);     // mpCurrentKF->GetPoseInverse() (:442)
    mul44(Tiw, Twc, Tic);                                    // (:457)
    corr = sim3_mul(sim3_of_pose(Tic), Scw);                 // (:460-461)
  }
  const Sim3 non = sim3_of_pose(Tiw);                        // (:468)
  sim3_store(corr, A.corrected + 8 * (size_t)r);
  sim3_store(non, A.non_corrected + 8 * (size_t)r);
  sim3_store(sim3_inverse(corr), A.swi + 8 * (size_t)r);     // (:478)
  float T[12];
  se3_of_sim3(corr, T);                                      // (:506-512)
  float ow[3];
  centre_of(T, ow);                                          // SetPose (:514)
#pragma unroll
  for (int i = 0; i < 12; ++i) A.tiw[12 * (size_t)r + i] = T[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { A.ow[3 * (size_t)r + i] = ow[i]; A.ow_new[3 * (size_t)kf + i] = ow[i]; }
  const Mat3 R = quat_rotation(corr.r);                      // toCvMat(Sim3) = toCvSE3(s*R, t) (Converter.cc:55-61)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A.scw_f32[12 * (size_t)r + 4 * i + j] = (float)(corr.s * R.m[i][j]);
  A.scw_f32[12 * (size_t)r + 3] = (float)corr.t.x; A.scw_f32[12 * (size_t)r + 7] = (float)corr.t.y; A.scw_f32[12 * (size_t)r + 11] = (float)corr.t.z;
}

struct GraphPoseArgs { int n_kf; const double* after; double* swr; float* tiw; float* ow; };

// grid: n_kf threads
__global__ __launch_bounds__(kBlock) void mc_graph_poses(GraphPoseArgs A) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= A.n_kf) return;
  const Sim3 S = sim3_load(A.after + 8 * (size_t)k);
  sim3_store(sim3_inverse(S), A.swr + 8 * (size_t)k);        // vCorrectedSwc (:1610)
  float T[12];
  se3_of_sim3(S, T);
#pragma unroll
  for (int i = 0; i < 12; ++i) A.tiw[12 * (size_t)k + i] = T[i];
  centre_of(T, A.ow + 3 * (size_t)k);
}

// ------------------------------------------------------------------------------------------------------------------ point kernels
// grid: n_entries threads.  kf_start[n_conn + 1] is the CSR of the per-keyframe lists: the rank of an entry by bisection.
__global__ __launch_bounds__(kBlock) void mc_owner(int n_entries, int n_conn, const int32_t* __restrict__ kf_start, const int32_t* __restrict__ kf_point,
                                                   const uint8_t* __restrict__ bad, const uint8_t* __restrict__ already, int32_t* owner) {
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_entries) return;
  int lo = 0, hi = n_conn;                                   // the last rank with kf_start[rank] <= e
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (kf_start[mid] <= e) lo = mid; else hi = mid; }
  const int p = kf_point[e];
  if (bad[p] || already[p]) return;                          // (:488-491)
  atomicMin(&owner[p], lo);
}

// The corrected position (:494-499, Optimizer.cc:1645-1650): widened to double, two Sim3 maps, rounded to float once
__device__ __forceinline__ void correct_point(const double* siw, const double* swi, const float* pin, float* pout) {
  const Vec3 P = vec3((double)pin[0], (double)pin[1], (double)pin[2]);
  const Vec3 Q = sim3_map(sim3_load(swi), sim3_map(sim3_load(siw), P));
  pout[0] = (float)Q.x; pout[1] = (float)Q.y; pout[2] = (float)Q.z;
}

// grid-stride over the points.  upd bit 0: the point was moved.
__global__ __launch_bounds__(kBlock) void mc_points_loop(int n, int n_conn, const int32_t* __restrict__ owner, const double* __restrict__ siw,
                                                         const double* __restrict__ swi, const float* __restrict__ pos, float* __restrict__ pos_new,
                                                         int32_t* __restrict__ corrected_by, uint8_t* __restrict__ upd) {
  for (int p = blockIdx.x * kBlock + threadIdx.x; p < n; p += gridDim.x * kBlock) {
    const int k = owner[p];
    if (k >= n_conn) { corrected_by[p] = -1; upd[p] = 0; continue; }
    correct_point(siw + 8 * (size_t)k, swi + 8 * (size_t)k, pos + 3 * (size_t)p, pos_new + 3 * (size_t)p);
    corrected_by[p] = k; upd[p] = LLD_MAPCORR_MOVED;
  }
}
__global__ __launch_bounds__(kBlock) void mc_points_graph(int n, const uint8_t* __restrict__ bad, const int32_t* __restrict__ corr_kf,
                                                          const double* __restrict__ before, const double* __restrict__ swr,
                                                          const float* __restrict__ pos, float* __restrict__ pos_new, uint8_t* __restrict__ upd) {
  for (int p = blockIdx.x * kBlock + threadIdx.x; p < n; p += gridDim.x * kBlock) {
    if (bad[p]) { upd[p] = 0; continue; }                    // (:1627-1628)
    const int r = corr_kf[p];
    correct_point(before + 8 * (size_t)r, swr + 8 * (size_t)r, pos + 3 * (size_t)p, pos_new + 3 * (size_t)p);
    upd[p] = LLD_MAPCORR_MOVED;
  }
}

// ------------------------------------------------------------------------------------------------------------------ normal and depth
struct NormalArgs {
  const int32_t* list; int n_list;           // the points of this launch: every one has at least one observation
  const int32_t* obs_start; const int32_t* obs_kf;
  lld_nd::Centres C;
  const float* pos;                          // the corrected positions
  const int32_t* owner; int n_conn;          // loop correction: a point without an owner is skipped, and the owner's rank picks the centres
  const uint8_t* bad;                        // owner == nullptr: a bad point is skipped
  const int32_t* ref_kf; const int32_t* ref_level; const float* level_scale; int n_levels;
  lld_nd::Out O; uint8_t* upd;
};

// grid: ceil(n_list / (256 / W)) blocks of 256; a group of W lanes per point
template <int W>
__global__ __launch_bounds__(kBlock) void mc_normal(NormalArgs A) {
  const int g = (blockIdx.x * kBlock + threadIdx.x) / W, gl = threadIdx.x & (W - 1);
  if (g >= A.n_list) return;                 // whole groups leave
  const int p = A.list[g];
  int k = 0;
  if (A.owner != nullptr) { k = A.owner[p]; if (k >= A.n_conn) return; }
  else if (A.bad[p]) return;                 // mbBad returns (MapPoint.cc:338-339)
  const int s = A.obs_start[p], e = A.obs_start[p + 1];
  const float px = A.pos[3 * (size_t)p], py = A.pos[3 * (size_t)p + 1], pz = A.pos[3 * (size_t)p + 2];
  float nx = 0.f, ny = 0.f, nz = 0.f;
  for (int c = s; c < e; c += W) {
    const int o = c + gl;
    float tx = 0.f, ty = 0.f, tz = 0.f;
    if (o < e) lld_nd::term(px, py, pz, lld_nd::centre(A.C, A.obs_kf[o], k), tx, ty, tz);
    const int cnt = e - c < W ? e - c : W;
    for (int l = 0; l < cnt; ++l) {          // normal = normal + ... in observation order, the same sum in every lane of the group
      if constexpr (W == 64) {               // the group is the wavefront: l is uniform
        nx = nx + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tx), l));
        ny = ny + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ty), l));
        nz = nz + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tz), l));
      } else {
        nx = nx + lld_wave::group_bcast<W>(tx, l); ny = ny + lld_wave::group_bcast<W>(ty, l); nz = nz + lld_wave::group_bcast<W>(tz, l);
      }
    }
  }
  if (gl == 0) {
    lld_nd::finish(A.O, p, px, py, pz, nx, ny, nz, e - s, lld_nd::centre(A.C, A.ref_kf[p], k), A.level_scale, A.ref_level[p], A.n_levels);
    A.upd[p] = LLD_MAPCORR_MOVED | LLD_LANDMARK_NORMAL_DEPTH;
  }
}

// ------------------------------------------------------------------------------------------------------------------ global BA
struct GbaChainArgs {
  int n_depths; const int32_t* depth_start; const int32_t* list;   // the visited keyframes Global BA did not optimise, by depth below one it did
  const int32_t* parent; const float* tcw; float* gba;             // gba[n_kf][12]: mTcwGBA
};

// grid: one block.  Depth d reads only depth d - 1 (or an optimised keyframe): a barrier between depths orders the float roundings.
__global__ __launch_bounds__(kBlock) void mc_gba_chain(GbaChainArgs A) {
  for (int d = 0; d < A.n_depths; ++d) {
    for (int i = A.depth_start[d] + threadIdx.x; i < A.depth_start[d + 1]; i += kBlock) {
      const int c = A.list[i], par = A.parent[c];
      float Twc[12], Tchildc[12], T[12];
      inverse_of(A.tcw + 12 * (size_t)par, Twc);             // pKF->GetPoseInverse(), before its SetPose (:685)
      mul44(A.tcw + 12 * (size_t)c, Twc, Tchildc);           // (:691)
      mul44(Tchildc, A.gba + 12 * (size_t)par, T);           // (:692)
#pragma unroll
      for (int q = 0; q < 12; ++q) A.gba[12 * (size_t)c + q] = T[q];
    }
    __threadfence_block();
    __syncthreads();
  }
}

// grid: n_kf threads
__global__ __launch_bounds__(kBlock) void mc_gba_centres(int n_kf, const uint8_t* __restrict__ visited, const float* __restrict__ gba, float* __restrict__ ow) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k < n_kf && visited[k]) centre_of(gba + 12 * (size_t)k, ow + 3 * (size_t)k);
}

struct GbaPointArgs {
  int n; const uint8_t* bad; const uint8_t* in_gba; const float* pos; const int32_t* ref_kf;   // pos: mPosGBA where in_gba, mWorldPos elsewhere
  const uint8_t* visited; const float* tcw; const float* gba; const float* ow_new;
  float* pos_new; uint8_t* moved;
};

__global__ __launch_bounds__(kBlock) void mc_points_gba(GbaPointArgs A) {
  for (int p = blockIdx.x * kBlock + threadIdx.x; p < A.n; p += gridDim.x * kBlock) {
    if (A.bad[p]) { A.moved[p] = 0; continue; }                                          // (:711-712)
    float* out = A.pos_new + 3 * (size_t)p;
    if (A.in_gba[p]) {                                                                   // (:714-718)
#pragma unroll
      for (int i = 0; i < 3; ++i) out[i] = A.pos[3 * (size_t)p + i];
      A.moved[p] = 1; continue;
    }
    const int r = A.ref_kf[p];
    if (!A.visited[r]) { A.moved[p] = 0; continue; }                                     // (:724-725)
    const float* Tb = A.tcw + 12 * (size_t)r;                                            // mTcwBefGBA
    const float* Tn = A.gba + 12 * (size_t)r;
    const float* P = A.pos + 3 * (size_t)p;
    float Xc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                                        // Xc = Rcw*P + tcw (:730)
      double s = (double)Tb[4 * i] * (double)P[0];
      s += (double)Tb[4 * i + 1] * (double)P[1];
      s += (double)Tb[4 * i + 2] * (double)P[2];
      Xc[i] = (float)s + Tb[4 * i + 3];
    }
    const float Rn[9] = {Tn[0], Tn[1], Tn[2], Tn[4], Tn[5], Tn[6], Tn[8], Tn[9], Tn[10]};
    float X[3];
    lld::rwc_mul(Rn, Xc, X);                                                             // Rwc*Xc + twc (:737)
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = X[i] + A.ow_new[3 * (size_t)r + i];
    A.moved[p] = 2;
  }
}

// ------------------------------------------------------------------------------------------------------------------ host side
bool finite_all(const float* v, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }
bool sim3_ok(const double* s) {
  for (int i = 0; i < 8; ++i) if (!std::isfinite(s[i])) return false;
  return s[7] > 0.0;
}

// The point table of (a) and (b): INVALID for a malformed table, UNSUPPORTED above the limits (reported after every INVALID).
// `skips(p)`: the rule never reads the reference keyframe of p.
template <class F>
int check_points(const lld_mapcorr_points* P, int n_kf, F skips) {
  const int n = P->n_points, n_obs = P->n_obs;
  if (n < 0 || n_obs < 0) return LLD_ERR_INVALID;
  if (n == 0) return LLD_OK;
  if (!P->pos || !P->bad || !P->obs_start || (n_obs > 0 && !P->obs_kf) || !P->ref_kf || !P->ref_level || !P->level_scale) return LLD_ERR_INVALID;
  if (P->n_levels < 1 || P->n_levels > LLD_ORB_MAX_LEVELS) return LLD_ERR_INVALID;
  if (P->obs_start[0] != 0 || P->obs_start[n] != n_obs) return LLD_ERR_INVALID;
  for (int i = 0; i < n; ++i) if (P->obs_start[i + 1] < P->obs_start[i]) return LLD_ERR_INVALID;
  for (int o = 0; o < n_obs; ++o) if (P->obs_kf[o] < 0 || P->obs_kf[o] >= n_kf) return LLD_ERR_INVALID;
  for (int i = 0; i < n; ++i) {
    if (P->obs_start[i + 1] == P->obs_start[i] || skips(i)) continue;
    if (P->ref_kf[i] < 0 || P->ref_kf[i] >= n_kf || P->ref_level[i] < 0 || P->ref_level[i] >= P->n_levels) return LLD_ERR_INVALID;
  }
  if (n > LLD_MAPCORR_MAX_POINTS) return LLD_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i) if (P->obs_start[i + 1] - P->obs_start[i] > LLD_LANDMARK_MAX_OBS) return LLD_ERR_UNSUPPORTED;
  return LLD_OK;
}

// The uploaded half of the point table and the two launch lists of mc_normal, binned while the table is staged.
struct PointSpans {
  Span<float> pos; Span<uint8_t> bad; Span<int32_t> obs_start, obs_kf, ref_kf, ref_level, list; Span<float> level_scale;
  int n_small = 0, n_wave = 0;               // list[0, n_small): 1..8 observations; list[n_small, n_small + n_wave): more
  void reserve(UploadBlock& B, const lld_mapcorr_points* P) {
    const size_t n = (size_t)P->n_points;
    pos = B.take<float>(n, 3); bad = B.take<uint8_t>(n); obs_start = B.take<int32_t>(n + 1); obs_kf = B.take<int32_t>((size_t)P->n_obs);
    ref_kf = B.take<int32_t>(n); ref_level = B.take<int32_t>(n); list = B.take<int32_t>(n); level_scale = B.take<float>(LLD_ORB_MAX_LEVELS);
  }
  void stage(const UploadBlock& B, const lld_mapcorr_points* P) {
    B.stage(pos, P->pos); B.stage(bad, P->bad); B.stage(obs_start, P->obs_start); B.stage(obs_kf, P->obs_kf);
    B.stage(ref_kf, P->ref_kf); B.stage(ref_level, P->ref_level);
    std::memset(B.host(level_scale), 0, LLD_ORB_MAX_LEVELS * sizeof(float));
    std::memcpy(B.host(level_scale), P->level_scale, (size_t)P->n_levels * sizeof(float));
    int32_t* L = B.host(list);
    const int n = P->n_points;
    n_small = 0;
    for (int i = 0; i < n; ++i) { const int c = P->obs_start[i + 1] - P->obs_start[i]; if (c >= 1 && c <= 8) L[n_small++] = i; }
    n_wave = 0;
    for (int i = 0; i < n; ++i) { const int c = P->obs_start[i + 1] - P->obs_start[i]; if (c > 8) L[n_small + n_wave++] = i; }
  }
};

void launch_normals(hipStream_t sm, NormalArgs A, const int32_t* d_list, int n_small, int n_wave) {
  if (n_small) {
    A.list = d_list; A.n_list = n_small;
    hipLaunchKernelGGL(mc_normal<8>, dim3((n_small + kBlock / 8 - 1) / (kBlock / 8)), dim3(kBlock), 0, sm, A);
  }
  if (n_wave) {
    A.list = d_list + n_small; A.n_list = n_wave;
    hipLaunchKernelGGL(mc_normal<64>, dim3((n_wave + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, sm, A);
  }
}

inline int blocks_for(int n) { return (n + kBlock - 1) / kBlock; }
inline int capped_blocks(const lld_ctx* ctx, int n) { const int b = blocks_for(n), cap = ctx->n_cu * 8; return b < cap ? b : cap; }

// Binds the block to the context's staging: the pinned buffer holds the uploaded prefix and the downloaded outputs [0, host_bytes).
int bind_block(lld_ctx* ctx, UploadBlock& B, size_t host_bytes) {
  void* hb; int st = lld_ctx_pinned(ctx, host_bytes, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind(static_cast<char*>(hb), static_cast<char*>(db));
  return LLD_OK;
}

}  // namespace

extern "C" {

int lld_loop_correct(lld_ctx* ctx, const lld_loop_correct_in* in, lld_loop_correct_out* out) {
  if (!ctx || !in || !out) return LLD_ERR_INVALID;
  const lld_mapcorr_points* P = &in->points;
  const int n_kf = in->n_kf, n_conn = in->n_conn, n_ent = in->n_entries, n = P->n_points;
  if (n_kf < 1 || n_conn < 1 || n_ent < 0 || n < 0) return LLD_ERR_INVALID;
  if (!in->kf_tcw || !in->conn || !in->scw || !in->kf_start || (n_ent > 0 && !in->kf_point) || (n > 0 && !in->already)) return LLD_ERR_INVALID;
  if (!out->corrected_sim3 || !out->non_corrected_sim3 || !out->tiw_corrected || !out->ow_corrected || !out->scw_f32) return LLD_ERR_INVALID;
  if (n > 0 && (!out->pos || !out->corrected_by || !out->normal || !out->min_distance || !out->max_distance || !out->updated)) return LLD_ERR_INVALID;
  if (in->cur < 0 || in->cur >= n_conn) return LLD_ERR_INVALID;
  const bool too_many_kf = n_kf > LLD_MAPCORR_MAX_KF;
  if (n_conn > n_kf) return LLD_ERR_INVALID;                 // a slot would have to repeat
  std::vector<int32_t> rank((size_t)n_kf, INT_MAX);
  for (int r = 0; r < n_conn; ++r) {
    const int k = in->conn[r];
    if (k < 0 || k >= n_kf || rank[k] != INT_MAX) return LLD_ERR_INVALID;
    rank[k] = r;
  }
  if (in->kf_start[0] != 0 || in->kf_start[n_conn] != n_ent) return LLD_ERR_INVALID;
  for (int r = 0; r < n_conn; ++r) if (in->kf_start[r + 1] < in->kf_start[r]) return LLD_ERR_INVALID;
  for (int e = 0; e < n_ent; ++e) if (in->kf_point[e] < 0 || in->kf_point[e] >= n) return LLD_ERR_INVALID;
  if (!finite_all(in->kf_tcw, (size_t)n_kf * 12) || !sim3_ok(in->scw)) return LLD_ERR_INVALID;
  std::vector<uint8_t> listed((size_t)n, 0);                 // the rule reads the reference keyframe of a listed point only
  for (int e = 0; e < n_ent; ++e) listed[in->kf_point[e]] = 1;
  int st = check_points(P, n_kf, [&](int i) { return !listed[i] || P->bad[i] || in->already[i]; });
  if (st == LLD_ERR_INVALID) return st;
  if (too_many_kf || n_ent > LLD_MAPCORR_MAX_ENTRIES) return LLD_ERR_UNSUPPORTED;
  if (st) return st;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  UploadBlock B;
  const Span<float> u_tcw = B.take<float>((size_t)n_kf, 12);
  const Span<int32_t> u_conn = B.take<int32_t>((size_t)n_conn), u_rank = B.take<int32_t>((size_t)n_kf);
  const Span<double> u_scw = B.take<double>(8);
  const Span<int32_t> u_start = B.take<int32_t>((size_t)n_conn + 1), u_point = B.take<int32_t>((size_t)n_ent);
  const Span<uint8_t> u_already = B.take<uint8_t>((size_t)n);
  const Span<int32_t> u_owner = B.take<int32_t>((size_t)n);  // staged as "no owner": the upload is the initialisation
  PointSpans PS; PS.reserve(B, P);
  B.end_upload();
  const Span<double> r_corr = B.take<double>((size_t)n_conn, 8), r_non = B.take<double>((size_t)n_conn, 8);
  const Span<float> r_tiw = B.take<float>((size_t)n_conn, 12), r_ow = B.take<float>((size_t)n_conn, 3), r_scwf = B.take<float>((size_t)n_conn, 12);
  const Span<float> r_pos = B.take<float>((size_t)n, 3), r_nrm = B.take<float>((size_t)n, 3), r_min = B.take<float>((size_t)n), r_max = B.take<float>((size_t)n);
  const Span<int32_t> r_by = B.take<int32_t>((size_t)n);
  const Span<uint8_t> r_upd = B.take<uint8_t>((size_t)n);
  const size_t out_end = B.size;
  const Span<double> s_swi = B.take<double>((size_t)n_conn, 8);
  const Span<float> s_ow_old = B.take<float>((size_t)n_kf, 3), s_ow_new = B.take<float>((size_t)n_kf, 3);
  st = bind_block(ctx, B, out_end); if (st) return st;
  B.stage(u_tcw, in->kf_tcw); B.stage(u_conn, in->conn); B.stage(u_rank, rank.data()); B.stage(u_scw, in->scw);
  B.stage(u_start, in->kf_start); B.stage(u_point, in->kf_point); B.stage(u_already, in->already);
  B.stage(u_owner, (const int32_t*)nullptr, kNoOwner & 0xff);
  if (n) PS.stage(B, P);

  hipStream_t sm = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, sm));
  hipLaunchKernelGGL(mc_centres, dim3(blocks_for(n_kf)), dim3(kBlock), 0, sm, n_kf, B.dev(u_tcw), B.dev(s_ow_old));
  LoopPoseArgs LP;
  LP.n_conn = n_conn; LP.cur = in->cur; LP.conn = B.dev(u_conn); LP.tcw = B.dev(u_tcw); LP.scw = B.dev(u_scw);
  LP.corrected = B.dev(r_corr); LP.non_corrected = B.dev(r_non); LP.swi = B.dev(s_swi);
  LP.tiw = B.dev(r_tiw); LP.ow = B.dev(r_ow); LP.scw_f32 = B.dev(r_scwf); LP.ow_new = B.dev(s_ow_new);
  hipLaunchKernelGGL(mc_loop_poses, dim3(blocks_for(n_conn)), dim3(kBlock), 0, sm, LP);
  if (n) {
    if (n_ent)
      hipLaunchKernelGGL(mc_owner, dim3(blocks_for(n_ent)), dim3(kBlock), 0, sm, n_ent, n_conn, B.dev(u_start), B.dev(u_point), B.dev(PS.bad),
                         B.dev(u_already), B.dev(u_owner));
    hipLaunchKernelGGL(mc_points_loop, dim3(capped_blocks(ctx, n)), dim3(kBlock), 0, sm, n, n_conn, B.dev(u_owner), B.dev(r_non), B.dev(s_swi),
                       B.dev(PS.pos), B.dev(r_pos), B.dev(r_by), B.dev(r_upd));
    NormalArgs A;
    A.list = nullptr; A.n_list = 0; A.obs_start = B.dev(PS.obs_start); A.obs_kf = B.dev(PS.obs_kf);
    A.C = lld_nd::Centres{B.dev(s_ow_old), B.dev(s_ow_new), B.dev(u_rank)};
    A.pos = B.dev(r_pos); A.owner = B.dev(u_owner); A.n_conn = n_conn; A.bad = B.dev(PS.bad);
    A.ref_kf = B.dev(PS.ref_kf); A.ref_level = B.dev(PS.ref_level); A.level_scale = B.dev(PS.level_scale); A.n_levels = P->n_levels;
    A.O = lld_nd::Out{B.dev(r_nrm), B.dev(r_min), B.dev(r_max)}; A.upd = B.dev(r_upd);
    launch_normals(sm, A, B.dev(PS.list), PS.n_small, PS.n_wave);
  }
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(B.h + B.up_bytes, B.d + B.up_bytes, out_end - B.up_bytes, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));

  std::memcpy(out->corrected_sim3, B.host(r_corr), (size_t)n_conn * 64); std::memcpy(out->non_corrected_sim3, B.host(r_non), (size_t)n_conn * 64);
  std::memcpy(out->tiw_corrected, B.host(r_tiw), (size_t)n_conn * 48); std::memcpy(out->ow_corrected, B.host(r_ow), (size_t)n_conn * 12);
  std::memcpy(out->scw_f32, B.host(r_scwf), (size_t)n_conn * 48);
  const uint8_t* upd = B.host(r_upd);
  for (int i = 0; i < n; ++i) {              // an entry the rule leaves alone keeps what the caller passed in
    out->corrected_by[i] = B.host(r_by)[i];
    out->updated[i] = upd[i];
    if (upd[i] & LLD_MAPCORR_MOVED) std::memcpy(out->pos + 3 * (size_t)i, B.host(r_pos) + 3 * (size_t)i, 12);
    if (upd[i] & LLD_LANDMARK_NORMAL_DEPTH) {
      std::memcpy(out->normal + 3 * (size_t)i, B.host(r_nrm) + 3 * (size_t)i, 12);
      out->min_distance[i] = B.host(r_min)[i]; out->max_distance[i] = B.host(r_max)[i];
    }
  }
  return LLD_OK;
}

int lld_essential_graph_apply(lld_ctx* ctx, const lld_essential_graph_apply_in* in, lld_essential_graph_apply_out* out) {
  if (!ctx || !in || !out) return LLD_ERR_INVALID;
  const lld_mapcorr_points* P = &in->points;
  const int n_kf = in->n_kf, n = P->n_points;
  if (n_kf < 1 || n < 0) return LLD_ERR_INVALID;
  if (!in->sim3_before || !in->sim3_after || (n > 0 && !in->corr_kf) || !out->tiw || !out->ow) return LLD_ERR_INVALID;
  if (n > 0 && (!out->pos || !out->normal || !out->min_distance || !out->max_distance || !out->updated)) return LLD_ERR_INVALID;
  for (int k = 0; k < n_kf; ++k) if (!sim3_ok(in->sim3_before + 8 * (size_t)k) || !sim3_ok(in->sim3_after + 8 * (size_t)k)) return LLD_ERR_INVALID;
  int st = check_points(P, n_kf, [&](int i) { return P->bad[i] != 0; });
  if (st == LLD_ERR_INVALID) return st;
  for (int i = 0; i < n; ++i) if (!P->bad[i] && (in->corr_kf[i] < 0 || in->corr_kf[i] >= n_kf)) return LLD_ERR_INVALID;
  if (n_kf > LLD_MAPCORR_MAX_KF) return LLD_ERR_UNSUPPORTED;
  if (st) return st;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  UploadBlock B;
  const Span<double> u_before = B.take<double>((size_t)n_kf, 8), u_after = B.take<double>((size_t)n_kf, 8);
  const Span<int32_t> u_corr = B.take<int32_t>((size_t)n);
  PointSpans PS; PS.reserve(B, P);
  B.end_upload();
  const Span<float> r_tiw = B.take<float>((size_t)n_kf, 12), r_ow = B.take<float>((size_t)n_kf, 3);
  const Span<float> r_pos = B.take<float>((size_t)n, 3), r_nrm = B.take<float>((size_t)n, 3), r_min = B.take<float>((size_t)n), r_max = B.take<float>((size_t)n);
  const Span<uint8_t> r_upd = B.take<uint8_t>((size_t)n);
  const size_t out_end = B.size;
  const Span<double> s_swr = B.take<double>((size_t)n_kf, 8);
  st = bind_block(ctx, B, out_end); if (st) return st;
  B.stage(u_before, in->sim3_before); B.stage(u_after, in->sim3_after); B.stage(u_corr, in->corr_kf);
  if (n) PS.stage(B, P);

  hipStream_t sm = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, sm));
  GraphPoseArgs G; G.n_kf = n_kf; G.after = B.dev(u_after); G.swr = B.dev(s_swr); G.tiw = B.dev(r_tiw); G.ow = B.dev(r_ow);
  hipLaunchKernelGGL(mc_graph_poses, dim3(blocks_for(n_kf)), dim3(kBlock), 0, sm, G);
  if (n) {
    hipLaunchKernelGGL(mc_points_graph, dim3(capped_blocks(ctx, n)), dim3(kBlock), 0, sm, n, B.dev(PS.bad), B.dev(u_corr), B.dev(u_before),
                       B.dev(s_swr), B.dev(PS.pos), B.dev(r_pos), B.dev(r_upd));
    NormalArgs A;
    A.list = nullptr; A.n_list = 0; A.obs_start = B.dev(PS.obs_start); A.obs_kf = B.dev(PS.obs_kf);
    A.C = lld_nd::Centres{B.dev(r_ow), B.dev(r_ow), nullptr};                  // every SetPose has run (:1619): all centres new
    A.pos = B.dev(r_pos); A.owner = nullptr; A.n_conn = 0; A.bad = B.dev(PS.bad);
    A.ref_kf = B.dev(PS.ref_kf); A.ref_level = B.dev(PS.ref_level); A.level_scale = B.dev(PS.level_scale); A.n_levels = P->n_levels;
    A.O = lld_nd::Out{B.dev(r_nrm), B.dev(r_min), B.dev(r_max)}; A.upd = B.dev(r_upd);
    launch_normals(sm, A, B.dev(PS.list), PS.n_small, PS.n_wave);
  }
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(B.h + B.up_bytes, B.d + B.up_bytes, out_end - B.up_bytes, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));

  std::memcpy(out->tiw, B.host(r_tiw), (size_t)n_kf * 48); std::memcpy(out->ow, B.host(r_ow), (size_t)n_kf * 12);
  const uint8_t* upd = B.host(r_upd);
  for (int i = 0; i < n; ++i) {
    out->updated[i] = upd[i];
    if (upd[i] & LLD_MAPCORR_MOVED) std::memcpy(out->pos + 3 * (size_t)i, B.host(r_pos) + 3 * (size_t)i, 12);
    if (upd[i] & LLD_LANDMARK_NORMAL_DEPTH) {
      std::memcpy(out->normal + 3 * (size_t)i, B.host(r_nrm) + 3 * (size_t)i, 12);
      out->min_distance[i] = B.host(r_min)[i]; out->max_distance[i] = B.host(r_max)[i];
    }
  }
  return LLD_OK;
}

int lld_global_ba_apply(lld_ctx* ctx, const lld_global_ba_apply_in* in, lld_global_ba_apply_out* out) {
  if (!ctx || !in || !out) return LLD_ERR_INVALID;
  const int n_kf = in->n_kf, n_org = in->n_origins, n = in->n_points;
  if (n_kf < 1 || n_org < 0 || n < 0) return LLD_ERR_INVALID;
  if (!in->kf_tcw || !in->kf_in_gba || !in->kf_tcw_gba || !in->parent || (n_org > 0 && !in->origins)) return LLD_ERR_INVALID;
  if (n > 0 && (!in->pos || !in->bad || !in->in_gba || !in->pos_gba || !in->ref_kf)) return LLD_ERR_INVALID;
  if (!out->visited || !out->tcw_new || !out->tcw_before || !out->ow_new || (n > 0 && (!out->pos || !out->moved))) return LLD_ERR_INVALID;
  // the spanning tree: children lists from the parent links; every keyframe with a parent must hang below a root, or it sits on a cycle
  std::vector<int32_t> child_start((size_t)n_kf + 1, 0), child((size_t)n_kf), order;
  for (int k = 0; k < n_kf; ++k) {
    const int p = in->parent[k];
    if (p < -1 || p >= n_kf || p == k) return LLD_ERR_INVALID;
    if (p >= 0) child_start[p + 1]++;
  }
  for (int k = 0; k < n_kf; ++k) child_start[k + 1] += child_start[k];
  { std::vector<int32_t> fill(child_start.begin(), child_start.end() - 1);
    for (int k = 0; k < n_kf; ++k) if (in->parent[k] >= 0) child[fill[in->parent[k]]++] = k; }
  order.reserve((size_t)n_kf);
  for (int k = 0; k < n_kf; ++k) if (in->parent[k] < 0) order.push_back(k);
  for (size_t q = 0; q < order.size(); ++q)
    for (int c = child_start[order[q]]; c < child_start[order[q] + 1]; ++c) order.push_back(child[c]);
  if ((int)order.size() != n_kf) return LLD_ERR_INVALID;     // a cycle
  // the walk of :679-702 from the origins.  An origin is a root of the tree and optimised: the walk reads its mTcwGBA as it is.
  std::vector<uint8_t> visited((size_t)n_kf, 0);
  std::vector<int32_t> depth((size_t)n_kf, 0), queue;
  for (int q = 0; q < n_org; ++q) {
    const int k = in->origins[q];
    if (k < 0 || k >= n_kf || visited[k] || in->parent[k] != -1 || !in->kf_in_gba[k]) return LLD_ERR_INVALID;
    visited[k] = 1; queue.push_back(k);
  }
  int n_depths = 0;
  for (size_t q = 0; q < queue.size(); ++q) {
    const int k = queue[q];
    for (int c = child_start[k]; c < child_start[k + 1]; ++c) {
      const int ch = child[c];
      visited[ch] = 1; queue.push_back(ch);
      depth[ch] = in->kf_in_gba[ch] ? 0 : depth[k] + 1;      // links below the nearest optimised ancestor
      if (depth[ch] > n_depths) n_depths = depth[ch];
    }
  }
  for (int k = 0; k < n_kf; ++k) if (in->kf_in_gba[k] && !visited[k]) return LLD_ERR_INVALID;
  for (int k = 0; k < n_kf; ++k) {
    if (!finite_all(in->kf_tcw + 12 * (size_t)k, 12)) return LLD_ERR_INVALID;
    if (in->kf_in_gba[k] && !finite_all(in->kf_tcw_gba + 12 * (size_t)k, 12)) return LLD_ERR_INVALID;
  }
  for (int i = 0; i < n; ++i) if (!in->bad[i] && !in->in_gba[i] && (in->ref_kf[i] < 0 || in->ref_kf[i] >= n_kf)) return LLD_ERR_INVALID;
  if (n_kf > LLD_MAPCORR_MAX_KF || n > LLD_MAPCORR_MAX_POINTS) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  // the composed keyframes by depth: a counting sort, ascending slot inside a depth
  std::vector<int32_t> depth_start((size_t)n_depths + 1, 0), chain;
  for (int k = 0; k < n_kf; ++k) if (depth[k] > 0) depth_start[depth[k]]++;
  for (int d = 0; d < n_depths; ++d) depth_start[d + 1] += depth_start[d];
  chain.resize((size_t)depth_start[n_depths]);
  { std::vector<int32_t> fill(depth_start.begin(), depth_start.end());
    for (int k = 0; k < n_kf; ++k) if (depth[k] > 0) chain[fill[depth[k] - 1]++] = k; }

  UploadBlock B;
  const Span<float> u_tcw = B.take<float>((size_t)n_kf, 12);
  const Span<int32_t> u_parent = B.take<int32_t>((size_t)n_kf), u_dstart = B.take<int32_t>((size_t)n_depths + 1), u_chain = B.take<int32_t>(chain.size());
  const Span<uint8_t> u_visited = B.take<uint8_t>((size_t)n_kf);
  const Span<float> u_pos = B.take<float>((size_t)n, 3);     // one position per point travels: mPosGBA of an optimised point, mWorldPos of any other
  const Span<uint8_t> u_bad = B.take<uint8_t>((size_t)n), u_in_gba = B.take<uint8_t>((size_t)n);
  const Span<int32_t> u_ref = B.take<int32_t>((size_t)n);
  const Span<float> r_gba = B.take<float>((size_t)n_kf, 12);   // uploaded as mTcwGBA of the optimised keyframes, downloaded as tcw_new: last of the upload
  B.end_upload();
  const Span<float> r_ow = B.take<float>((size_t)n_kf, 3), r_pos = B.take<float>((size_t)n, 3);
  const Span<uint8_t> r_moved = B.take<uint8_t>((size_t)n);
  const size_t out_end = B.size;
  int st = bind_block(ctx, B, out_end); if (st) return st;
  B.stage(u_tcw, in->kf_tcw); B.stage(u_parent, in->parent); B.stage(u_dstart, depth_start.data()); B.stage(u_chain, chain.data());
  B.stage(u_visited, visited.data()); B.stage(u_bad, in->bad); B.stage(u_in_gba, in->in_gba);
  B.stage(u_ref, in->ref_kf);
  for (int i = 0; i < n; ++i) std::memcpy(B.host(u_pos) + 3 * (size_t)i, (in->in_gba[i] ? in->pos_gba : in->pos) + 3 * (size_t)i, 12);
  for (int k = 0; k < n_kf; ++k) {
    float* g = B.host(r_gba) + 12 * (size_t)k;
    if (in->kf_in_gba[k]) std::memcpy(g, in->kf_tcw_gba + 12 * (size_t)k, 48); else std::memset(g, 0, 48);
  }

  hipStream_t sm = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, sm));
  if (n_depths) {
    GbaChainArgs C; C.n_depths = n_depths; C.depth_start = B.dev(u_dstart); C.list = B.dev(u_chain); C.parent = B.dev(u_parent);
    C.tcw = B.dev(u_tcw); C.gba = B.dev(r_gba);
    hipLaunchKernelGGL(mc_gba_chain, dim3(1), dim3(kBlock), 0, sm, C);
  }
  hipLaunchKernelGGL(mc_gba_centres, dim3(blocks_for(n_kf)), dim3(kBlock), 0, sm, n_kf, B.dev(u_visited), B.dev(r_gba), B.dev(r_ow));
  if (n) {
    GbaPointArgs A;
    A.n = n; A.bad = B.dev(u_bad); A.in_gba = B.dev(u_in_gba); A.pos = B.dev(u_pos); A.ref_kf = B.dev(u_ref);
    A.visited = B.dev(u_visited); A.tcw = B.dev(u_tcw); A.gba = B.dev(r_gba); A.ow_new = B.dev(r_ow); A.pos_new = B.dev(r_pos); A.moved = B.dev(r_moved);
    hipLaunchKernelGGL(mc_points_gba, dim3(capped_blocks(ctx, n)), dim3(kBlock), 0, sm, A);
  }
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(B.h + r_gba.off, B.d + r_gba.off, out_end - r_gba.off, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));

  for (int k = 0; k < n_kf; ++k) {           // a keyframe the walk does not reach keeps what the caller passed in
    out->visited[k] = visited[k];
    if (!visited[k]) continue;
    std::memcpy(out->tcw_new + 12 * (size_t)k, B.host(r_gba) + 12 * (size_t)k, 48);
    std::memcpy(out->tcw_before + 12 * (size_t)k, in->kf_tcw + 12 * (size_t)k, 48);    // mTcwBefGBA = GetPose() (:699)
    std::memcpy(out->ow_new + 3 * (size_t)k, B.host(r_ow) + 3 * (size_t)k, 12);
  }
  for (int i = 0; i < n; ++i) {
    out->moved[i] = B.host(r_moved)[i];
    if (out->moved[i]) std::memcpy(out->pos + 3 * (size_t)i, B.host(r_pos) + 3 * (size_t)i, 12);
  }
  return LLD_OK;
}

}  // extern "C"
