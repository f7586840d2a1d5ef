// lld_new_points.hip — the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:287-451) for one keyframe against
// up to LLD_NEWPTS_MAX_PAIRS neighbours in one call: parallax test, linear triangulation or stereo un-projection, depth tests,
// reprojection gates, scale-consistency gate.  The rules restated, their quirks and the deviation (the closed-form stereo parallax
// cosine) are written out in include/lld_amd.h; tests/newpoints_ref.py restates them independently in numpy.
//
// The whole file is compiled without FMA contraction: every float operation is the one IEEE operation the restatement performs.
//
// Kernels (one call = one upload, these two kernels, one download; no atomics, no scratch):
//   np_match    one workgroup of 64 per run of up to 64 consecutive matches of ONE pair (the host lists the runs), one lane per
//               match.  The two keyframe records are copied to LDS once per workgroup and read from there (uniform addresses:
//               broadcasts; the level tables are indexed by octave in LDS, not in registers).  The host gathers the matched
//               keypoints into match-major arrays, so every per-match load is coalesced and no caller-supplied index is ever
//               dereferenced on the device.  The 4x4 Jacobi works on 32 doubles per lane in LDS, lane-interleaved (conflict free).
//   np_compact  one workgroup of 1024: an order-preserving scan over the statuses (ballot ranks inside a wavefront, 16 wavefront
//               totals through LDS) writes the exclusive rank of every match and new_match; the per-pair counts are differences of
//               ranks at the pair boundaries, so they and the compaction offsets cannot disagree.  Also copies pair_status.
// The baseline gate is one rule in one place: the host evaluates it per pair while it validates the pairs and uploads the flags.
#pragma clang fp contract(off)

#include <cmath>
#include <vector>

#include "lld_common.h"
#include "lld_device_math.h"
#include "lld_ransac.h"

namespace {

constexpr int kLanes = 64;                   // matches per np_match workgroup
constexpr int kJacDoubles = 32;              // per lane: A^T A (4x4) and its eigenvectors
constexpr int kScan = 1024;                  // threads of np_compact
constexpr int kKfWords = sizeof(lld_new_points_kf) / 4;
constexpr int kMatchWords = 13;              // floats gathered per match (below), the last one the two octaves

// match-major planes of the gathered input: plane q of match i is at in[q * N + i]
enum { P_X1, P_Y1, P_RX1, P_RY1, P_UR1, P_D1, P_X2, P_Y2, P_RX2, P_RY2, P_UR2, P_D2, P_OCT };

struct Dev {
  const lld_new_points_kf* kf1; const lld_new_points_kf* kf2;
  const int32_t* match_start; const int2* runs; const float* in; const uint8_t* skipped;
  uint8_t* status; uint8_t* source; float* x3d; uint8_t* pair_status; int32_t* n_new; int32_t* new_match; int32_t* total;
  int32_t* rank;
  int32_t N, n_pairs, monocular;
};

// Mat::dot of row r of Rcw with x: the double sum.
__device__ __forceinline__ double row_dot(const float* Rcw, int r, const float* x) {
  double s = (double)Rcw[3 * r] * (double)x[0];
  s += (double)Rcw[3 * r + 1] * (double)x[1];
  s += (double)Rcw[3 * r + 2] * (double)x[2];
  return s;
}

__host__ __device__ __forceinline__ double norm3(const float* v) {
  double s = (double)v[0] * (double)v[0];
  s += (double)v[1] * (double)v[1];
  s += (double)v[2] * (double)v[2];
#ifdef __HIP_DEVICE_COMPILE__
  return __dsqrt_rn(s);
#else
  return std::sqrt(s);
#endif
}

// Ow = -Rwc*tcw (src/KeyFrame.cc:85)
__host__ __device__ __forceinline__ void camera_center(const lld_new_points_kf* k, float* ow) {
  lld::rwc_mul(k->Rcw, k->tcw, ow);
#pragma unroll
  for (int i = 0; i < 3; ++i) ow[i] = -ow[i];
}

// The baseline gate (:245-262), evaluated once per pair on the host while it validates the pairs (IEEE division and square root
// on both sides; this file is compiled without contraction for the host too).  The kernels read the flag.
inline bool pair_skipped(const lld_new_points_kf* k1, const lld_new_points_kf* k2, int monocular) {
  float ow1[3], ow2[3];
  camera_center(k1, ow1);
  camera_center(k2, ow2);
  const float v[3] = {ow2[0] - ow1[0], ow2[1] - ow1[1], ow2[2] - ow1[2]};
  const float baseline = (float)norm3(v);
  if (!monocular) return baseline < k2->mb;
  const float ratio = baseline / k2->median_depth;
  return (double)ratio < 0.01;
}

// cos(2*atan2(mb/2, depth)) in closed form (the DEVIATION of include/lld_amd.h)
__device__ __forceinline__ float cos_stereo(float mb, float depth) {
  const float a = mb * 0.5f;                 // mb/2
  const double a2 = (double)a * (double)a, d2 = (double)depth * (double)depth;
  return (float)((d2 - a2) / (d2 + a2));
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:638-654); false when z > 0 fails
__device__ __forceinline__ bool unproject_stereo(const lld_new_points_kf* k, const float* ow, float invfx, float invfy, float u, float v,
                                                 float z, float* x3d) {
  if (!(z > 0.0f)) return false;
  const float c[3] = {(u - k->cx) * z * invfx, (v - k->cy) * z * invfy, z};
  lld::rwc_mul(k->Rcw, c, x3d);
#pragma unroll
  for (int i = 0; i < 3; ++i) x3d[i] = x3d[i] + ow[i];
  return true;
}

// One reprojection gate (:364-388 / :391-414); true when the error exceeds the bound.  mbf is keyframe 1's for both.
__device__ __forceinline__ bool reproj_fails(const lld_new_points_kf* k, const float* x3d, float z, float kx, float ky, float ur,
                                             bool stereo, float mbf, float sigma2) {
  const float x = (float)(row_dot(k->Rcw, 0, x3d) + (double)k->tcw[0]);
  const float y = (float)(row_dot(k->Rcw, 1, x3d) + (double)k->tcw[1]);
  const float invz = (float)(1.0 / (double)z);
  const float u = k->fx * x * invz + k->cx;
  const float v = k->fy * y * invz + k->cy;
  const float ex = u - kx, ey = v - ky;
  if (!stereo) return (double)(ex * ex + ey * ey) > 5.991 * (double)sigma2;
  const float u_r = u - mbf * invz;
  const float er = u_r - ur;
  return (double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sigma2;
}

// grid: the runs, block 64
__global__ __launch_bounds__(kLanes) void np_match(Dev d) {
  __shared__ double jac[kJacDoubles * kLanes];
  __shared__ lld_new_points_kf kfs[2];
  const int lane = threadIdx.x;
  const int2 run = d.runs[blockIdx.x];
  const int pair = run.x;
  {
    const uint32_t* s1 = reinterpret_cast<const uint32_t*>(d.kf1);
    const uint32_t* s2 = reinterpret_cast<const uint32_t*>(d.kf2 + pair);
    uint32_t* dst = reinterpret_cast<uint32_t*>(kfs);
    for (int q = lane; q < kKfWords; q += kLanes) { dst[q] = s1[q]; dst[kKfWords + q] = s2[q]; }
  }
  __syncthreads();
  const int i = run.y + lane;
  if (i >= d.match_start[pair + 1] || i >= d.N) return;
  const lld_new_points_kf* k1 = &kfs[0];
  const lld_new_points_kf* k2 = &kfs[1];
  float ow1[3], ow2[3];
  camera_center(k1, ow1);
  camera_center(k2, ow2);
  int status = LLD_NEWPTS_NEW, source = LLD_NEWPTS_SRC_TRIANGULATED;
  float x3d[3] = {0.0f, 0.0f, 0.0f};
  const size_t N = (size_t)d.N;
  do {
    if (d.skipped[pair]) { status = LLD_NEWPTS_PAIR_SKIPPED; break; }
    const float* in = d.in + i;
    const float kx1 = in[P_X1 * N], ky1 = in[P_Y1 * N], ur1 = in[P_UR1 * N], dp1 = in[P_D1 * N];
    const float kx2 = in[P_X2 * N], ky2 = in[P_Y2 * N], ur2 = in[P_UR2 * N], dp2 = in[P_D2 * N];
    const uint32_t oct = __float_as_uint(in[P_OCT * N]);
    const int oct1 = (int)(oct & 0xffu), oct2 = (int)((oct >> 8) & 0xffu);
    const bool st1 = ur1 >= 0.0f, st2 = ur2 >= 0.0f;                            // :294, :298
    const float invfx1 = __fdiv_rn(1.0f, k1->fx), invfy1 = __fdiv_rn(1.0f, k1->fy);
    const float invfx2 = __fdiv_rn(1.0f, k2->fx), invfy2 = __fdiv_rn(1.0f, k2->fy);
    const float xn1[3] = {(kx1 - k1->cx) * invfx1, (ky1 - k1->cy) * invfy1, 1.0f};   // :301-302
    const float xn2[3] = {(kx2 - k2->cx) * invfx2, (ky2 - k2->cy) * invfy2, 1.0f};
    float ray1[3], ray2[3];
    lld::rwc_mul(k1->Rcw, xn1, ray1);                                               // :304-305
    lld::rwc_mul(k2->Rcw, xn2, ray2);
    double dot = (double)ray1[0] * (double)ray2[0];
    dot += (double)ray1[1] * (double)ray2[1];
    dot += (double)ray1[2] * (double)ray2[2];
    const float cosRays = (float)(dot / (norm3(ray1) * norm3(ray2)));           // :306
    float cs1 = cosRays + 1.0f, cs2 = cs1;                                     // :308-310
    if (st1) cs1 = cos_stereo(k1->mb, dp1);                                    // :312-315
    else if (st2) cs2 = cos_stereo(k2->mb, dp2);
    const float cs = cs2 < cs1 ? cs2 : cs1;                                    // std::min (:317)
    if (cosRays < cs && cosRays > 0.0f && (st1 || st2 || (double)cosRays < 0.9998)) {   // :320
      float A[16];
#pragma unroll
      for (int j = 0; j < 4; ++j) {                                            // :323-327, Tcw = [Rcw | tcw]
        const float r10 = j < 3 ? k1->Rcw[j] : k1->tcw[0], r11 = j < 3 ? k1->Rcw[3 + j] : k1->tcw[1], r12 = j < 3 ? k1->Rcw[6 + j] : k1->tcw[2];
        const float r20 = j < 3 ? k2->Rcw[j] : k2->tcw[0], r21 = j < 3 ? k2->Rcw[3 + j] : k2->tcw[1], r22 = j < 3 ? k2->Rcw[6 + j] : k2->tcw[2];
        A[j] = xn1[0] * r12 - r10;
        A[4 + j] = xn1[1] * r12 - r11;
        A[8 + j] = xn2[0] * r22 - r20;
        A[12 + j] = xn2[1] * r22 - r21;
      }
      const SP B{jac + lane, kLanes}, V = B.at(16);
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < 4; ++k) s += (double)A[4 * k + a] * (double)A[4 * k + b];
          B[4 * a + b] = s;
          B[4 * b + a] = s;
        }
      jacobi(B, V, 4);
      int e = 0;                                                               // the smallest eigenvalue, the highest index on a tie
      for (int k = 1; k < 4; ++k)
        if (B[5 * k] <= B[5 * e]) e = k;
      int m = 0;                                                               // canonical sign
      for (int k = 1; k < 4; ++k)
        if (fabs(V[4 * k + e]) > fabs(V[4 * m + e])) m = k;
      const bool neg = V[4 * m + e] < 0.0;
      const double v0 = V[e], v1 = V[4 + e], v2 = V[8 + e], v3 = V[12 + e];
      const float x[4] = {(float)(neg ? -v0 : v0), (float)(neg ? -v1 : v1), (float)(neg ? -v2 : v2), (float)(neg ? -v3 : v3)};
      if (x[3] == 0.0f) { status = LLD_NEWPTS_W_ZERO; break; }                  // :334
      const double inv = 1.0 / (double)x[3];                                   // :338
      x3d[0] = (float)((double)x[0] * inv); x3d[1] = (float)((double)x[1] * inv); x3d[2] = (float)((double)x[2] * inv);
    } else if (st1 && cs1 < cs2) {                                             // :341-343
      source = LLD_NEWPTS_SRC_STEREO1;
      if (!unproject_stereo(k1, ow1, invfx1, invfy1, in[P_RX1 * N], in[P_RY1 * N], dp1, x3d)) { status = LLD_NEWPTS_NO_DEPTH; break; }
    } else if (st2 && cs2 < cs1) {                                             // :345-347
      source = LLD_NEWPTS_SRC_STEREO2;
      if (!unproject_stereo(k2, ow2, invfx2, invfy2, in[P_RX2 * N], in[P_RY2 * N], dp2, x3d)) { status = LLD_NEWPTS_NO_DEPTH; break; }
    } else {                                                                   // :349-350
      status = LLD_NEWPTS_LOW_PARALLAX;
      break;
    }
    const float z1 = (float)(row_dot(k1->Rcw, 2, x3d) + (double)k1->tcw[2]);    // :355-357
    if (z1 <= 0.0f) { status = LLD_NEWPTS_Z1; break; }
    const float z2 = (float)(row_dot(k2->Rcw, 2, x3d) + (double)k2->tcw[2]);    // :359-361
    if (z2 <= 0.0f) { status = LLD_NEWPTS_Z2; break; }
    if (reproj_fails(k1, x3d, z1, kx1, ky1, ur1, st1, k1->mbf, k1->level_sigma2[oct1])) { status = LLD_NEWPTS_REPROJ1; break; }
    if (reproj_fails(k2, x3d, z2, kx2, ky2, ur2, st2, k1->mbf, k2->level_sigma2[oct2])) { status = LLD_NEWPTS_REPROJ2; break; }
    const float n1[3] = {x3d[0] - ow1[0], x3d[1] - ow1[1], x3d[2] - ow1[2]};    // :417-421
    const float n2[3] = {x3d[0] - ow2[0], x3d[1] - ow2[1], x3d[2] - ow2[2]};
    const float dist1 = (float)norm3(n1), dist2 = (float)norm3(n2);
    if (dist1 == 0.0f || dist2 == 0.0f) { status = LLD_NEWPTS_DIST_ZERO; break; }   // :423
    const float ratioDist = __fdiv_rn(dist2, dist1);                            // :426-427
    const float ratioOctave = __fdiv_rn(k1->scale_factors[oct1], k2->scale_factors[oct2]);
    const float ratioFactor = 1.5f * k1->scale_factor;                          // :233
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) { status = LLD_NEWPTS_SCALE; break; }   // :431
  } while (false);
  const bool isnew = status == LLD_NEWPTS_NEW;
  d.status[i] = (uint8_t)status;
  d.source[i] = (uint8_t)source;
  d.x3d[3 * (size_t)i] = isnew ? x3d[0] : 0.0f; d.x3d[3 * (size_t)i + 1] = isnew ? x3d[1] : 0.0f; d.x3d[3 * (size_t)i + 2] = isnew ? x3d[2] : 0.0f;
}

// grid: 1, block 1024
__global__ __launch_bounds__(kScan) void np_compact(Dev d) {
  __shared__ int wsum[kScan / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int base = 0;
  for (int c = 0; c < d.N; c += kScan) {
    const int i = c + tid;
    const bool flag = i < d.N && d.status[i] == LLD_NEWPTS_NEW;
    const unsigned long long m = __ballot(flag);
    const int r = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < kScan / 64; ++q) { const int s = wsum[q]; off += q < w ? s : 0; tot += s; }
    if (i < d.N) d.rank[i] = base + off + r;
    if (flag) d.new_match[base + off + r] = i;
    base += tot;
    __syncthreads();
  }
  if (tid == 0) { d.rank[d.N] = base; *d.total = base; }
  __syncthreads();
  if (tid < d.n_pairs) {
    d.n_new[tid] = d.rank[d.match_start[tid + 1]] - d.rank[d.match_start[tid]];
    d.pair_status[tid] = d.skipped[tid];
  }
}

inline size_t al(size_t b) { return (b + 255) & ~size_t(255); }

inline bool finite_all(const float* v, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
  return true;
}

int check_kf(const lld_new_points_kf& k, bool is_kf1, bool monocular) {
  if (k.n_levels < 1 || k.n_levels > LLD_ORB_MAX_LEVELS) return LLD_ERR_INVALID;
  if (!finite_all(k.Rcw, 9) || !finite_all(k.tcw, 3) || !finite_all(&k.fx, 4) || !std::isfinite(k.mb)) return LLD_ERR_INVALID;
  if (!(k.fx > 0.0f) || !(k.fy > 0.0f)) return LLD_ERR_INVALID;
  if (is_kf1 && (!std::isfinite(k.mbf) || !std::isfinite(k.scale_factor))) return LLD_ERR_INVALID;
  if (!is_kf1 && monocular && !std::isfinite(k.median_depth)) return LLD_ERR_INVALID;
  return LLD_OK;
}

}  // namespace

extern "C" {

int lld_new_points_triangulate(lld_ctx* ctx, const lld_new_points_in* in, lld_new_points_out* out) {
  if (!ctx || !in || !out) return LLD_ERR_INVALID;
  const int32_t n_pairs = in->n_pairs, n1 = in->n_keys1;
  if (n_pairs < 1 || n1 < 0) return LLD_ERR_INVALID;
  if (n_pairs > LLD_NEWPTS_MAX_PAIRS) return LLD_ERR_UNSUPPORTED;
  if (!in->kf2 || !in->key_start || !in->match_start) return LLD_ERR_INVALID;
  if (in->monocular != 0 && in->monocular != 1) return LLD_ERR_INVALID;
  if (in->key_start[0] != 0 || in->match_start[0] != 0) return LLD_ERR_INVALID;
  for (int p = 0; p < n_pairs; ++p)
    if (in->key_start[p + 1] < in->key_start[p] || in->match_start[p + 1] < in->match_start[p]) return LLD_ERR_INVALID;
  const int32_t N = in->match_start[n_pairs];
  if (N > LLD_NEWPTS_MAX_MATCHES) return LLD_ERR_UNSUPPORTED;
  int st = check_kf(in->kf1, true, in->monocular != 0);
  for (int p = 0; p < n_pairs && !st; ++p) st = check_kf(in->kf2[p], false, in->monocular != 0);
  if (st) return st;
  if (N > 0 && (!in->matches || !in->keys1_xy || !in->ur1 || !in->depth1 || !in->octave1 || !in->keys2_xy || !in->ur2 || !in->depth2 ||
                !in->octave2))
    return LLD_ERR_INVALID;
  for (int p = 0; p < n_pairs; ++p) {
    const int32_t nk2 = in->key_start[p + 1] - in->key_start[p];
    for (int i = in->match_start[p]; i < in->match_start[p + 1]; ++i) {
      const int32_t a = in->matches[2 * (size_t)i], b = in->matches[2 * (size_t)i + 1];
      if (a < 0 || a >= n1 || b < 0 || b >= nk2) return LLD_ERR_INVALID;
      const int32_t o1 = in->octave1[a], o2 = in->octave2[in->key_start[p] + b];
      if (o1 < 0 || o1 >= in->kf1.n_levels || o2 < 0 || o2 >= in->kf2[p].n_levels) return LLD_ERR_INVALID;
    }
  }
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  std::vector<int2> runs;
  for (int p = 0; p < n_pairs; ++p)
    for (int i = in->match_start[p]; i < in->match_start[p + 1]; i += kLanes) runs.push_back(make_int2(p, i));

  size_t inb = 0, outb = 0;
  auto add_in = [&](size_t b) { const size_t o = inb; inb += al(b); return o; };
  auto add_out = [&](size_t b) { const size_t o = outb; outb += al(b); return o; };
  const size_t o_kf1 = add_in(sizeof(lld_new_points_kf)), o_kf2 = add_in(sizeof(lld_new_points_kf) * (size_t)n_pairs);
  const size_t o_ms = add_in((size_t)(n_pairs + 1) * 4), o_runs = add_in(runs.size() * sizeof(int2));
  const size_t o_in = add_in((size_t)kMatchWords * N * 4), o_skip = add_in((size_t)n_pairs);
  const size_t r_st = add_out((size_t)N), r_src = add_out((size_t)N), r_x = add_out((size_t)N * 12), r_ps = add_out((size_t)n_pairs);
  const size_t r_nn = add_out((size_t)n_pairs * 4), r_nm = add_out((size_t)N * 4), r_tot = add_out(4);
  const size_t rankb = al((size_t)(N + 1) * 4);
  void* hb; st = lld_ctx_pinned(ctx, inb + outb, &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, inb + outb + rankb + 256, &db); if (st) return st;
  char* h = (char*)hb; char* dv = (char*)db; char* h_out = h + inb; char* d_out = dv + inb;
  std::memcpy(h + o_kf1, &in->kf1, sizeof(lld_new_points_kf));
  std::memcpy(h + o_kf2, in->kf2, sizeof(lld_new_points_kf) * (size_t)n_pairs);
  std::memcpy(h + o_ms, in->match_start, (size_t)(n_pairs + 1) * 4);
  for (int p = 0; p < n_pairs; ++p) h[o_skip + p] = pair_skipped(&in->kf1, in->kf2 + p, in->monocular) ? 1 : 0;
  if (!runs.empty()) std::memcpy(h + o_runs, runs.data(), runs.size() * sizeof(int2));
  {
    float* g = reinterpret_cast<float*>(h + o_in);
    const float* raw1 = in->keys1_raw_xy ? in->keys1_raw_xy : in->keys1_xy;
    const float* raw2 = in->keys2_raw_xy ? in->keys2_raw_xy : in->keys2_xy;
    const size_t n = (size_t)N;
    for (int p = 0; p < n_pairs; ++p)
      for (int i = in->match_start[p]; i < in->match_start[p + 1]; ++i) {
        const size_t a = (size_t)in->matches[2 * (size_t)i], b = (size_t)in->key_start[p] + (size_t)in->matches[2 * (size_t)i + 1];
        g[P_X1 * n + i] = in->keys1_xy[2 * a]; g[P_Y1 * n + i] = in->keys1_xy[2 * a + 1];
        g[P_RX1 * n + i] = raw1[2 * a]; g[P_RY1 * n + i] = raw1[2 * a + 1];
        g[P_UR1 * n + i] = in->ur1[a]; g[P_D1 * n + i] = in->depth1[a];
        g[P_X2 * n + i] = in->keys2_xy[2 * b]; g[P_Y2 * n + i] = in->keys2_xy[2 * b + 1];
        g[P_RX2 * n + i] = raw2[2 * b]; g[P_RY2 * n + i] = raw2[2 * b + 1];
        g[P_UR2 * n + i] = in->ur2[b]; g[P_D2 * n + i] = in->depth2[b];
        const uint32_t oct = (uint32_t)in->octave1[a] | ((uint32_t)in->octave2[b] << 8);
        std::memcpy(&g[P_OCT * n + i], &oct, 4);
      }
  }
  Dev d;
  d.kf1 = reinterpret_cast<const lld_new_points_kf*>(dv + o_kf1); d.kf2 = reinterpret_cast<const lld_new_points_kf*>(dv + o_kf2);
  d.match_start = reinterpret_cast<const int32_t*>(dv + o_ms); d.runs = reinterpret_cast<const int2*>(dv + o_runs);
  d.in = reinterpret_cast<const float*>(dv + o_in); d.skipped = reinterpret_cast<const uint8_t*>(dv + o_skip);
  d.status = reinterpret_cast<uint8_t*>(d_out + r_st); d.source = reinterpret_cast<uint8_t*>(d_out + r_src);
  d.x3d = reinterpret_cast<float*>(d_out + r_x); d.pair_status = reinterpret_cast<uint8_t*>(d_out + r_ps);
  d.n_new = reinterpret_cast<int32_t*>(d_out + r_nn); d.new_match = reinterpret_cast<int32_t*>(d_out + r_nm);
  d.total = reinterpret_cast<int32_t*>(d_out + r_tot); d.rank = reinterpret_cast<int32_t*>(d_out + outb);
  d.N = N; d.n_pairs = n_pairs; d.monocular = in->monocular;
  hipStream_t sm = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(dv, h, inb, hipMemcpyHostToDevice, sm));
  if (!runs.empty()) hipLaunchKernelGGL(np_match, dim3((unsigned)runs.size()), dim3(kLanes), 0, sm, d);
  hipLaunchKernelGGL(np_compact, dim3(1), dim3(kScan), 0, sm, d);
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(h_out, d_out, outb, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  const int32_t total = *reinterpret_cast<const int32_t*>(h_out + r_tot);
  if (out->status && N) std::memcpy(out->status, h_out + r_st, (size_t)N);
  if (out->source && N) std::memcpy(out->source, h_out + r_src, (size_t)N);
  if (out->x3d && N) std::memcpy(out->x3d, h_out + r_x, (size_t)N * 12);
  if (out->pair_status) std::memcpy(out->pair_status, h_out + r_ps, (size_t)n_pairs);
  if (out->n_new) std::memcpy(out->n_new, h_out + r_nn, (size_t)n_pairs * 4);
  if (out->new_match && total > 0) std::memcpy(out->new_match, h_out + r_nm, (size_t)total * 4);
  out->n_new_total = total;
  return LLD_OK;
}

}  // extern "C"
