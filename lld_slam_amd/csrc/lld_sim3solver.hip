// lld_sim3solver.hip — ORB-SLAM2's Sim3Solver (src/Sim3Solver.cc) as a batch of independent solvers whose RANSAC state stays in
// HBM between iterate() calls.  The rules restated and the two deviations (one rand() stream per solver; the numerics OpenCV
// decides) are written out in include/lld_amd.h.
//
// The whole file is compiled without FMA contraction: every float / double operation is the one IEEE operation the restatement
// tests/sim3solver_ref.py performs, in its order, so that the two agree bit for bit (up to device libm's atan2 / sin / cos).
//
// Layout on the device (one handle):
//   x1[N_total], x2[N_total]  float4 (mvX3Dc1/2, (float)mvnMaxError1/2)      im[N_total] float4 (mvP1im1, mvP2im2)
//   i1[N_total]  int (mvnIndices1)
//   desc[n]      S3Desc: the solver's range, its RANSAC constants (SetRansacParameters, computed on the host), both K
//   st[n]        S3State: the rand() stream, mnIterations, mnBestInliers and the best hypothesis (R, t, s, T12)
//   res[n]       S3Res: the last iterate()'s outputs      flags[sum n1] uint8 vbInliers
//   per call     hypothesis slots [hyp_off[s], hyp_off[s+1]) of every solver (the host bound min(n, mRansacMaxIts))
// Kernels of one iterate call (no host trip between them):
//   s3_sample    one lane per solver: the window min(n, mRansacMaxIts - mnIterations) (0 when N < mRansacMinInliers), the stream
//                saved, 3 indices per hypothesis (RandomInt and the swap-with-back removal of vAvailableIndices)
//   s3_hyp       one lane per hypothesis, 64 per workgroup: Horn in registers, the 4x4 Jacobi lane-interleaved in LDS
//   s3_count     one wavefront per hypothesis: CheckInliers over N, count by ballot / popcount
//   s3_resolve   one workgroup per solver: iterate()'s order replayed (>= best, > min returns), the state and outputs, vbInliers
//                recomputed and scattered by mvnIndices1, the stream advanced by the draws actually made
#pragma clang fp contract(off)

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "lld_common.h"
#include "lld_ransac.h"

namespace {

constexpr int kHypLanes = 64;                // hypotheses per s3_hyp workgroup
constexpr int kJacDoubles = 32;              // per lane: N (4x4) and its eigenvectors (4x4)
constexpr int kThreads = 256;                // resolve workgroups

struct S3Desc {
  int32_t off, n, n1, fl_off;
  int32_t min_inliers, max_its, fix_scale, pad;
  float k1[4], k2[4];                        // fx, fy, cx, cy of pKF1 / pKF2
};

struct S3State {
  RansacStream rng;
  int32_t n_iter;                            // mnIterations
  int32_t best;                              // mnBestInliers
  int32_t window;                            // hypotheses drawn for this call
  int32_t run;                               // of which iterate() made (the rest is speculative)
  float best_R[9], best_t[3], best_s;        // mBestRotation / Translation / Scale
  float best_T12[12];                        // mBestT12 rows 0..2
};

struct S3Res {
  float T12[12], R[9], t[3], s;
  int32_t has_pose, n_inliers, no_more, iterations, best_inliers, pad[3];
};

struct S3Hyp {
  float T12[12], T21[12];                    // rows 0..2 of mT12i / mT21i
  float R[9], t[3], s;                       // mR12i, mt12i, ms12i
  int32_t n_inliers, record, idx[3];
};

// ------------------------------------------------------------------ float products summed in double (DEVIATION 2)
__device__ __host__ inline float dot3f(float a0, float a1, float a2, float b0, float b1, float b2) {
  double s = (double)a0 * (double)b0;
  s += (double)a1 * (double)b1;
  s += (double)a2 * (double)b2;
  return (float)s;
}

// Project (:380-400) with T = [R | t] row-major 3x4: P3Dc = R*X + t, then FromCameraToImage's float steps.
__device__ __host__ inline void project(const float* T, float X, float Y, float Z, const float* k, float& u, float& v) {
  const float xc = dot3f(T[0], T[1], T[2], X, Y, Z) + T[3];
  const float yc = dot3f(T[4], T[5], T[6], X, Y, Z) + T[7];
  const float zc = dot3f(T[8], T[9], T[10], X, Y, Z) + T[11];
  const float invz = 1.0f / zc;
  const float x = xc * invz;
  const float y = yc * invz;
  u = k[0] * x + k[2];
  v = k[1] * y + k[3];
}

// CheckInliers (:340-364) for one correspondence: X3Dc2 through T12 into K1, X3Dc1 through T21 into K2, both errors below their
// (float of size_t) thresholds.
__device__ inline bool is_inlier(const float* T12, const float* T21, float4 x1, float4 x2, float4 im, const float* k1,
                                 const float* k2) {
  float u21, v21, u12, v12;
  project(T12, x2.x, x2.y, x2.z, k1, u21, v21);
  project(T21, x1.x, x1.y, x1.z, k2, u12, v12);
  const float d1x = im.x - u21, d1y = im.y - v21;
  const float d2x = u12 - im.z, d2y = v12 - im.w;
  double e1 = (double)d1x * (double)d1x; e1 += (double)d1y * (double)d1y;
  double e2 = (double)d2x * (double)d2x; e2 += (double)d2y * (double)d2y;
  return (float)e1 < x1.w && (float)e2 < x2.w;
}

// ComputeSim3 (:226-337) on the 3 sampled points; P1[r][i] = coordinate r of point i.  jac: 32 doubles of LDS for the Jacobi.
__device__ void horn(const float P1[3][3], const float P2[3][3], bool fix_scale, SP jac, S3Hyp& h) {
  float O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {              // ComputeCentroid: cv::reduce(SUM), C / P.cols
    O1[r] = ((P1[r][0] + P1[r][1]) + P1[r][2]) / 3.0f;
    O2[r] = ((P2[r][0] + P2[r][1]) + P2[r][2]) / 3.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) { Pr1[r][i] = P1[r][i] - O1[r]; Pr2[r][i] = P2[r][i] - O2[r]; }
  }
  float M[3][3];                             // M = Pr2 * Pr1^T
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = dot3f(Pr2[i][0], Pr2[i][1], Pr2[i][2], Pr1[j][0], Pr1[j][1], Pr1[j][2]);
  // the N entries: float arithmetic on M's floats, held in double, stored into a float 4x4
  const float N11 = M[0][0] + M[1][1] + M[2][2];
  const float N12 = M[1][2] - M[2][1];
  const float N13 = M[2][0] - M[0][2];
  const float N14 = M[0][1] - M[1][0];
  const float N22 = M[0][0] - M[1][1] - M[2][2];
  const float N23 = M[0][1] + M[1][0];
  const float N24 = M[2][0] + M[0][2];
  const float N33 = -M[0][0] + M[1][1] - M[2][2];
  const float N34 = M[1][2] + M[2][1];
  const float N44 = -M[0][0] - M[1][1] + M[2][2];
  const float Nm[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
  SP A = jac, V = jac.at(16);
#pragma unroll
  for (int q = 0; q < 16; ++q) A[q] = (double)Nm[q];
  jacobi(A, V, 4);                           // cv::eigen: the largest eigenvalue, the lowest index on a tie
  int e = 0;
  for (int k = 1; k < 4; ++k)
    if (A[5 * k] > A[5 * e]) e = k;
  int m = 0;                                 // canonical sign
  for (int k = 1; k < 4; ++k)
    if (fabs(V[4 * k + e]) > fabs(V[4 * m + e])) m = k;
  const bool neg = V[4 * m + e] < 0.0;
  float q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = (float)(neg ? -V[4 * k + e] : V[4 * k + e]);
  // angle-axis: ang = atan2(norm(vec), w); vec = 2*ang*vec/norm(vec)
  double nv = (double)q[1] * (double)q[1];
  nv += (double)q[2] * (double)q[2];
  nv += (double)q[3] * (double)q[3];
  nv = sqrt(nv);
  const double ang = atan2(nv, (double)q[0]);
  const double alpha = (2.0 * ang) / nv;
  float vec[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) vec[k] = (float)((double)q[k + 1] * alpha);
  // Rodrigues
  double th = (double)vec[0] * (double)vec[0];
  th += (double)vec[1] * (double)vec[1];
  th += (double)vec[2] * (double)vec[2];
  th = sqrt(th);
  float R[3][3];
  if (th < DBL_EPSILON) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0f : 0.0f;
  } else {
    const double r[3] = {(double)vec[0] / th, (double)vec[1] / th, (double)vec[2] / th};
    const double c = cos(th), sn = sin(th), c1 = 1.0 - c;
    const double K[3][3] = {{0.0, -r[2], r[1]}, {r[2], 0.0, -r[0]}, {-r[1], r[0], 0.0}};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i][j] = (float)((c * (i == j ? 1.0 : 0.0) + c1 * (r[i] * r[j])) + sn * K[i][j]);
  }
  float P3[3][3];                            // P3 = R * Pr2
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) P3[i][j] = dot3f(R[i][0], R[i][1], R[i][2], Pr2[0][j], Pr2[1][j], Pr2[2][j]);
  float s = 1.0f;
  if (!fix_scale) {                          // nom = Pr1.dot(P3), den = sum of pow(P3, 2), both row-major in double
    double nom = (double)Pr1[0][0] * (double)P3[0][0];
    double den = (double)(P3[0][0] * P3[0][0]);
#pragma unroll
    for (int q9 = 1; q9 < 9; ++q9) {
      nom += (double)Pr1[q9 / 3][q9 % 3] * (double)P3[q9 / 3][q9 % 3];
      den += (double)(P3[q9 / 3][q9 % 3] * P3[q9 / 3][q9 % 3]);
    }
    s = (float)(nom / den);
  }
  // t = O1 - (s*R)*O2; T12 = [sR | t]; T21 = [(1/s) R^T | -((1/s) R^T) t]
  float sR[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) sR[i][j] = s * R[i][j];
  float t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = O1[i] - dot3f(sR[i][0], sR[i][1], sR[i][2], O2[0], O2[1], O2[2]);
  const double inv = 1.0 / (double)s;
  float sRi[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) sRi[i][j] = (float)(inv * (double)R[j][i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      h.T12[4 * i + j] = sR[i][j];
      h.T21[4 * i + j] = sRi[i][j];
      h.R[3 * i + j] = R[i][j];
    }
    h.T12[4 * i + 3] = t[i];
    h.T21[4 * i + 3] = -dot3f(sRi[i][0], sRi[i][1], sRi[i][2], t[0], t[1], t[2]);
    h.t[i] = t[i];
  }
  h.s = s;
}

struct Dev {
  const float4* x1; const float4* x2; const float4* im; const int32_t* i1;
  const S3Desc* desc; S3State* st; S3Res* res; uint8_t* flags;
  const int32_t* hyp_off;                    // [n + 1] this call's hypothesis slots (bounds; 0 for inactive solvers)
  S3Hyp* hyp;                                // [slots]
  int n, n_iterations;
};

// ------------------------------------------------------------------ kernels
__global__ void s3_sample(Dev d) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n) return;
  const int bound = d.hyp_off[s + 1] - d.hyp_off[s];
  if (bound == 0) return;                    // not active in this call
  const S3Desc ds = d.desc[s];
  S3State& st = d.st[s];
  // iterate (:140-207): N < mRansacMinInliers -> bNoMore with no draws; else the loop runs while mnIterations < budget AND
  // fewer than n this call, i.e. min(n, budget - mnIterations) iterations unless a pose is returned first.
  const int n_it = d.n_iterations > 0 ? d.n_iterations : ds.max_its;   // 0: find(), iterate(mRansacMaxIts)
  int W = ds.n < ds.min_inliers ? 0 : max(0, min(n_it, ds.max_its - st.n_iter));
  if (W > bound) W = bound;                  // cannot happen: bound = min(n_it, mRansacMaxIts)
  st.window = W;
  st.rng.save();                             // ring is advanced in place; s3_resolve rewinds it to the saved one + the draws made
  int32_t head = st.rng.head;
  S3Hyp* out = d.hyp + d.hyp_off[s];
  for (int k = 0; k < W; ++k) draw_set<3>(st.rng.ring, head, ds.n, out[k].idx);
}

// ComputeSim3 on one hypothesis per lane.
__global__ __launch_bounds__(kHypLanes) void s3_hyp(Dev d, int n_slots) {
  __shared__ double lds[kJacDoubles * kHypLanes];
  const int g = blockIdx.x * kHypLanes + threadIdx.x;
  if (g >= n_slots) return;
  const int s = solver_of(d.hyp_off, d.n, g);
  if (g - d.hyp_off[s] >= d.st[s].window) return;
  const S3Desc ds = d.desc[s];
  S3Hyp& h = d.hyp[g];
  float P1[3][3], P2[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {              // mvX3Dc1[idx].copyTo(P3Dc1i.col(i))
    const int c = ds.off + h.idx[i];
    const float4 a = d.x1[c], b = d.x2[c];
    P1[0][i] = a.x; P1[1][i] = a.y; P1[2][i] = a.z;
    P2[0][i] = b.x; P2[1][i] = b.y; P2[2][i] = b.z;
  }
  horn(P1, P2, ds.fix_scale != 0, SP{lds + threadIdx.x, kHypLanes}, h);
  h.record = 0;
}

__global__ __launch_bounds__(256) void s3_count(Dev d, int n_slots) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_slots) return;
  const int s = solver_of(d.hyp_off, d.n, g);
  if (g - d.hyp_off[s] >= d.st[s].window) return;
  const S3Desc ds = d.desc[s];
  float T12[12], T21[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) { T12[q] = d.hyp[g].T12[q]; T21[q] = d.hyp[g].T21[q]; }
  const int cnt = wave_count(ds.n, [&](int i) {
    return is_inlier(T12, T21, d.x1[ds.off + i], d.x2[ds.off + i], d.im[ds.off + i], ds.k1, ds.k2);
  });
  if ((threadIdx.x & 63) == 0) d.hyp[g].n_inliers = cnt;
}

__global__ __launch_bounds__(kThreads) void s3_resolve(Dev d) {
  const int s = blockIdx.x;
  const int h0 = d.hyp_off[s];
  if (d.hyp_off[s + 1] == h0) return;        // not active
  __shared__ float T_sh[24];                 // the returned hypothesis's T12 / T21
  __shared__ int has_sh;
  const S3Desc ds = d.desc[s];
  S3State& st = d.st[s];
  S3Res& res = d.res[s];
  const int tid = threadIdx.x;
  if (tid == 0) {
    int has = 0, run = st.window, n_in = 0;
    for (int k = 0; k < st.window; ++k) {
      S3Hyp& h = d.hyp[h0 + k];
      if (h.n_inliers < st.best) continue;
      h.record = 1;                          // mvbBestInliers, mnBestInliers, mBestT12 / Rotation / Translation / Scale
      st.best = h.n_inliers;
      for (int q = 0; q < 12; ++q) st.best_T12[q] = h.T12[q];
      for (int q = 0; q < 9; ++q) st.best_R[q] = h.R[q];
      for (int q = 0; q < 3; ++q) st.best_t[q] = h.t[q];
      st.best_s = h.s;
      if (h.n_inliers > ds.min_inliers) {
        has = 1; run = k + 1; n_in = h.n_inliers;
        for (int q = 0; q < 12; ++q) { T_sh[q] = h.T12[q]; T_sh[12 + q] = h.T21[q]; }
        break;
      }
    }
    st.run = run;
    st.n_iter += run;
    int no_more = 0;
    if (ds.n < ds.min_inliers) no_more = 1;
    else if (!has && st.n_iter >= ds.max_its) no_more = 1;
    res.has_pose = has;
    res.n_inliers = n_in;
    res.no_more = no_more;
    res.iterations = st.n_iter;
    res.best_inliers = st.best;
    for (int q = 0; q < 12; ++q) res.T12[q] = has ? st.best_T12[q] : 0.0f;
    for (int q = 0; q < 9; ++q) res.R[q] = st.best_R[q];
    for (int q = 0; q < 3; ++q) res.t[q] = st.best_t[q];
    res.s = st.best_s;
    has_sh = has;
    st.rng.rewind(3 * run);                  // the stream after the draws made: 3 per iteration run
  }
  __syncthreads();
  float T12[12], T21[12];                    // read only when a pose is returned
  for (int q = 0; q < 12; ++q) { T12[q] = T_sh[q]; T21[q] = T_sh[12 + q]; }
  scatter_inliers<kThreads>(d.flags + ds.fl_off, ds.n1, has_sh != 0, d.i1 + ds.off, ds.n, [&](int i) {
    return is_inlier(T12, T21, d.x1[ds.off + i], d.x2[ds.off + i], d.im[ds.off + i], ds.k1, ds.k2);
  });
}

}  // namespace

// ------------------------------------------------------------------ host side
struct lld_sim3solver_batch {
  lld_ctx* ctx = nullptr;
  int n = 0;
  std::vector<S3Desc> desc;
  int64_t n1_total = 0;
  void* dmem = nullptr;                      // points, descriptors, state, results, flags
  void* dcall = nullptr; size_t dcall_bytes = 0;
  Dev dev{};
  std::vector<int32_t> last_off;             // the last call's hyp_off (host copy)
};

extern "C" void lld_sim3solver_params_default(lld_sim3solver_params* p) {
  if (!p) return;
  p->probability = 0.99; p->min_inliers = 20; p->max_iterations = 300;
}

static int s3_check_problem(const lld_sim3solver_problem& q) {
  if (q.n < 0 || q.n1 < 0) return LLD_ERR_INVALID;
  if (q.n > LLD_SIM3S_MAX_CORRESPONDENCES || q.n1 > LLD_SIM3S_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  if (q.n > 0 && (!q.xyz1 || !q.xyz2 || !q.sigma2_1 || !q.sigma2_2 || !q.index1)) return LLD_ERR_INVALID;
  if (!(q.fx1 > 0.0f) || !(q.fy1 > 0.0f) || !(q.fx2 > 0.0f) || !(q.fy2 > 0.0f)) return LLD_ERR_INVALID;
  if (!indices_unique_in_range(q.index1, q.n, q.n1)) return LLD_ERR_INVALID;
  for (int i = 0; i < q.n; ++i)
    for (float s2 : {q.sigma2_1[i], q.sigma2_2[i]})
      if (!(s2 >= 0.0f) || !(9.210 * s2 < 4294967296.0)) return LLD_ERR_INVALID;   // NaN and inf fail too
  return LLD_OK;
}

static int s3_check_params(const lld_sim3solver_params& p) {
  if (p.min_inliers < 3) return LLD_ERR_UNSUPPORTED;
  if (p.max_iterations < 1 || p.max_iterations > LLD_SIM3S_MAX_ITERATIONS) return LLD_ERR_INVALID;
  if (!(p.probability > 0.0 && p.probability < 1.0)) return LLD_ERR_INVALID;
  return LLD_OK;
}

// The constructor's per-correspondence values (:64-109): camera points, FromCameraToImage, the size_t thresholds.
static void s3_camera_point(const float* R, const float* t, const float* X, float* Xc) {
  for (int r = 0; r < 3; ++r) Xc[r] = dot3f(R[3 * r], R[3 * r + 1], R[3 * r + 2], X[0], X[1], X[2]) + t[r];
}

static void s3_to_image(const float* Xc, float fx, float fy, float cx, float cy, float* uv) {
  const float invz = 1.0f / Xc[2];
  const float x = Xc[0] * invz;
  const float y = Xc[1] * invz;
  uv[0] = fx * x + cx;
  uv[1] = fy * y + cy;
}

static float s3_max_error(float sigma2) {
  const size_t e = (size_t)(9.210 * (double)sigma2);   // std::vector<size_t>::push_back(9.210*sigmaSquare)
  return (float)e;
}

static int s3_upload(lld_sim3solver_batch* b, const lld_sim3solver_problem* problems, std::vector<S3State>& st, int64_t ntot);

extern "C" int lld_sim3solver_batch_create(lld_ctx* ctx, int32_t n, const lld_sim3solver_problem* problems,
                                           const lld_sim3solver_params* params, lld_sim3solver_batch** out) {
  if (!ctx || !problems || !params || !out || n < 1) return LLD_ERR_INVALID;
  *out = nullptr;
  if (n > LLD_SIM3S_MAX_SOLVERS) return LLD_ERR_UNSUPPORTED;
  if (int st = s3_check_params(*params)) return st;
  for (int s = 0; s < n; ++s)
    if (int st = s3_check_problem(problems[s])) return st;
  auto* b = new lld_sim3solver_batch();
  b->ctx = ctx; b->n = n;
  b->desc.resize(n);
  int64_t ntot = 0;
  std::vector<S3State> st(n);
  for (int s = 0; s < n; ++s) {
    const lld_sim3solver_problem& q = problems[s];
    S3Desc& ds = b->desc[s];
    std::memset(&ds, 0, sizeof(ds));
    ds.off = (int32_t)ntot; ds.n = q.n; ds.n1 = q.n1; ds.fl_off = (int32_t)b->n1_total;
    ds.fix_scale = q.fix_scale != 0;
    ds.k1[0] = q.fx1; ds.k1[1] = q.fy1; ds.k1[2] = q.cx1; ds.k1[3] = q.cy1;
    ds.k2[0] = q.fx2; ds.k2[1] = q.fy2; ds.k2[2] = q.cx2; ds.k2[3] = q.cy2;
    // SetRansacParameters (:114-138), literally
    const int N = q.n;
    const int minInliers = params->min_inliers;
    const float epsilon = (float)minInliers / N;                  // N = 0: inf
    ds.min_inliers = minInliers;
    ds.max_its = ransac_max_iterations(params->probability, epsilon, minInliers, N, params->max_iterations);
    std::memset(&st[s], 0, sizeof(S3State));
    srand_state(q.seed, st[s].rng.ring, &st[s].rng.head);
    ntot += N;
    b->n1_total += q.n1;
  }
  if (int rc = s3_upload(b, problems, st, ntot)) {   // nothing half-built survives a failure
    lld_sim3solver_batch_destroy(b);
    return rc;
  }
  *out = b;
  return LLD_OK;
}

static int s3_upload(lld_sim3solver_batch* b, const lld_sim3solver_problem* problems, std::vector<S3State>& st, int64_t ntot) {
  lld_ctx* ctx = b->ctx;
  const int n = b->n;
  const int64_t nt = std::max<int64_t>(ntot, 1);
  std::vector<float4> x1(nt), x2(nt), im(nt);
  std::vector<int32_t> i1(nt);
  for (int s = 0; s < n; ++s) {
    const lld_sim3solver_problem& q = problems[s];
    const int64_t o = b->desc[s].off;
    for (int i = 0; i < q.n; ++i) {
      float c1[3], c2[3], p1[2], p2[2];
      s3_camera_point(q.Rcw1, q.tcw1, q.xyz1 + 3 * i, c1);
      s3_camera_point(q.Rcw2, q.tcw2, q.xyz2 + 3 * i, c2);
      s3_to_image(c1, q.fx1, q.fy1, q.cx1, q.cy1, p1);
      s3_to_image(c2, q.fx2, q.fy2, q.cx2, q.cy2, p2);
      x1[o + i] = make_float4(c1[0], c1[1], c1[2], s3_max_error(q.sigma2_1[i]));
      x2[o + i] = make_float4(c2[0], c2[1], c2[2], s3_max_error(q.sigma2_2[i]));
      im[o + i] = make_float4(p1[0], p1[1], p2[0], p2[1]);
      i1[o + i] = q.index1[i];
    }
  }
  const int64_t nfl = std::max<int64_t>(b->n1_total, 1);
  size_t bytes = 3 * lld_slab::pad(sizeof(float4) * nt) + lld_slab::pad(sizeof(int32_t) * nt) + lld_slab::pad(sizeof(S3Desc) * n) +
                 lld_slab::pad(sizeof(S3State) * n) + lld_slab::pad(sizeof(S3Res) * n) + lld_slab::pad(nfl);
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&b->dmem, bytes) != hipSuccess) { b->dmem = nullptr; return LLD_ERR_ALLOC; }
  lld_slab sl; sl.base = (char*)b->dmem; sl.size = bytes;
  Dev& d = b->dev;
  d.x1 = sl.take<float4>(nt);
  d.x2 = sl.take<float4>(nt);
  d.im = sl.take<float4>(nt);
  d.i1 = sl.take<int32_t>(nt);
  d.desc = sl.take<S3Desc>(n);
  d.st = sl.take<S3State>(n);
  d.res = sl.take<S3Res>(n);
  d.flags = sl.take<uint8_t>(nfl);
  d.n = n;
  hipStream_t stream = ctx->stream;
  std::vector<S3Res> res(n);
  std::memset(res.data(), 0, sizeof(S3Res) * n);
  LLD_HIP_TRY(hipMemcpyAsync((void*)d.x1, x1.data(), sizeof(float4) * nt, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemcpyAsync((void*)d.x2, x2.data(), sizeof(float4) * nt, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemcpyAsync((void*)d.im, im.data(), sizeof(float4) * nt, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemcpyAsync((void*)d.i1, i1.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemcpyAsync((void*)d.desc, b->desc.data(), sizeof(S3Desc) * n, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemcpyAsync(d.st, st.data(), sizeof(S3State) * n, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemcpyAsync(d.res, res.data(), sizeof(S3Res) * n, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemsetAsync(d.flags, 0, nfl, stream));
  LLD_HIP_TRY(hipStreamSynchronize(stream));
  return LLD_OK;
}

extern "C" void lld_sim3solver_batch_destroy(lld_sim3solver_batch* b) {
  if (!b) return;
  if (b->ctx) (void)hipSetDevice(b->ctx->device);
  if (b->dmem) (void)hipFree(b->dmem);
  if (b->dcall) (void)hipFree(b->dcall);
  delete b;
}

// iterate(n_iterations) on the active solvers; n_iterations = 0: each solver's own mRansacMaxIts (find()).
static int s3_iterate(lld_sim3solver_batch* b, int32_t n_iterations, const uint8_t* active) {
  LLD_HIP_TRY(hipSetDevice(b->ctx->device));
  const int n = b->n;
  const std::vector<int32_t> off = ransac_call_offsets(n, active, [&](int s) {
    const int its = b->desc[s].max_its;
    return n_iterations > 0 ? std::min(n_iterations, its) : its;
  });
  const int slots = off[n];
  // the previous call's hypotheses stay readable only until this call touches the per-call buffers
  b->last_off.clear();
  size_t need = lld_slab::pad(sizeof(int32_t) * (n + 1)) + lld_slab::pad(sizeof(S3Hyp) * (size_t)std::max(slots, 1));
  if (int rc = lld_grow_device(&b->dcall, &b->dcall_bytes, need)) {
    if (rc == LLD_ERR_ALLOC) b->dev.hyp_off = nullptr;
    return rc;
  }
  lld_slab sl; sl.base = (char*)b->dcall; sl.size = need;
  Dev d = b->dev;
  int32_t* hoff = sl.take<int32_t>(n + 1);
  d.hyp_off = hoff;
  d.hyp = sl.take<S3Hyp>((size_t)std::max(slots, 1));
  d.n_iterations = n_iterations;
  b->dev = d;
  hipStream_t stream = b->ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(hoff, off.data(), sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice, stream));
  s3_sample<<<(n + 63) / 64, 64, 0, stream>>>(d);
  if (slots > 0) {
    s3_hyp<<<(slots + kHypLanes - 1) / kHypLanes, kHypLanes, 0, stream>>>(d, slots);
    s3_count<<<(slots + 3) / 4, 256, 0, stream>>>(d, slots);
  }
  s3_resolve<<<n, kThreads, 0, stream>>>(d);
  LLD_HIP_TRY(hipGetLastError());
  b->last_off = off;
  return LLD_OK;
}

extern "C" int lld_sim3solver_batch_iterate(lld_sim3solver_batch* b, int32_t n_iterations, const uint8_t* active) {
  if (!b) return LLD_ERR_INVALID;
  if (n_iterations < 1) return LLD_ERR_INVALID;
  if (n_iterations > LLD_SIM3S_MAX_ITERATIONS) return LLD_ERR_UNSUPPORTED;
  return s3_iterate(b, n_iterations, active);
}

extern "C" int lld_sim3solver_batch_find(lld_sim3solver_batch* b, const uint8_t* active) {
  if (!b) return LLD_ERR_INVALID;
  return s3_iterate(b, 0, active);
}

extern "C" int lld_sim3solver_batch_download(lld_sim3solver_batch* b, lld_sim3solver_result* outs) {
  if (!b || !outs) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t stream = b->ctx->stream;
  std::vector<S3Res> res(b->n);
  std::vector<uint8_t> flags(std::max<int64_t>(b->n1_total, 1));
  LLD_HIP_TRY(hipMemcpyAsync(res.data(), b->dev.res, sizeof(S3Res) * b->n, hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipMemcpyAsync(flags.data(), b->dev.flags, flags.size(), hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipStreamSynchronize(stream));
  for (int s = 0; s < b->n; ++s) {
    lld_sim3solver_result& o = outs[s];
    const S3Res& r = res[s];
    for (int q = 0; q < 12; ++q) o.T12[q] = r.T12[q];
    for (int q = 0; q < 9; ++q) o.R[q] = r.R[q];
    for (int q = 0; q < 3; ++q) o.t[q] = r.t[q];
    o.s = r.s;
    o.has_pose = r.has_pose; o.n_inliers = r.n_inliers; o.no_more = r.no_more; o.iterations = r.iterations;
    o.best_inliers = r.best_inliers; o.n1 = b->desc[s].n1;
    if (o.inlier) std::memcpy(o.inlier, flags.data() + b->desc[s].fl_off, b->desc[s].n1);
  }
  return LLD_OK;
}

extern "C" int lld_sim3solver_batch_hypotheses(lld_sim3solver_batch* b, int32_t solver, int32_t capacity,
                                               lld_sim3solver_hypothesis* out, int32_t* n_window, int32_t* n_run) {
  if (!b || solver < 0 || solver >= b->n || capacity < 0 || (capacity > 0 && !out) || !n_window || !n_run) return LLD_ERR_INVALID;
  *n_window = 0; *n_run = 0;
  if (b->last_off.empty() || b->last_off[solver + 1] == b->last_off[solver]) return LLD_OK;
  LLD_HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t stream = b->ctx->stream;
  S3State st;
  LLD_HIP_TRY(hipMemcpyAsync(&st, b->dev.st + solver, sizeof(S3State), hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipStreamSynchronize(stream));
  const int W = st.window, h0 = b->last_off[solver], m = std::min(W, capacity);
  *n_window = W; *n_run = st.run;
  if (m == 0) return LLD_OK;
  std::vector<S3Hyp> hy(m);
  LLD_HIP_TRY(hipMemcpyAsync(hy.data(), b->dev.hyp + h0, sizeof(S3Hyp) * m, hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipStreamSynchronize(stream));
  for (int k = 0; k < m; ++k) {
    lld_sim3solver_hypothesis& o = out[k];
    o.n_inliers = hy[k].n_inliers;
    o.record = hy[k].record;
    for (int i = 0; i < 3; ++i) o.idx[i] = hy[k].idx[i];
    o.s = hy[k].s;
    for (int q = 0; q < 9; ++q) o.R[q] = hy[k].R[q];
    for (int q = 0; q < 3; ++q) o.t[q] = hy[k].t[q];
    for (int q = 0; q < 12; ++q) o.T12[q] = hy[k].T12[q];
  }
  return LLD_OK;
}

extern "C" int lld_sim3solver_find(lld_ctx* ctx, const lld_sim3solver_problem* problem, const lld_sim3solver_params* params,
                                   lld_sim3solver_result* out) {
  if (!ctx || !problem || !params || !out) return LLD_ERR_INVALID;
  lld_sim3solver_batch* b = nullptr;
  if (int st = lld_sim3solver_batch_create(ctx, 1, problem, params, &b)) return st;
  int st = lld_sim3solver_batch_find(b, nullptr);   // find() = iterate(mRansacMaxIts)
  if (st == LLD_OK) st = lld_sim3solver_batch_download(b, out);
  lld_sim3solver_batch_destroy(b);
  return st;
}
