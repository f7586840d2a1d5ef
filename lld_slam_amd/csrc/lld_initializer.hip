// lld_initializer.hip — ORB-SLAM2's Initializer (src/Initializer.cc): the homography / fundamental RANSAC of the monocular
// bootstrap and the reconstruction of the motion, as one device-resident sequence per Initialize() call.  The rules restated and
// the two deviations (a fresh rand() stream per call; the numerics OpenCV decides) are written out in include/lld_amd.h.
//
// The whole file is compiled without FMA contraction: every float / double operation is the one IEEE operation the restatement
// tests/initializer_ref.py performs, in its order, so that the two agree bit for bit (up to device libm's acos).
//
// Layout on the device (one handle): keys1[n1] float2 (mvKeys1) for the handle's life; per call one buffer with
//   keys2[n2] float2, match[N] int2 (mvMatches12), sets[8*iterations] int (mvSets)         <- the call's single upload
//   hyp[2*iterations] IHyp (H hypotheses, then F)      res IRes      inl_H[N], inl_F[N] uint8
//   motion[8] IMotion   rt_flag / rt_cos / rt_p3d [8*N] (CheckRT per motion hypothesis and match)   p3d[3*n1], tri[n1]
// Kernels of one call (no host trip between them):
//   ini_hyp      one lane per hypothesis, 16 per workgroup: the DLT's A^T A accumulated in LDS, the 9x9 Jacobi lane-interleaved
//                in LDS, for F the rank-2 step (3x3 SVD), the composition with T1 / T2 and H's inverse
//   ini_score    one wavefront per hypothesis: CheckHomography / CheckFundamental over the N matches, 64 at a time; the float
//                score is added in match order (lane by lane, every lane holding the same running sum), the count by ballot
//   ini_resolve  one workgroup: the `>` scans in iteration order, RH and the model, both winners' inlier masks, then one lane
//                builds the 4 (DecomposeE) or 8 (Faugeras) motion hypotheses
//   ini_checkrt  (N / 64) x 8 workgroups: Triangulate (4x4 Jacobi in LDS) and CheckRT's tests for one match and one motion
//   ini_select   one workgroup per motion: nGood and the exact min(50, nGood-1)-th smallest cosParallax (bitwise selection)
//   ini_final    one workgroup: ReconstructF's / ReconstructH's decision, vP3D and vbTriangulated scattered by match.first
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <vector>

#include "lld_common.h"
#include "lld_ransac.h"
#include "lld_wave.h"

namespace {

#define LLD_HD __device__ inline

constexpr int kHypLanes = 16;                // hypotheses per ini_hyp workgroup
constexpr int kHypDoubles = 162;             // per lane: A^T A (9x9) and its eigenvectors (9x9)
constexpr int kRtLanes = 64;                 // matches per ini_checkrt workgroup
constexpr int kRtDoubles = 32;               // per lane: A^T A (4x4) and its eigenvectors
constexpr int kThreads = 256;
constexpr double kSvdCut = 1e-9;             // a singular direction is kept when ||A v_k|| > kSvdCut * ||A v_0||

struct IHyp {
  int32_t idx[8];
  float M[9];                                // H21i or F21i
  float Minv[9];                             // H12i (H only)
  float score;
  int32_t n_inliers;
};

struct IMotion {
  float R[9], t[3];
  float P2[12];                              // K*[R|t]
  float O2[3];                               // -R^T t
};

struct IRes {
  int32_t success, model;
  float SH, SF, RH;
  float H21[9], F21[9];
  int32_t n_inliers_H, n_inliers_F;
  float R21[9], t21[3];
  int32_t n_good[8];
  float parallax[8];
  int32_t best_index, n_matches;
  int32_t win_H, win_F;
  int32_t n_motion;                          // internal: motion hypotheses built (0, 4 or 8)
  int32_t n_model_inliers;                   // internal: N of ReconstructF / ReconstructH
};

struct Dev {
  const float2* keys1; const float2* keys2; const int2* match; const int32_t* sets;
  IHyp* hyp; IRes* res; uint8_t* inl_H; uint8_t* inl_F;
  IMotion* motion; uint8_t* rt_flag; float* rt_cos; float* rt_p3d;
  float* p3d; uint8_t* tri;
  int n1, n2, N, iterations;
  float K[9];
  float nrm1[4], nrm2[4];                    // Normalize: meanX, meanY, sX, sY of each frame
  float sigma, min_parallax;
  int min_triangulated;
};

// ------------------------------------------------------------------ float matrices (DEVIATION 2)
// C (M x N) = A (M x K) * B (K x N): the float products summed in double in index order from the first, rounded to float once.
template <int M, int K, int N>
LLD_HD void matmul(const float* A, const float* B, float* C) {
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double s = (double)A[i * K] * (double)B[j];
#pragma unroll
      for (int k = 1; k < K; ++k) s += (double)A[i * K + k] * (double)B[k * N + j];
      C[i * N + j] = (float)s;
    }
}

LLD_HD void transpose3(const float* A, float* At) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) At[3 * i + j] = A[3 * j + i];
}

// cv::determinant of a float 3x3, in double on the widened entries.
LLD_HD double det3(const float* a) {
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7], a8 = a[8];
  return (a0 * (a4 * a8 - a5 * a7) - a1 * (a3 * a8 - a5 * a6)) + a2 * (a3 * a7 - a4 * a6);
}

// Mat::inv() of a float 3x3: cofactors over the determinant in double; a zero determinant gives the zero matrix (cv::invert).
LLD_HD void inv3(const float* a, float* o) {
  const double a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], a4 = a[4], a5 = a[5], a6 = a[6], a7 = a[7], a8 = a[8];
  const double det = det3(a);
  if (det == 0.0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) o[q] = 0.0f;
    return;
  }
  const double d = 1.0 / det;
  o[0] = (float)((a4 * a8 - a5 * a7) * d); o[1] = (float)((a2 * a7 - a1 * a8) * d); o[2] = (float)((a1 * a5 - a2 * a4) * d);
  o[3] = (float)((a5 * a6 - a3 * a8) * d); o[4] = (float)((a0 * a8 - a2 * a6) * d); o[5] = (float)((a2 * a3 - a0 * a5) * d);
  o[6] = (float)((a3 * a7 - a4 * a6) * d); o[7] = (float)((a1 * a6 - a0 * a7) * d); o[8] = (float)((a0 * a4 - a1 * a3) * d);
}

// cv::norm of a float 3-vector, in double.
LLD_HD double norm3(const float* v) {
  double s = (double)v[0] * (double)v[0];
  s += (double)v[1] * (double)v[1];
  s += (double)v[2] * (double)v[2];
  return sqrt(s);
}

// v / cv::norm(v): the reciprocal in double times the widened float, rounded.
LLD_HD void unit3(float* v) {
  const double r = 1.0 / norm3(v);
#pragma unroll
  for (int i = 0; i < 3; ++i) v[i] = (float)((double)v[i] * r);
}

// Eigenvector of the smallest eigenvalue (the highest index on a tie) of the n x n Jacobi result, canonical sign, as floats.
template <int n>
LLD_HD void null_vector(SP B, SP V, float* x) {
  int e = 0;
  for (int k = 1; k < n; ++k)
    if (B[k * n + k] <= B[e * n + e]) e = k;
  int m = 0;
  for (int k = 1; k < n; ++k)
    if (fabs(V[k * n + e]) > fabs(V[m * n + e])) m = k;
  const bool neg = V[m * n + e] < 0.0;
#pragma unroll
  for (int k = 0; k < n; ++k) x[k] = (float)(neg ? -V[k * n + e] : V[k * n + e]);
}

// Full SVD of a float 3x3, A = U diag(w) Vt with w descending (DEVIATION 2).  jac: 18 doubles.
LLD_HD void svd3(const float* A, SP jac, float* U, float* w, float* Vt) {
  SP B = jac, V = jac.at(9);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s += (double)A[3 * k + a] * (double)A[3 * k + b];
      B[3 * a + b] = s;
      B[3 * b + a] = s;
    }
  jacobi(B, V, 3);
  int o0 = 0;                                // the largest eigenvalue, the lowest index on a tie
  for (int k = 1; k < 3; ++k)
    if (B[4 * k] > B[4 * o0]) o0 = k;
  int o2 = -1;                               // the smallest of the others, the highest index on a tie
  for (int k = 0; k < 3; ++k)
    if (k != o0 && (o2 < 0 || B[4 * k] <= B[4 * o2])) o2 = k;
  const int o1 = 3 - o0 - o2;
  double v[3][3], u[3][3], wd[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int c = k == 0 ? o0 : (k == 1 ? o1 : o2);
    int m = 0;
    for (int j = 1; j < 3; ++j)
      if (fabs(V[3 * j + c]) > fabs(V[3 * m + c])) m = j;
    const bool neg = V[3 * m + c] < 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) v[k][j] = neg ? -V[3 * j + c] : V[3 * j + c];
#pragma unroll
    for (int i = 0; i < 3; ++i) {            // A v_k
      double s = (double)A[3 * i] * v[k][0];
      s += (double)A[3 * i + 1] * v[k][1];
      s += (double)A[3 * i + 2] * v[k][2];
      u[k][i] = s;
    }
    wd[k] = sqrt((u[k][0] * u[k][0] + u[k][1] * u[k][1]) + u[k][2] * u[k][2]);
  }
  // U's columns: A v_k / ||A v_k||; a (near) zero direction is completed to an orthonormal basis
  if (wd[0] > 0.0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) u[0][i] = u[0][i] / wd[0];
  } else {
    u[0][0] = 1.0; u[0][1] = 0.0; u[0][2] = 0.0;
  }
  if (wd[1] > kSvdCut * wd[0]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) u[1][i] = u[1][i] / wd[1];
  } else {                                   // the axis u0 is smallest along (the lowest on a tie), made orthogonal to u0
    const double b0 = fabs(u[0][0]), b1 = fabs(u[0][1]), b2 = fabs(u[0][2]);
    const int m = (b1 < b0) ? ((b2 < b1) ? 2 : 1) : ((b2 < b0) ? 2 : 0);
    const double um = m == 0 ? u[0][0] : (m == 1 ? u[0][1] : u[0][2]);
    double p[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = (i == m ? 1.0 : 0.0) - um * u[0][i];
    const double pn = sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) u[1][i] = p[i] / pn;
  }
  if (wd[2] > kSvdCut * wd[0]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) u[2][i] = u[2][i] / wd[2];
  } else {                                   // u0 x u1
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w[k] = (float)wd[k];
#pragma unroll
    for (int i = 0; i < 3; ++i) { U[3 * i + k] = (float)u[k][i]; Vt[3 * k + i] = (float)v[k][i]; }
  }
}

// Normalize's T (:790-794) from (meanX, meanY, sX, sY).
LLD_HD void norm_T(const float* nm, float* T) {
  T[0] = nm[2]; T[1] = 0.0f; T[2] = -nm[0] * nm[2];
  T[3] = 0.0f; T[4] = nm[3]; T[5] = -nm[1] * nm[3];
  T[6] = 0.0f; T[7] = 0.0f; T[8] = 1.0f;
}

// ------------------------------------------------------------------ hypotheses
// ComputeH21 (:226-266) or ComputeF21 (:268-303) on the 8 normalized pairs, composed as FindHomography / FindFundamental do.
// jac: kHypDoubles doubles.
LLD_HD void fit_hypothesis(bool is_F, const float* pn1, const float* pn2, const float* nrm1, const float* nrm2, SP jac, float* M,
                           float* Minv) {
  SP B = jac, V = jac.at(81);
  for (int q = 0; q < 81; ++q) B[q] = 0.0;
  for (int j = 0; j < 8; ++j) {
    const float u1 = pn1[2 * j], v1 = pn1[2 * j + 1], u2 = pn2[2 * j], v2 = pn2[2 * j + 1];
    if (is_F) {
      const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0f};
#pragma unroll
      for (int a = 0; a < 9; ++a)
#pragma unroll
        for (int b = a; b < 9; ++b) B[9 * a + b] = B[9 * a + b] + (double)r[a] * (double)r[b];
    } else {
      const float r0[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, v2 * u1, v2 * v1, v2};
      const float r1[9] = {u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, -u2 * u1, -u2 * v1, -u2};
#pragma unroll
      for (int a = 0; a < 9; ++a)
#pragma unroll
        for (int b = a; b < 9; ++b) {
          double s = B[9 * a + b] + (double)r0[a] * (double)r0[b];
          s = s + (double)r1[a] * (double)r1[b];
          B[9 * a + b] = s;
        }
    }
  }
  for (int a = 1; a < 9; ++a)
    for (int b = 0; b < a; ++b) B[9 * a + b] = B[9 * b + a];
  jacobi(B, V, 9);
  float h[9];
  null_vector<9>(B, V, h);
  float T1[9], T2[9], tmp[9];
  norm_T(nrm1, T1);
  norm_T(nrm2, T2);
  if (is_F) {
    float U[9], w[3], Vt[9], UW[9], Fn[9], T2t[9];
    svd3(h, jac, U, w, Vt);
    w[2] = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) UW[3 * i + k] = U[3 * i + k] * w[k];   // u*diag(w)
    matmul<3, 3, 3>(UW, Vt, Fn);
    transpose3(T2, T2t);
    matmul<3, 3, 3>(T2t, Fn, tmp);           // F21i = T2t*Fn*T1
    matmul<3, 3, 3>(tmp, T1, M);
#pragma unroll
    for (int q = 0; q < 9; ++q) Minv[q] = 0.0f;
  } else {
    float T2inv[9];
    inv3(T2, T2inv);
    matmul<3, 3, 3>(T2inv, h, tmp);          // H21i = T2inv*Hn*T1
    matmul<3, 3, 3>(tmp, T1, M);
    inv3(M, Minv);                           // H12i = H21i.inv()
  }
}

// One match of CheckHomography (:337-385): both one-sided score terms (0 when the side fails) and the inlier bit.
LLD_HD bool score_H(const float* H, const float* Hi, float u1, float v1, float u2, float v2, float invS2, float& c1, float& c2) {
  const float th = 5.991f;
  bool in = true;
  const float w2in1inv = (float)(1.0 / (double)(Hi[6] * u2 + Hi[7] * v2 + Hi[8]));
  const float u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
  const float v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
  const float sq1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  const float chi1 = sq1 * invS2;
  if (chi1 > th) { in = false; c1 = 0.0f; } else c1 = th - chi1;
  const float w1in2inv = (float)(1.0 / (double)(H[6] * u1 + H[7] * v1 + H[8]));
  const float u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
  const float v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
  const float sq2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  const float chi2 = sq2 * invS2;
  if (chi2 > th) { in = false; c2 = 0.0f; } else c2 = th - chi2;
  return in;
}

// One match of CheckFundamental (:413-465).
LLD_HD bool score_F(const float* F, float u1, float v1, float u2, float v2, float invS2, float& c1, float& c2) {
  const float th = 3.841f, thScore = 5.991f;
  bool in = true;
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float cc2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + cc2;
  const float sq1 = num2 * num2 / (a2 * a2 + b2 * b2);
  const float chi1 = sq1 * invS2;
  if (chi1 > th) { in = false; c1 = 0.0f; } else c1 = thScore - chi1;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float cc1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + cc1;
  const float sq2 = num1 * num1 / (a1 * a1 + b1 * b1);
  const float chi2 = sq2 * invS2;
  if (chi2 > th) { in = false; c2 = 0.0f; } else c2 = thScore - chi2;
  return in;
}

LLD_HD float inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

// ------------------------------------------------------------------ motion hypotheses
LLD_HD void fill_motion(const float* K, const float* R, const float* t, IMotion& m) {
  float Rt[12], Rtr[9], o[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) { m.R[3 * i + j] = R[3 * i + j]; Rt[4 * i + j] = R[3 * i + j]; }
    m.t[i] = t[i];
    Rt[4 * i + 3] = t[i];
  }
  matmul<3, 3, 4>(K, Rt, m.P2);              // P2 = K*[R|t]
  transpose3(R, Rtr);
  matmul<3, 3, 1>(Rtr, t, o);                // O2 = -R.t()*t
#pragma unroll
  for (int i = 0; i < 3; ++i) m.O2[i] = -o[i];
}

// ReconstructF's E21 and DecomposeE (:479-497, :909-929): (R1,t), (R2,t), (R1,-t), (R2,-t).  jac: 18 doubles.
LLD_HD void motions_F(const float* F, const float* K, SP jac, IMotion* out) {
  float Kt[9], tmp[9], E[9], U[9], w[3], Vt[9];
  transpose3(K, Kt);
  matmul<3, 3, 3>(Kt, F, tmp);
  matmul<3, 3, 3>(tmp, K, E);
  svd3(E, jac, U, w, Vt);
  float t[3] = {U[2], U[5], U[8]};
  unit3(t);
  const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  float Wt[9], R1[9], R2[9];
  transpose3(W, Wt);
  matmul<3, 3, 3>(U, W, tmp);
  matmul<3, 3, 3>(tmp, Vt, R1);
  if (det3(R1) < 0.0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) R1[q] = -R1[q];
  }
  matmul<3, 3, 3>(U, Wt, tmp);
  matmul<3, 3, 3>(tmp, Vt, R2);
  if (det3(R2) < 0.0) {
#pragma unroll
    for (int q = 0; q < 9; ++q) R2[q] = -R2[q];
  }
  const float tn[3] = {-t[0], -t[1], -t[2]};
  fill_motion(K, R1, t, out[0]);
  fill_motion(K, R2, t, out[1]);
  fill_motion(K, R1, tn, out[2]);
  fill_motion(K, R2, tn, out[3]);
}

// ReconstructH's eight Faugeras hypotheses (:584-686).  Returns 0 on the d1/d2, d2/d3 exit, else 8.  jac: 18 doubles.
LLD_HD int motions_H(const float* H, const float* K, SP jac, IMotion* out) {
  float invK[9], tmp[9], A[9], U[9], w[3], Vt[9];
  inv3(K, invK);
  matmul<3, 3, 3>(invK, H, tmp);
  matmul<3, 3, 3>(tmp, K, A);
  svd3(A, jac, U, w, Vt);
  const float s = (float)(det3(U) * det3(Vt));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return 0;
  const float aux1 = (float)sqrt((double)((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)));
  const float aux3 = (float)sqrt((double)((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3)));
  const float rad = (float)sqrt((double)((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)));
  const float aux_stheta = rad / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float aux_sphi = rad / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  float sU[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) sU[q] = s * U[q];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = i & 3;
    const float x1 = k < 2 ? aux1 : -aux1;
    const float x3 = (k & 1) ? -aux3 : aux3;
    const bool flip = k == 1 || k == 2;      // {aux, -aux, -aux, aux}
    float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float tp[3];
    if (i < 4) {                             // case d' = d2
      const float st = flip ? -aux_stheta : aux_stheta;
      Rp[0] = ctheta; Rp[2] = -st; Rp[6] = st; Rp[8] = ctheta;
      tp[0] = x1 * (d1 - d3); tp[1] = 0.0f * (d1 - d3); tp[2] = -x3 * (d1 - d3);
    } else {                                 // case d' = -d2
      const float sp = flip ? -aux_sphi : aux_sphi;
      Rp[0] = cphi; Rp[2] = sp; Rp[4] = -1.0f; Rp[6] = sp; Rp[8] = -cphi;
      tp[0] = x1 * (d1 + d3); tp[1] = 0.0f * (d1 + d3); tp[2] = x3 * (d1 + d3);
    }
    float R[9], t[3];
    matmul<3, 3, 3>(sU, Rp, tmp);            // R = s*U*Rp*Vt
    matmul<3, 3, 3>(tmp, Vt, R);
    matmul<3, 3, 1>(U, tp, t);               // t = U*tp, t/norm(t)
    unit3(t);
    fill_motion(K, R, t, out[i]);
  }
  return 8;
}

LLD_HD bool finite_f(float x) { return x - x == 0.0f; }   // isfinite: inf - inf and NaN - NaN are NaN

// ------------------------------------------------------------------ CheckRT for one match (:830-894)
// Returns bit 0: counted in nGood (vP3D written), bit 1: vbGood.  jac: kRtDoubles doubles.
LLD_HD int check_rt_one(const IMotion& m, const float* K, float th2, float x1, float y1, float x2, float y2, SP jac, float& cosp,
                        float* p) {
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float P1[12] = {K[0], K[1], K[2], 0.0f, K[3], K[4], K[5], 0.0f, K[6], K[7], K[8], 0.0f};
  float A[16];
#pragma unroll
  for (int j = 0; j < 4; ++j) {              // Triangulate (:734-747)
    A[j] = x1 * P1[8 + j] - P1[j];
    A[4 + j] = y1 * P1[8 + j] - P1[4 + j];
    A[8 + j] = x2 * m.P2[8 + j] - m.P2[j];
    A[12 + j] = y2 * m.P2[8 + j] - m.P2[4 + j];
  }
  SP B = jac, V = jac.at(16);
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
  float x[4];
  null_vector<4>(B, V, x);
  const double inv = 1.0 / (double)x[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = (float)((double)x[i] * inv);
  cosp = 0.0f;
  if (!finite_f(p[0]) || !finite_f(p[1]) || !finite_f(p[2])) return 0;
  const float dist1 = (float)norm3(p);       // normal1 = p3dC1 - O1, O1 = 0
  const float n2[3] = {p[0] - m.O2[0], p[1] - m.O2[1], p[2] - m.O2[2]};
  const float dist2 = (float)norm3(n2);
  double dot = (double)p[0] * (double)n2[0];
  dot += (double)p[1] * (double)n2[1];
  dot += (double)p[2] * (double)n2[2];
  cosp = (float)(dot / (double)(dist1 * dist2));
  const bool low = (double)cosp < 0.99998;
  if (p[2] <= 0.0f && low) return 0;
  float p2[3];
  matmul<3, 3, 1>(m.R, p, p2);               // p3dC2 = R*p3dC1+t
#pragma unroll
  for (int i = 0; i < 3; ++i) p2[i] = p2[i] + m.t[i];
  if (p2[2] <= 0.0f && low) return 0;
  const float invZ1 = (float)(1.0 / (double)p[2]);
  const float im1x = fx * p[0] * invZ1 + cx;
  const float im1y = fy * p[1] * invZ1 + cy;
  const float e1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
  if (e1 > th2) return 0;
  const float invZ2 = (float)(1.0 / (double)p2[2]);
  const float im2x = fx * p2[0] * invZ2 + cx;
  const float im2y = fy * p2[1] * invZ2 + cy;
  const float e2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
  if (e2 > th2) return 0;
  return low ? 3 : 1;
}

LLD_HD float th2_of(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }

// acos(c)*180/CV_PI, stored in a float.
LLD_HD float parallax_deg(float c) { return (float)(acos((double)c) * 180.0 / 3.1415926535897932384626433832795); }

// Order-preserving key of a float (sign-magnitude to unsigned).
LLD_HD uint32_t float_key(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
LLD_HD float key_float(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

// The final rule of ReconstructF (:499-569) / ReconstructH (:689-731) on the hypotheses' nGood and parallax.
LLD_HD bool decide(int model, int n_motion, const int32_t* g, const float* par, int N, int min_tri, float min_par, int& best) {
  best = -1;
  if (n_motion == 0) return false;
  if (model == 1) {
    const int maxGood = max(g[0], max(g[1], max(g[2], g[3])));
    const int nMinGood = max((int)(0.9 * N), min_tri);
    int nsimilar = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if ((double)g[i] > 0.7 * maxGood) nsimilar++;
    if (maxGood < nMinGood || nsimilar > 1) return false;
    best = maxGood == g[0] ? 0 : (maxGood == g[1] ? 1 : (maxGood == g[2] ? 2 : 3));
    const float pb = best == 0 ? par[0] : (best == 1 ? par[1] : (best == 2 ? par[2] : par[3]));
    return pb > min_par;
  }
  int bestGood = 0, second = 0;
  float bestPar = -1.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (g[i] > bestGood) { second = bestGood; bestGood = g[i]; best = i; bestPar = par[i]; }
    else if (g[i] > second) second = g[i];
  }
  return (double)second < 0.75 * bestGood && bestPar >= min_par && bestGood > min_tri && (double)bestGood > 0.9 * N;
}

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(kHypLanes) void ini_hyp(Dev d) {
  __shared__ double lds[kHypDoubles * kHypLanes];
  const int g = blockIdx.x * kHypLanes + threadIdx.x;
  if (g >= 2 * d.iterations) return;
  const bool is_F = g >= d.iterations;
  const int it = is_F ? g - d.iterations : g;
  IHyp& h = d.hyp[g];
  float pn1[16], pn2[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) {              // vPn1[mvMatches12[idx].first], vPn2[...second] (Normalize, :771-787)
    const int idx = d.sets[8 * it + j];
    h.idx[j] = idx;
    const int2 mt = d.match[idx];
    const float2 a = d.keys1[mt.x], b = d.keys2[mt.y];
    pn1[2 * j] = (a.x - d.nrm1[0]) * d.nrm1[2]; pn1[2 * j + 1] = (a.y - d.nrm1[1]) * d.nrm1[3];
    pn2[2 * j] = (b.x - d.nrm2[0]) * d.nrm2[2]; pn2[2 * j + 1] = (b.y - d.nrm2[1]) * d.nrm2[3];
  }
  float M[9], Minv[9];
  fit_hypothesis(is_F, pn1, pn2, d.nrm1, d.nrm2, SP{lds + threadIdx.x, kHypLanes}, M, Minv);
#pragma unroll
  for (int q = 0; q < 9; ++q) { h.M[q] = M[q]; h.Minv[q] = Minv[q]; }
}

__global__ __launch_bounds__(256) void ini_score(Dev d) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= 2 * d.iterations) return;
  const bool is_F = g >= d.iterations;
  float M[9], Mi[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) { M[q] = d.hyp[g].M[q]; Mi[q] = d.hyp[g].Minv[q]; }
  const float invS2 = inv_sigma2(d.sigma);
  float score = 0.0f;
  int cnt = 0;
  for (int i0 = 0; i0 < d.N; i0 += 64) {
    const int i = i0 + lane;
    float c1 = 0.0f, c2 = 0.0f;
    bool in = false;
    if (i < d.N) {
      const int2 mt = d.match[i];
      const float2 a = d.keys1[mt.x], b = d.keys2[mt.y];
      in = is_F ? score_F(M, a.x, a.y, b.x, b.y, invS2, c1, c2) : score_H(M, Mi, a.x, a.y, b.x, b.y, invS2, c1, c2);
    }
    cnt += __popcll(__ballot(in));
    // the sequential float sum in match order: every lane adds the 64 matches' two terms in order (a failed side and a lane past
    // N add +0, which leaves a sum that is never -0 unchanged)
#pragma unroll
    for (int l = 0; l < 64; ++l) {
      score = score + __shfl(c1, l);
      score = score + __shfl(c2, l);
    }
  }
  if (lane == 0) { d.hyp[g].score = score; d.hyp[g].n_inliers = cnt; }
}

__global__ __launch_bounds__(kThreads) void ini_resolve(Dev d) {
  __shared__ float M_sh[27];                 // H21, H12, F21 of the winners
  __shared__ int win_sh[2];
  __shared__ double jac[18];
  const int tid = threadIdx.x;
  IRes& res = *d.res;
  if (tid == 0) {
    int wH = -1, wF = -1;
    float SH = 0.0f, SF = 0.0f;
    for (int it = 0; it < d.iterations; ++it) {          // if(currentScore>score) (:165, :216)
      const float s = d.hyp[it].score;
      if (s > SH) { SH = s; wH = it; }
    }
    for (int it = 0; it < d.iterations; ++it) {
      const float s = d.hyp[d.iterations + it].score;
      if (s > SF) { SF = s; wF = it; }
    }
    const float RH = SH / (SH + SF);
    const int model = (double)RH > 0.40 ? 0 : 1;
    res.success = 0; res.model = model;
    res.SH = SH; res.SF = SF; res.RH = RH;
    res.win_H = wH; res.win_F = wF;
    res.n_inliers_H = wH >= 0 ? d.hyp[wH].n_inliers : 0;
    res.n_inliers_F = wF >= 0 ? d.hyp[d.iterations + wF].n_inliers : 0;
    for (int q = 0; q < 9; ++q) {
      const float h = wH >= 0 ? d.hyp[wH].M[q] : 0.0f, hi = wH >= 0 ? d.hyp[wH].Minv[q] : 0.0f;
      const float f = wF >= 0 ? d.hyp[d.iterations + wF].M[q] : 0.0f;
      res.H21[q] = h; res.F21[q] = f;
      M_sh[q] = h; M_sh[9 + q] = hi; M_sh[18 + q] = f;
      res.R21[q] = 0.0f;
    }
    for (int q = 0; q < 3; ++q) res.t21[q] = 0.0f;
    for (int q = 0; q < 8; ++q) { res.n_good[q] = 0; res.parallax[q] = 0.0f; }
    res.best_index = -1;
    res.n_matches = d.N;
    win_sh[0] = wH; win_sh[1] = wF;
    int n_motion = 0;
    if (model == 0 && wH >= 0) n_motion = motions_H(M_sh, d.K, SP{jac, 1}, d.motion);
    else if (model == 1 && wF >= 0) { motions_F(M_sh + 18, d.K, SP{jac, 1}, d.motion); n_motion = 4; }
    res.n_motion = n_motion;
    res.n_model_inliers = model == 0 ? res.n_inliers_H : res.n_inliers_F;
  }
  __syncthreads();
  float H[9], Hi[9], F[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) { H[q] = M_sh[q]; Hi[q] = M_sh[9 + q]; F[q] = M_sh[18 + q]; }
  const bool hasH = win_sh[0] >= 0, hasF = win_sh[1] >= 0;
  const float invS2 = inv_sigma2(d.sigma);
  for (int i = tid; i < d.N; i += kThreads) {
    const int2 mt = d.match[i];
    const float2 a = d.keys1[mt.x], b = d.keys2[mt.y];
    float c1, c2;
    d.inl_H[i] = hasH && score_H(H, Hi, a.x, a.y, b.x, b.y, invS2, c1, c2);
    d.inl_F[i] = hasF && score_F(F, a.x, a.y, b.x, b.y, invS2, c1, c2);
  }
}

__global__ __launch_bounds__(kRtLanes) void ini_checkrt(Dev d) {
  __shared__ double lds[kRtDoubles * kRtLanes];
  const int h = blockIdx.y;
  const int i = blockIdx.x * kRtLanes + threadIdx.x;
  if (h >= d.res->n_motion || i >= d.N) return;
  const size_t o = (size_t)h * d.N + i;
  const uint8_t in = d.res->model == 0 ? d.inl_H[i] : d.inl_F[i];
  int flag = 0;
  float cosp = 0.0f, p[3] = {0.0f, 0.0f, 0.0f};
  if (in) {
    const int2 mt = d.match[i];
    const float2 a = d.keys1[mt.x], b = d.keys2[mt.y];
    flag = check_rt_one(d.motion[h], d.K, th2_of(d.sigma), a.x, a.y, b.x, b.y, SP{lds + threadIdx.x, kRtLanes}, cosp, p);
  }
  d.rt_flag[o] = (uint8_t)flag;
  d.rt_cos[o] = cosp;
  d.rt_p3d[3 * o] = p[0]; d.rt_p3d[3 * o + 1] = p[1]; d.rt_p3d[3 * o + 2] = p[2];
}

__global__ __launch_bounds__(kThreads) void ini_select(Dev d) {
  __shared__ int sh[4];
  const int h = blockIdx.x, tid = threadIdx.x;
  if (h >= d.res->n_motion) return;
  const uint8_t* fl = d.rt_flag + (size_t)h * d.N;
  const float* cs = d.rt_cos + (size_t)h * d.N;
  int c = 0;
  for (int i = tid; i < d.N; i += kThreads) c += fl[i] & 1;
  const int nGood = lld_wave::block_sum(c, sh);
  float par = 0.0f;
  if (nGood > 0) {
    // sorted[idx], idx = min(50, nGood-1): the largest key with at most idx counted keys below it, built bit by bit
    const int idx = min(50, nGood - 1);
    uint32_t key = 0;
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t trial = key | (1u << bit);
      int below = 0;
      for (int i = tid; i < d.N; i += kThreads) below += ((fl[i] & 1) && float_key(cs[i]) < trial) ? 1 : 0;
      if (lld_wave::block_sum(below, sh) <= idx) key = trial;
    }
    par = parallax_deg(key_float(key));
  }
  if (tid == 0) { d.res->n_good[h] = nGood; d.res->parallax[h] = par; }
}

__global__ __launch_bounds__(kThreads) void ini_final(Dev d) {
  __shared__ int ok_sh, best_sh;
  const int tid = threadIdx.x;
  IRes& res = *d.res;
  if (tid == 0) {
    int best = -1;
    const bool ok = decide(res.model, res.n_motion, res.n_good, res.parallax, res.n_model_inliers, d.min_triangulated,
                           d.min_parallax, best);
    res.success = ok ? 1 : 0;
    res.best_index = best;
    if (ok) {
      for (int q = 0; q < 9; ++q) res.R21[q] = d.motion[best].R[q];
      for (int q = 0; q < 3; ++q) res.t21[q] = d.motion[best].t[q];
    }
    ok_sh = ok; best_sh = best;
  }
  for (int i = tid; i < d.n1; i += kThreads) {
    d.tri[i] = 0;
    d.p3d[3 * i] = 0.0f; d.p3d[3 * i + 1] = 0.0f; d.p3d[3 * i + 2] = 0.0f;
  }
  __syncthreads();
  if (!ok_sh) return;
  const size_t o = (size_t)best_sh * d.N;
  for (int i = tid; i < d.N; i += kThreads) {
    const int fl = d.rt_flag[o + i];
    if (!(fl & 1)) continue;
    const int k = d.match[i].x;                // vMatches12[i].first
    d.p3d[3 * k] = d.rt_p3d[3 * (o + i)]; d.p3d[3 * k + 1] = d.rt_p3d[3 * (o + i) + 1]; d.p3d[3 * k + 2] = d.rt_p3d[3 * (o + i) + 2];
    d.tri[k] = (fl >> 1) & 1;
  }
}

// Normalize's means and scales (:751-782): sequential float sums over all keypoints of the frame.
void normalize_frame(const float* xy, int n, float* nm) {
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; ++i) { meanX += xy[2 * i]; meanY += xy[2 * i + 1]; }
  meanX = meanX / n; meanY = meanY / n;
  float devX = 0, devY = 0;
  for (int i = 0; i < n; ++i) { devX += fabsf(xy[2 * i] - meanX); devY += fabsf(xy[2 * i + 1] - meanY); }
  devX = devX / n; devY = devY / n;
  nm[0] = meanX; nm[1] = meanY;
  nm[2] = (float)(1.0 / (double)devX); nm[3] = (float)(1.0 / (double)devY);
}

bool all_finite(const float* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

}  // namespace

// ------------------------------------------------------------------ host side
struct lld_initializer {
  lld_ctx* ctx = nullptr;
  lld_initializer_params params{};
  int n1 = 0;
  float K[9] = {};
  float nrm1[4] = {};
  void* dkeys1 = nullptr;
  void* dcall = nullptr; size_t dcall_bytes = 0;
  std::vector<char> stage;
  Dev dev{};
  bool has_call = false;
};

extern "C" void lld_initializer_params_default(lld_initializer_params* p) {
  if (!p) return;
  p->sigma = 1.0f; p->iterations = 200; p->min_parallax = 1.0f; p->min_triangulated = 50; p->seed = 0;
}

extern "C" int lld_initializer_create(lld_ctx* ctx, const float* K, int32_t n1, const float* keys1_xy,
                                      const lld_initializer_params* params, lld_initializer** out) {
  if (!ctx || !K || !keys1_xy || !params || !out) return LLD_ERR_INVALID;
  *out = nullptr;
  if (n1 < 1) return LLD_ERR_INVALID;
  if (n1 > LLD_INIT_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  if (params->iterations < 1 || params->iterations > LLD_INIT_MAX_ITERATIONS) return LLD_ERR_INVALID;
  if (!(params->sigma > 0.0f) || !std::isfinite(params->sigma)) return LLD_ERR_INVALID;
  if (!all_finite(K, 9) || !(K[0] > 0.0f) || !(K[4] > 0.0f)) return LLD_ERR_INVALID;
  if (!all_finite(keys1_xy, 2 * (size_t)n1)) return LLD_ERR_INVALID;
  auto* h = new lld_initializer();
  h->ctx = ctx; h->params = *params; h->n1 = n1;
  std::memcpy(h->K, K, sizeof(h->K));
  normalize_frame(keys1_xy, n1, h->nrm1);
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&h->dkeys1, sizeof(float2) * (size_t)n1) != hipSuccess) {
    h->dkeys1 = nullptr;
    lld_initializer_destroy(h);
    return LLD_ERR_ALLOC;
  }
  if (hipMemcpyAsync(h->dkeys1, keys1_xy, sizeof(float2) * (size_t)n1, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    lld_initializer_destroy(h);
    return LLD_ERR_HIP;
  }
  *out = h;
  return LLD_OK;
}

extern "C" void lld_initializer_destroy(lld_initializer* h) {
  if (!h) return;
  if (h->ctx) (void)hipSetDevice(h->ctx->device);
  if (h->dkeys1) (void)hipFree(h->dkeys1);
  if (h->dcall) (void)hipFree(h->dcall);
  delete h;
}

static void ini_copy_result(const IRes& r, lld_initializer_result* o) {
  o->success = r.success; o->model = r.model;
  o->SH = r.SH; o->SF = r.SF; o->RH = r.RH;
  for (int q = 0; q < 9; ++q) { o->H21[q] = r.H21[q]; o->F21[q] = r.F21[q]; o->R21[q] = r.R21[q]; }
  for (int q = 0; q < 3; ++q) o->t21[q] = r.t21[q];
  for (int q = 0; q < 8; ++q) { o->n_good[q] = r.n_good[q]; o->parallax[q] = r.parallax[q]; }
  o->n_inliers_H = r.n_inliers_H; o->n_inliers_F = r.n_inliers_F;
  o->best_index = r.best_index; o->n_matches = r.n_matches;
  o->win_H = r.win_H; o->win_F = r.win_F;
}

extern "C" int lld_initializer_initialize(lld_initializer* h, int32_t n2, const float* keys2_xy, int32_t n12, const int32_t* matches12,
                                          lld_initializer_result* result) {
  if (!h || !keys2_xy || !matches12 || !result) return LLD_ERR_INVALID;
  if (n2 < 1 || n12 < 1) return LLD_ERR_INVALID;
  if (n2 > LLD_INIT_MAX_KEYPOINTS || n12 > LLD_INIT_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  if (n12 != h->n1) return LLD_ERR_INVALID;
  if (!all_finite(keys2_xy, 2 * (size_t)n2)) return LLD_ERR_INVALID;
  int N = 0;
  for (int i = 0; i < n12; ++i) {
    if (matches12[i] >= n2) return LLD_ERR_INVALID;
    if (matches12[i] >= 0) ++N;
  }
  if (N < 8) return LLD_ERR_INVALID;           // the reference would draw from an empty vAvailableIndices
  h->has_call = false;
  lld_ctx* ctx = h->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const int its = h->params.iterations, n1 = h->n1;
  // the call's single upload: keys2 | mvMatches12 | mvSets
  const size_t b_keys = lld_slab::pad(sizeof(float2) * (size_t)n2), b_match = lld_slab::pad(sizeof(int2) * (size_t)N),
               b_sets = lld_slab::pad(sizeof(int32_t) * 8 * (size_t)its);
  const size_t up = b_keys + b_match + b_sets;
  h->stage.assign(up, 0);
  std::memcpy(h->stage.data(), keys2_xy, sizeof(float2) * (size_t)n2);
  int2* match = reinterpret_cast<int2*>(h->stage.data() + b_keys);
  int32_t* sets = reinterpret_cast<int32_t*>(h->stage.data() + b_keys + b_match);
  for (int i = 0, k = 0; i < n12; ++i)        // mvMatches12 (:54-63): index order of vMatches12 >= 0
    if (matches12[i] >= 0) match[k++] = make_int2(i, matches12[i]);
  {                                           // mvSets (:78-97) from a fresh stream after srand(seed) (DEVIATION 1)
    uint32_t ring[31]; int32_t head;
    srand_state(h->params.seed, ring, &head);
    for (int it = 0; it < its; ++it) draw_set<8>(ring, head, N, sets + 8 * it);
  }
  const size_t NN = (size_t)N;
  const size_t need = up + lld_slab::pad(sizeof(IHyp) * 2 * (size_t)its) + lld_slab::pad(sizeof(IRes)) + 2 * lld_slab::pad(NN) +
                      lld_slab::pad(sizeof(IMotion) * 8) + lld_slab::pad(8 * NN) + lld_slab::pad(sizeof(float) * 8 * NN) +
                      lld_slab::pad(sizeof(float) * 24 * NN) + lld_slab::pad(sizeof(float) * 3 * (size_t)n1) + lld_slab::pad((size_t)n1);
  if (int rc = lld_grow_device(&h->dcall, &h->dcall_bytes, need)) return rc;
  lld_slab sl; sl.base = (char*)h->dcall; sl.size = need;
  Dev d{};
  char* up_base = sl.take<char>(up);
  d.keys1 = (const float2*)h->dkeys1;
  d.keys2 = (const float2*)up_base;
  d.match = (const int2*)(up_base + b_keys);
  d.sets = (const int32_t*)(up_base + b_keys + b_match);
  d.hyp = sl.take<IHyp>(2 * (size_t)its);
  d.res = sl.take<IRes>(1);
  d.inl_H = sl.take<uint8_t>(NN);
  d.inl_F = sl.take<uint8_t>(NN);
  d.motion = sl.take<IMotion>(8);
  d.rt_flag = sl.take<uint8_t>(8 * NN);
  d.rt_cos = sl.take<float>(8 * NN);
  d.rt_p3d = sl.take<float>(24 * NN);
  d.p3d = sl.take<float>(3 * (size_t)n1);
  d.tri = sl.take<uint8_t>((size_t)n1);
  d.n1 = n1; d.n2 = n2; d.N = N; d.iterations = its;
  std::memcpy(d.K, h->K, sizeof(d.K));
  std::memcpy(d.nrm1, h->nrm1, sizeof(d.nrm1));
  normalize_frame(keys2_xy, n2, d.nrm2);
  d.sigma = h->params.sigma; d.min_parallax = h->params.min_parallax; d.min_triangulated = h->params.min_triangulated;
  h->dev = d;
  hipStream_t stream = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(up_base, h->stage.data(), up, hipMemcpyHostToDevice, stream));
  ini_hyp<<<(2 * its + kHypLanes - 1) / kHypLanes, kHypLanes, 0, stream>>>(d);
  ini_score<<<(2 * its + 3) / 4, 256, 0, stream>>>(d);
  ini_resolve<<<1, kThreads, 0, stream>>>(d);
  ini_checkrt<<<dim3((N + kRtLanes - 1) / kRtLanes, 8), kRtLanes, 0, stream>>>(d);
  ini_select<<<8, kThreads, 0, stream>>>(d);
  ini_final<<<1, kThreads, 0, stream>>>(d);
  LLD_HIP_TRY(hipGetLastError());
  IRes r;
  LLD_HIP_TRY(hipMemcpyAsync(&r, d.res, sizeof(IRes), hipMemcpyDeviceToHost, stream));
  if (result->inlier_H) LLD_HIP_TRY(hipMemcpyAsync(result->inlier_H, d.inl_H, NN, hipMemcpyDeviceToHost, stream));
  if (result->inlier_F) LLD_HIP_TRY(hipMemcpyAsync(result->inlier_F, d.inl_F, NN, hipMemcpyDeviceToHost, stream));
  if (result->p3d) LLD_HIP_TRY(hipMemcpyAsync(result->p3d, d.p3d, sizeof(float) * 3 * (size_t)n1, hipMemcpyDeviceToHost, stream));
  if (result->triangulated) LLD_HIP_TRY(hipMemcpyAsync(result->triangulated, d.tri, (size_t)n1, hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipStreamSynchronize(stream));
  ini_copy_result(r, result);
  h->has_call = true;
  return LLD_OK;
}

extern "C" int lld_initializer_hypotheses(lld_initializer* h, int32_t model, int32_t capacity, lld_initializer_hypothesis* out,
                                          int32_t* n) {
  if (!h || (model != 0 && model != 1) || capacity < 0 || (capacity > 0 && !out) || !n) return LLD_ERR_INVALID;
  *n = 0;
  if (!h->has_call) return LLD_OK;
  const int its = h->dev.iterations, m = std::min(its, capacity);
  *n = its;
  if (m == 0) return LLD_OK;
  LLD_HIP_TRY(hipSetDevice(h->ctx->device));
  std::vector<IHyp> hy(m);
  LLD_HIP_TRY(hipMemcpyAsync(hy.data(), h->dev.hyp + (model ? its : 0), sizeof(IHyp) * m, hipMemcpyDeviceToHost, h->ctx->stream));
  LLD_HIP_TRY(hipStreamSynchronize(h->ctx->stream));
  for (int k = 0; k < m; ++k) {
    for (int j = 0; j < 8; ++j) out[k].idx[j] = hy[k].idx[j];
    for (int q = 0; q < 9; ++q) out[k].M[q] = hy[k].M[q];
    out[k].score = hy[k].score;
    out[k].n_inliers = hy[k].n_inliers;
  }
  return LLD_OK;
}

extern "C" int lld_initializer_find(lld_ctx* ctx, const float* K, int32_t n1, const float* keys1_xy, int32_t n2, const float* keys2_xy,
                                    int32_t n12, const int32_t* matches12, const lld_initializer_params* params,
                                    lld_initializer_result* result) {
  lld_initializer* h = nullptr;
  if (int st = lld_initializer_create(ctx, K, n1, keys1_xy, params, &h)) return st;
  const int st = lld_initializer_initialize(h, n2, keys2_xy, n12, matches12, result);
  lld_initializer_destroy(h);
  return st;
}
