// lld_pnp.hip — ORB-SLAM2's PnPsolver (src/PnPsolver.cc) as a batch of independent solvers whose RANSAC state stays in HBM
// between iterate() calls.  The rules restated and the two deviations (one rand() stream per solver; the null-space basis of a
// minimal set) are written out in include/lld_amd.h.
//
// The whole file is compiled without FMA contraction: every double / float operation is the one IEEE operation the reference's
// C++ performs, in its order, so that the restatement tests/pnp_ref.py agrees bit for bit.  Every sum over correspondences runs
// in ascending index order on one lane, as the reference's loops do.
//
// Layout on the device (one handle):
//   pt[N_total]  float4 (X, Y, Z, mvMaxError)      uv[N_total] float2      kp[N_total] int (mvKeyPointIndices)
//   desc[n]      PnpDesc: the solver's range, its RANSAC constants (SetRansacParameters, computed on the host) and camera
//   st[n]        PnpState: the rand() stream, mnIterations, mnBestInliers and the best hypothesis (double R|t, float Tcw)
//   res[n]       PnpRes: the last iterate()'s outputs      flags[sum n_keypoints] uint8 vbInliers
//   per call     hypothesis slots [hyp_off[s], hyp_off[s+1]) of every solver (the host bound max(n, mRansacMaxIts)):
//                sampled indices, R|t, inlier counts, the record / Refine job of each; Refine jobs [job_off[s], job_off[s]+bound+1)
// Kernels of one iterate call (no host trip between them):
//   pnp_sample   one lane per solver: the window max(n, budget - mnIterations) (0 when N < mRansacMinInliers), the stream saved,
//                4 indices per hypothesis (RandomInt and the swap-with-back removal of vAvailableIndices)
//   pnp_hyp      one lane per hypothesis, 32 per workgroup, scratch lane-interleaved in LDS: EPnP on the minimal set
//   pnp_count    one wavefront per hypothesis: CheckInliers over N, count by ballot / popcount
//   pnp_records  one lane per solver: the strict prefix maximum over eligible hypotheses -> the records, one Refine job each (and
//                one for the best set carried in from the previous call)
//   pnp_refine   one workgroup per job: the record's inliers in ascending order, EPnP on them (sums one lane each, 12x12 Jacobi),
//                CheckInliers
//   pnp_resolve  one workgroup per solver: iterate()'s order replayed, the state and outputs, vbInliers scattered by keypoint,
//                the stream advanced by the draws actually made
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <vector>

#include "lld_common.h"
#include "lld_pnp_internal.h"
#include "lld_ransac.h"
#include "lld_wave.h"

namespace {

constexpr double kPinvCut = 1e-14;           // eigenvalue of A^T A kept when > kPinvCut * the largest
constexpr int kHypLanes = 32;                // minimal-set hypotheses per workgroup (bound by their LDS scratch)
constexpr int kThreads = 256;                // refine / resolve workgroups

struct PnpDesc {
  int32_t off, n, n_kp, kp_off;
  int32_t min_inliers, max_its, pad[2];
  double fu, fv, uc, vc;
};

struct PnpState {
  RansacStream rng;
  int32_t n_iter;                            // mnIterations
  int32_t best;                              // mnBestInliers
  int32_t window;                            // hypotheses drawn for this call (0: N < mRansacMinInliers)
  int32_t run;                               // of which iterate() made (the rest is speculative)
  int32_t carried_job;                       // the job refining the carried-in best set, or -1
  int32_t pad[3];
  double best_rt[12];                        // mRi / mti of the record (row-major R, then t)
  float best_tcw[12];                        // mBestTcw (float)
};

using lld_pnp::PnpRes;                       // the last iterate()'s outputs (lld_pnp_internal.h)

struct PnpJob {                              // one Refine
  int32_t solver, hyp;                       // hyp: global hypothesis slot, -1 = the carried-in best set
  int32_t n_inliers, ok;                     // outcome
  double rt[12];                             // refined R|t
};

struct HypRec {
  int32_t n_inliers;
  int32_t record;                            // 1: a new best
  int32_t job;                               // the Refine that iterate() would run here (best-so-far set), -1: not eligible
  int32_t pad;
};

// Selection sort of the indices by ascending |lambda| into ord (stored as doubles).
__device__ void order_abs(SP A, int n, SP ord) {
  for (int i = 0; i < n; ++i) ord[i] = (double)i;
  for (int i = 0; i < n; ++i) {
    int m = i;
    for (int j = i + 1; j < n; ++j)
      if (fabs(A[(int)ord[j] * (n + 1)]) < fabs(A[(int)ord[m] * (n + 1)])) m = j;
    double t = ord[i]; ord[i] = ord[m]; ord[m] = t;
  }
}

// A^T A of an m x n matrix given by a functor -> jac[0 .. n*n), its Jacobi into jac / jac+25, w_k into jac+50.
template <class F>
__device__ void pinv_eig(F A, int m, int n, SP jac) {
  SP B = jac, V = jac.at(25), w = jac.at(50);
  for (int a = 0; a < n; ++a)
    for (int b = a; b < n; ++b) {
      double s = 0.0;
      for (int i = 0; i < m; ++i) s += A(i, a) * A(i, b);
      B[a * n + b] = s;
      B[b * n + a] = s;
    }
  jacobi(B, V, n);
  double lmax = 0.0;
  for (int k = 0; k < n; ++k)
    if (fabs(B[k * n + k]) > lmax) lmax = fabs(B[k * n + k]);
  for (int k = 0; k < n; ++k) {
    double l = B[k * n + k];
    w[k] = l > kPinvCut * lmax ? 1.0 / l : 0.0;
  }
}

// x = (A^T A)^+ atb with the decomposition of pinv_eig (atb in jac+56 .. +61, y in jac+61 .. +66).
__device__ void pinv_solve(SP jac, int n, SP x) {
  SP V = jac.at(25), w = jac.at(50), atb = jac.at(56), y = jac.at(61);
  for (int k = 0; k < n; ++k) {
    double s = 0.0;
    for (int c = 0; c < n; ++c) s += V[c * n + k] * atb[c];
    y[k] = w[k] * s;
  }
  for (int a = 0; a < n; ++a) {
    double s = 0.0;
    for (int k = 0; k < n; ++k) s += V[a * n + k] * y[k];
    x[a] = s;
  }
}

constexpr int kJac = 66;                     // doubles of pinv / Jacobi scratch (5x5 + 5x5 + w + atb + y)

// Scratch of one EPnP (doubles): see the offsets.
constexpr int oCws = 0;                      // cws[4][3]
constexpr int oCi = 12;                      // cc_inv[3][3]
constexpr int oBasis = 21;                   // v[4][12] (v[i] = ut row 11 - i)
constexpr int oL = 69;                       // L_6x10
constexpr int oRho = 129;                    // rho[6]
constexpr int oGa = 135;                     // Gauss-Newton A[6][4]
constexpr int oGb = 159;                     // b[6]
constexpr int oGx = 165;                     // x[4]
constexpr int oQr = 169;                     // qr_solve A1[4], A2[4]
constexpr int oBetas = 177;                  // betas[3][4]
constexpr int oCcs = 189;                    // ccs[3][4][3]
constexpr int oR = 225;                      // R[3][9], t[3][3]
constexpr int oT = 252;
constexpr int oOrd = 261;                    // sort order (12)
constexpr int oJac = 273;                    // kJac
static_assert(oJac + kJac <= 339, "Jacobi scratch");
constexpr int oAbt = 339;                    // abt[9], pc0[3]
constexpr int oPc0 = 348;
constexpr int kEpnpCore = 351;
constexpr int oMt = oL;                      // minimal sets only: M^T (12 x 8), dead before L / rho / Gauss-Newton are written
constexpr int oPts = kEpnpCore;              // minimal sets only: pws[4][3], us[4][2], alphas[4][4]
constexpr int kHypScratch = oPts + 36;       // 387 doubles per lane
static_assert(oMt + 96 <= oGx, "M^T overlays L, rho and the Gauss-Newton system only");

// choose_control_points (:375-409) after the sums and compute_barycentric_coordinates' CC and cc_inv (:411-434).  pp: the 3x3
// PW0^T PW0 in jac[0..9) on entry; c0 in cws[0..3).
__device__ void control_points(SP w, int n) {
  SP jac = w.at(oJac), V = jac.at(25), ord = w.at(oOrd), cws = w.at(oCws), tmp = jac.at(61);
  jacobi(jac, V, 3);
  order_abs(jac, 3, ord);
  for (int i = 1; i < 4; ++i) {
    int e = (int)ord[3 - i];                 // descending |lambda|, as cvSVD orders dc
    canonical_col(V, 3, e, tmp);
    double k = sqrt(fabs(jac[e * 4]) / n);
    for (int j = 0; j < 3; ++j) cws[3 * i + j] = cws[j] + k * tmp[j];
  }
  auto CC = [&](int i, int j) { return cws[3 * (j + 1) + i] - cws[i]; };
  pinv_eig(CC, 3, 3, jac);
  SP ci = w.at(oCi);
  for (int b = 0; b < 3; ++b) {
    for (int c = 0; c < 3; ++c) jac[56 + c] = CC(b, c);
    SP x = w.at(oGx);
    pinv_solve(jac, 3, x);
    for (int a = 0; a < 3; ++a) ci[3 * a + b] = x[a];
  }
}

__device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// compute_L_6x10 (:760-800) and compute_rho (:802-810).
__device__ void fill_L_rho(SP w) {
  SP v = w.at(oBasis), L = w.at(oL), rho = w.at(oRho), cws = w.at(oCws);
  for (int i = 0; i < 6; ++i) {
    const int a = i < 3 ? 0 : (i < 5 ? 1 : 2);
    const int b = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);
    double dv[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int k = 0; k < 3; ++k) dv[q][k] = v[12 * q + 3 * a + k] - v[12 * q + 3 * b + k];
    L[10 * i + 0] = dot3(dv[0], dv[0]);
    L[10 * i + 1] = 2.0 * dot3(dv[0], dv[1]);
    L[10 * i + 2] = dot3(dv[1], dv[1]);
    L[10 * i + 3] = 2.0 * dot3(dv[0], dv[2]);
    L[10 * i + 4] = 2.0 * dot3(dv[1], dv[2]);
    L[10 * i + 5] = dot3(dv[2], dv[2]);
    L[10 * i + 6] = 2.0 * dot3(dv[0], dv[3]);
    L[10 * i + 7] = 2.0 * dot3(dv[1], dv[3]);
    L[10 * i + 8] = 2.0 * dot3(dv[2], dv[3]);
    L[10 * i + 9] = dot3(dv[3], dv[3]);
  }
  const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double d0 = cws[3 * pa[i]] - cws[3 * pb[i]], d1 = cws[3 * pa[i] + 1] - cws[3 * pb[i] + 1], d2 = cws[3 * pa[i] + 2] - cws[3 * pb[i] + 2];
    rho[i] = d0 * d0 + d1 * d1 + d2 * d2;
  }
}

// qr_solve (:840-952) on the 6x4 A / b of w; x written only when no column is zero (the reference returns early otherwise).
__device__ void qr_solve(SP w) {
  SP A = w.at(oGa), b = w.at(oGb), X = w.at(oGx), A1 = w.at(oQr), A2 = w.at(oQr + 4);
  const int nr = 6, nc = 4;
  for (int k = 0; k < nc; ++k) {
    double eta = fabs(A[k * nc + k]);
    for (int i = k + 1; i < nr; ++i) {
      double elt = fabs(A[i * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) return;
    double sum = 0.0, inv_eta = 1. / eta;
    for (int i = k; i < nr; ++i) {
      A[i * nc + k] *= inv_eta;
      sum += A[i * nc + k] * A[i * nc + k];
    }
    double sigma = sqrt(sum);
    if (A[k * nc + k] < 0) sigma = -sigma;
    A[k * nc + k] += sigma;
    A1[k] = sigma * A[k * nc + k];
    A2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; ++j) {
      double s = 0;
      for (int i = k; i < nr; ++i) s += A[i * nc + k] * A[i * nc + j];
      double tau = s / A1[k];
      for (int i = k; i < nr; ++i) A[i * nc + j] -= tau * A[i * nc + k];
    }
  }
  for (int j = 0; j < nc; ++j) {
    double tau = 0;
    for (int i = j; i < nr; ++i) tau += A[i * nc + j] * b[i];
    tau /= A1[j];
    for (int i = j; i < nr; ++i) b[i] -= tau * A[i * nc + j];
  }
  X[nc - 1] = b[nc - 1] / A2[nc - 1];
  for (int i = nc - 2; i >= 0; --i) {
    double s = 0;
    for (int j = i + 1; j < nc; ++j) s += A[i * nc + j] * X[j];
    X[i] = (b[i] - s) / A2[i];
  }
}

// gauss_newton (:818-838) with compute_A_and_b_gauss_newton (:812-816).
__device__ void gauss_newton(SP w, SP betas) {
  SP L = w.at(oL), rho = w.at(oRho), A = w.at(oGa), b = w.at(oGb), X = w.at(oGx);
  for (int i = 0; i < 4; ++i) X[i] = 0.0;
  for (int it = 0; it < 5; ++it) {
    double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
    for (int i = 0; i < 6; ++i) {
      SP r = L.at(10 * i);
      A[4 * i + 0] = 2 * r[0] * b0 + r[1] * b1 + r[3] * b2 + r[6] * b3;
      A[4 * i + 1] = r[1] * b0 + 2 * r[2] * b1 + r[4] * b2 + r[7] * b3;
      A[4 * i + 2] = r[3] * b0 + r[4] * b1 + 2 * r[5] * b2 + r[8] * b3;
      A[4 * i + 3] = r[6] * b0 + r[7] * b1 + r[8] * b2 + 2 * r[9] * b3;
      b[i] = rho[i] - (r[0] * b0 * b0 + r[1] * b0 * b1 + r[2] * b1 * b1 + r[3] * b0 * b2 + r[4] * b1 * b2 + r[5] * b2 * b2 +
                       r[6] * b0 * b3 + r[7] * b1 * b3 + r[8] * b2 * b3 + r[9] * b3 * b3);
    }
    qr_solve(w);
    for (int i = 0; i < 4; ++i) betas[i] += X[i];
  }
}

// find_betas_approx_1/2/3 (:667-758), each followed by gauss_newton, and compute_ccs (:454-466) with solve_for_sign (:629-634)
// decided on the first point (alpha0: its barycentric coordinates).
__device__ void betas_and_ccs(SP w, const double* alpha0) {
  SP L = w.at(oL), rho = w.at(oRho), jac = w.at(oJac), x = w.at(oGx), atb = jac.at(56);
  const int c4[4] = {0, 1, 3, 6};
  for (int set = 0; set < 3; ++set) {
    SP bet = w.at(oBetas + 4 * set);
    const int k = set == 0 ? 4 : (set == 1 ? 3 : 5);
    auto A = [&](int i, int c) { return L[10 * i + (set == 0 ? c4[c] : c)]; };
    pinv_eig(A, 6, k, jac);
    for (int c = 0; c < k; ++c) {
      double s = 0.0;
      for (int i = 0; i < 6; ++i) s += A(i, c) * rho[i];
      atb[c] = s;
    }
    pinv_solve(jac, k, x);
    if (set == 0) {
      if (x[0] < 0) {
        bet[0] = sqrt(-x[0]); bet[1] = -x[1] / bet[0]; bet[2] = -x[2] / bet[0]; bet[3] = -x[3] / bet[0];
      } else {
        bet[0] = sqrt(x[0]); bet[1] = x[1] / bet[0]; bet[2] = x[2] / bet[0]; bet[3] = x[3] / bet[0];
      }
    } else {
      if (x[0] < 0) {
        bet[0] = sqrt(-x[0]); bet[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0;
      } else {
        bet[0] = sqrt(x[0]); bet[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0;
      }
      if (x[1] < 0) bet[0] = -bet[0];
      bet[2] = set == 2 ? x[3] / bet[0] : 0.0;
      bet[3] = 0.0;
    }
    gauss_newton(w, bet);
    SP ccs = w.at(oCcs + 12 * set), v = w.at(oBasis);
    for (int q = 0; q < 12; ++q) ccs[q] = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j)
        for (int kk = 0; kk < 3; ++kk) ccs[3 * j + kk] += bet[i] * v[12 * i + 3 * j + kk];
    double pz = alpha0[0] * ccs[2] + alpha0[1] * ccs[5] + alpha0[2] * ccs[8] + alpha0[3] * ccs[11];
    if (pz < 0.0)
      for (int q = 0; q < 12; ++q) ccs[q] = -ccs[q];
  }
}

// estimate_R_and_t (:569-627) after its sums: abt (3x3) and pc0 in w; pw0 = cws[0] (the same sum).  Writes R / t of `set`.
__device__ void rotation(SP w, int set, SP abt, SP pc0) {
  SP jac = w.at(oJac), V = jac.at(25), ord = w.at(oOrd), R = w.at(oR + 9 * set), t = w.at(oT + 3 * set), cws = w.at(oCws);
  auto A = [&](int i, int c) { return abt[3 * i + c]; };
  SP B = jac;
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) {
      double s = 0.0;
      for (int i = 0; i < 3; ++i) s += A(i, a) * A(i, b);
      B[a * 3 + b] = s;
      B[b * 3 + a] = s;
    }
  jacobi(B, V, 3);
  order_abs(B, 3, ord);
  double vv[3][3], uu[3][3];
  bool has[3];
  const double lmax = fabs(B[(int)ord[2] * 4]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = (int)ord[2 - k];
    SP tmp = jac.at(56);
    canonical_col(V, 3, e, tmp);
    vv[k][0] = tmp[0]; vv[k][1] = tmp[1]; vv[k][2] = tmp[2];
    const double lk = B[e * 4];
    if (lk > kPinvCut * lmax) {
      double s = sqrt(lk);
#pragma unroll
      for (int i = 0; i < 3; ++i) uu[k][i] = (abt[3 * i] * vv[k][0] + abt[3 * i + 1] * vv[k][1] + abt[3 * i + 2] * vv[k][2]) / s;
      has[k] = true;
    } else if (k == 2 && has[0] && has[1]) {
      uu[2][0] = uu[0][1] * uu[1][2] - uu[0][2] * uu[1][1];
      uu[2][1] = uu[0][2] * uu[1][0] - uu[0][0] * uu[1][2];
      uu[2][2] = uu[0][0] * uu[1][1] - uu[0][1] * uu[1][0];
      has[k] = true;
    } else {
      uu[k][0] = uu[k][1] = uu[k][2] = 0.0;
      has[k] = false;
    }
  }
  double r[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) s += uu[k][i] * vv[k][j];
      r[i][j] = s;
    }
  const double det = r[0][0] * r[1][1] * r[2][2] + r[0][1] * r[1][2] * r[2][0] + r[0][2] * r[1][0] * r[2][1] -
                     r[0][2] * r[1][1] * r[2][0] - r[0][1] * r[1][0] * r[2][2] - r[0][0] * r[1][2] * r[2][1];
  if (det < 0) { r[2][0] = -r[2][0]; r[2][1] = -r[2][1]; r[2][2] = -r[2][2]; }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = r[i][j];
    t[i] = pc0[i] - (r[i][0] * cws[0] + r[i][1] * cws[1] + r[i][2] * cws[2]);
  }
}

// The null space of a minimal set (DEVIATION 2): fill_M (:436-452) transposed into Mt (12 x 8), its Householder QR, and
// columns 9..12 of Q as v[0..3] with canonical signs.  alpha(i, q), u(i), v(i): the 4 correspondences.
template <class FA, class FU, class FV>
__device__ void null4_qr(SP w, FA alpha, FU uu, FV vv, const PnpDesc& ds) {
  SP jac = w.at(oJac);
  SP A = w.at(oMt);
  for (int i = 0; i < 4; ++i) {
    const double u = uu(i), v = vv(i);
    for (int q = 0; q < 4; ++q) {
      const double a = alpha(i, q);
      A[(3 * q) * 8 + 2 * i] = a * ds.fu;         A[(3 * q) * 8 + 2 * i + 1] = 0.0;
      A[(3 * q + 1) * 8 + 2 * i] = 0.0;           A[(3 * q + 1) * 8 + 2 * i + 1] = a * ds.fv;
      A[(3 * q + 2) * 8 + 2 * i] = a * (ds.uc - u); A[(3 * q + 2) * 8 + 2 * i + 1] = a * (ds.vc - v);
    }
  }
  SP hb = jac;                                   // reflector scales (the Jacobi scratch is free here)
  for (int kk = 0; kk < 8; ++kk) {
    double s2 = 0.0;
    for (int i = kk; i < 12; ++i) s2 += A[i * 8 + kk] * A[i * 8 + kk];
    double sigma = sqrt(s2);
    if (A[kk * 8 + kk] < 0.0) sigma = -sigma;
    const double v0 = A[kk * 8 + kk] + sigma;
    hb[kk] = sigma * v0;
    A[kk * 8 + kk] = v0;
    if (hb[kk] == 0.0) continue;
    for (int j = kk + 1; j < 8; ++j) {
      double dd = 0.0;
      for (int i = kk; i < 12; ++i) dd += A[i * 8 + kk] * A[i * 8 + j];
      const double tau = dd / hb[kk];
      for (int i = kk; i < 12; ++i) A[i * 8 + j] = A[i * 8 + j] - tau * A[i * 8 + kk];
    }
  }
  SP basis = w.at(oBasis), y = jac.at(8);
  for (int c = 0; c < 4; ++c) {
    for (int i = 0; i < 12; ++i) y[i] = i == 8 + c ? 1.0 : 0.0;
    for (int kk = 7; kk >= 0; --kk) {
      if (hb[kk] == 0.0) continue;
      double dd = 0.0;
      for (int i = kk; i < 12; ++i) dd += A[i * 8 + kk] * y[i];
      const double tau = dd / hb[kk];
      for (int i = kk; i < 12; ++i) y[i] = y[i] - tau * A[i * 8 + kk];
    }
    int m = 0;
    for (int i = 1; i < 12; ++i) if (fabs(y[i]) > fabs(y[m])) m = i;
    const bool neg = y[m] < 0.0;
    for (int i = 0; i < 12; ++i) basis[12 * c + i] = neg ? -y[i] : y[i];
  }
}

// CheckInliers (:308-340) for one correspondence: Xc, Yc, invZc float; ue, ve double; distX, distY, error2 float.
__device__ inline bool is_inlier(const double* rt, float4 p, float2 uv, double fu, double fv, double uc, double vc) {
  const double x = p.x, y = p.y, z = p.z;
  float Xc = (float)(rt[0] * x + rt[1] * y + rt[2] * z + rt[9]);
  float Yc = (float)(rt[3] * x + rt[4] * y + rt[5] * z + rt[10]);
  float invZc = (float)(1 / (rt[6] * x + rt[7] * y + rt[8] * z + rt[11]));
  double ue = uc + fu * (double)Xc * (double)invZc;
  double ve = vc + fv * (double)Yc * (double)invZc;
  float distX = (float)((double)uv.x - ue);
  float distY = (float)((double)uv.y - ve);
  float error2 = distX * distX + distY * distY;
  return error2 < p.w;
}

struct Dev {
  const float4* pt; const float2* uv; const int32_t* kp;
  const PnpDesc* desc; PnpState* st; PnpRes* res; uint8_t* flags;
  const int32_t* hyp_off;                    // [n + 1] this call's hypothesis slots (bounds; 0 for inactive solvers)
  int32_t* idx;                              // [4 * slots]
  double* rt;                                // [12 * slots]
  HypRec* hyp;                               // [slots]
  PnpJob* job;                               // [slots + n]: solver s owns [hyp_off[s] + s, hyp_off[s + 1] + s + 1)
  double* scratch;                           // refine workgroups: [grid][8 * max_n]
  int32_t* scratch_idx;                      // [grid][max_n]
  int n, n_iterations, max_n;
  const uint8_t* live;                       // [n] device, or null: all.  A solver with live = 0 keeps its state and last results (lld_pnp_internal.h)
};

// ------------------------------------------------------------------ kernels
__global__ void pnp_sample(Dev d) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n) return;
  const int bound = d.hyp_off[s + 1] - d.hyp_off[s];
  if (bound == 0) return;                    // not active in this call
  const PnpDesc ds = d.desc[s];
  PnpState& st = d.st[s];
  if (d.live && !d.live[s]) { st.window = 0; return; }   // no hypothesis of its slots is evaluated
  // iterate (:165-258): N < mRansacMinInliers -> bNoMore with no draws; else the loop runs while mnIterations < budget or
  // fewer than n this call, i.e. max(n, budget - mnIterations) iterations unless a Refine succeeds first.
  const int n_it = d.n_iterations > 0 ? d.n_iterations : ds.max_its;   // 0: find(), iterate(mRansacMaxIts)
  int W = ds.n < ds.min_inliers ? 0 : max(n_it, ds.max_its - st.n_iter);
  if (W > bound) W = bound;                  // cannot happen: bound = max(n_it, mRansacMaxIts)
  st.window = W;
  st.rng.save();                             // ring is advanced in place; pnp_resolve rewinds it to the saved one + the draws made
  int32_t head = st.rng.head;
  int32_t* out = d.idx + 4 * d.hyp_off[s];
  for (int k = 0; k < W; ++k) draw_set<4>(st.rng.ring, head, ds.n, out + 4 * k);
}

// EPnP on the 4 correspondences of one hypothesis (compute_pose :477-525), scratch lane-interleaved in dynamic LDS.
__global__ __launch_bounds__(kHypLanes) void pnp_hyp(Dev d, int n_slots) {
  extern __shared__ double lds[];
  const int g = blockIdx.x * kHypLanes + threadIdx.x;
  if (g >= n_slots) return;
  const int s = solver_of(d.hyp_off, d.n, g);
  const int k = g - d.hyp_off[s];
  if (k >= d.st[s].window) return;
  const PnpDesc ds = d.desc[s];
  SP w{lds + threadIdx.x, kHypLanes};
  SP pws = w.at(oPts), us = w.at(oPts + 12), al = w.at(oPts + 20), cws = w.at(oCws), jac = w.at(oJac);
  for (int i = 0; i < 4; ++i) {              // add_correspondence (:363-373)
    const int j = ds.off + d.idx[4 * g + i];
    const float4 p = d.pt[j]; const float2 u = d.uv[j];
    pws[3 * i] = p.x; pws[3 * i + 1] = p.y; pws[3 * i + 2] = p.z;
    us[2 * i] = u.x; us[2 * i + 1] = u.y;
  }
  for (int j = 0; j < 3; ++j) {
    double c = 0;
    for (int i = 0; i < 4; ++i) c += pws[3 * i + j];
    cws[j] = c / 4;
  }
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) {
      double s2 = 0.0;
      for (int i = 0; i < 4; ++i) s2 += (pws[3 * i + a] - cws[a]) * (pws[3 * i + b] - cws[b]);
      jac[3 * a + b] = s2; jac[3 * b + a] = s2;
    }
  control_points(w, 4);
  SP ci = w.at(oCi);
  for (int i = 0; i < 4; ++i) {
    double d0 = pws[3 * i] - cws[0], d1 = pws[3 * i + 1] - cws[1], d2 = pws[3 * i + 2] - cws[2];
    for (int j = 0; j < 3; ++j) al[4 * i + 1 + j] = ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2;
    al[4 * i] = 1.0 - al[4 * i + 1] - al[4 * i + 2] - al[4 * i + 3];
  }
  auto alpha = [&](int i, int q) { return al[4 * i + q]; };
  auto uu = [&](int i) { return us[2 * i]; };
  auto vv = [&](int i) { return us[2 * i + 1]; };
  null4_qr(w, alpha, uu, vv, ds);
  fill_L_rho(w);
  const double a0[4] = {al[0], al[1], al[2], al[3]};
  betas_and_ccs(w, a0);
  double best_err = 0.0;
  int best = 0;
  for (int set = 0; set < 3; ++set) {        // compute_R_and_t (:636-665) per beta set
    SP ccs = w.at(oCcs + 12 * set), abt = w.at(oAbt), pc0 = w.at(oPc0);
    double pcs[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        pcs[i][j] = al[4 * i] * ccs[j] + al[4 * i + 1] * ccs[3 + j] + al[4 * i + 2] * ccs[6 + j] + al[4 * i + 3] * ccs[9 + j];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double c = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) c += pcs[i][j];
      pc0[j] = c / 4;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double s2 = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) s2 += (pcs[i][j] - pc0[j]) * (pws[3 * i + c] - cws[c]);
        abt[3 * j + c] = s2;
      }
    rotation(w, set, abt, pc0);
    SP R = w.at(oR + 9 * set), t = w.at(oT + 3 * set);
    double sum2 = 0.0;                       // reprojection_error (:546-567)
    for (int i = 0; i < 4; ++i) {
      const double px = pws[3 * i], py = pws[3 * i + 1], pz = pws[3 * i + 2];
      const double Xc = R[0] * px + R[1] * py + R[2] * pz + t[0];
      const double Yc = R[3] * px + R[4] * py + R[5] * pz + t[1];
      const double iz = 1.0 / (R[6] * px + R[7] * py + R[8] * pz + t[2]);
      const double ue = ds.uc + ds.fu * Xc * iz, ve = ds.vc + ds.fv * Yc * iz;
      const double u = us[2 * i], v = us[2 * i + 1];
      sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    const double err = sum2 / 4;
    if (set == 0 || err < best_err) { best_err = err; best = set; }
  }
  double* out = d.rt + 12 * (size_t)g;
  for (int q = 0; q < 9; ++q) out[q] = w[oR + 9 * best + q];
  for (int q = 0; q < 3; ++q) out[9 + q] = w[oT + 3 * best + q];
}

// One wavefront per hypothesis slot: CheckInliers' count.
__global__ __launch_bounds__(256) void pnp_count(Dev d, int n_slots) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_slots) return;
  const int s = solver_of(d.hyp_off, d.n, g);
  if (g - d.hyp_off[s] >= d.st[s].window) return;
  const PnpDesc ds = d.desc[s];
  double rt[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) rt[q] = d.rt[12 * (size_t)g + q];
  const int cnt = wave_count(ds.n, [&](int i) {
    return is_inlier(rt, d.pt[ds.off + i], d.uv[ds.off + i], ds.fu, ds.fv, ds.uc, ds.vc);
  });
  if ((threadIdx.x & 63) == 0) d.hyp[g] = HypRec{cnt, 0, -1, 0};
}

// One lane per solver: records (strict increases of the count among eligible hypotheses) and the Refine each eligible
// hypothesis would run: the one of its best-so-far set.
__global__ void pnp_records(Dev d) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n) return;
  const int h0 = d.hyp_off[s];
  if (d.hyp_off[s + 1] == h0) {              // not active: its one job slot is empty
    d.job[h0 + s].solver = -1;
    return;
  }
  if (d.live && !d.live[s]) {                // its slots were laid out, none of its jobs exists
    for (int q = 0; q < d.hyp_off[s + 1] - h0 + 1; ++q) d.job[h0 + s + q].solver = -1;
    return;
  }
  PnpState& st = d.st[s];
  const PnpDesc ds = d.desc[s];
  const int j0 = h0 + s;
  int nj = 0;
  int best = st.best, cur = -1;
  st.carried_job = -1;
  if (best >= ds.min_inliers && best > 0) {  // the best set of an earlier call
    PnpJob& j = d.job[j0 + nj];
    j.solver = s; j.hyp = -1; j.ok = -1;
    cur = j0 + nj; st.carried_job = cur; ++nj;
  }
  for (int k = 0; k < st.window; ++k) {
    HypRec& h = d.hyp[h0 + k];
    if (h.n_inliers >= ds.min_inliers) {
      if (h.n_inliers > best) {
        best = h.n_inliers;
        PnpJob& j = d.job[j0 + nj];
        j.solver = s; j.hyp = h0 + k; j.ok = -1;
        cur = j0 + nj; ++nj;
        h.record = 1;
      }
      h.job = cur;
    }
  }
  for (int q = nj; q < d.hyp_off[s + 1] - h0 + 1; ++q) d.job[j0 + q].solver = -1;
}

// Refine (:260-306): EPnP on the record's inliers in ascending order, then CheckInliers; ok when the count is > mRansacMinInliers.
__global__ __launch_bounds__(kThreads) void pnp_refine(Dev d, int n_jobs) {
  __shared__ double w_[kEpnpCore];
  __shared__ double mtm[144], vv[144];
  __shared__ double rt_sh[12];
  __shared__ int cnt_sh[kThreads / 64 + 1], n_sel_sh;
  __shared__ int wave_base[kThreads];
  SP w{w_, 1};
  double* al = d.scratch + (size_t)blockIdx.x * 8 * d.max_n;          // alphas[4 n]
  double* term = al + 4 * (size_t)d.max_n;                              // per-point terms [3 n] (+ n spare)
  int32_t* sel = d.scratch_idx + (size_t)blockIdx.x * d.max_n;
  const int tid = threadIdx.x;
  for (int jb = blockIdx.x; jb < n_jobs; jb += gridDim.x) {
    PnpJob& job = d.job[jb];
    if (job.solver < 0) continue;            // uniform over the block
    const int s = job.solver;
    const PnpDesc ds = d.desc[s];
    if (tid < 12) rt_sh[tid] = job.hyp < 0 ? d.st[s].best_rt[tid] : d.rt[12 * (size_t)job.hyp + tid];
    __syncthreads();
    // mvbBestInliers: the record's CheckInliers, compacted in ascending order
    {
      double rt[12];
      for (int q = 0; q < 12; ++q) rt[q] = rt_sh[q];
      const int chunk = (ds.n + kThreads - 1) / kThreads, b0 = min(ds.n, tid * chunk), b1 = min(ds.n, b0 + chunk);
      int c = 0;
      for (int i = b0; i < b1; ++i) c += is_inlier(rt, d.pt[ds.off + i], d.uv[ds.off + i], ds.fu, ds.fv, ds.uc, ds.vc);
      wave_base[tid] = c;
      __syncthreads();
      if (tid == 0) {
        int a = 0;
        for (int t = 0; t < kThreads; ++t) { int x = wave_base[t]; wave_base[t] = a; a += x; }
        n_sel_sh = a;
      }
      __syncthreads();
      int o = wave_base[tid];
      for (int i = b0; i < b1; ++i)
        if (is_inlier(rt, d.pt[ds.off + i], d.uv[ds.off + i], ds.fu, ds.fv, ds.uc, ds.vc)) sel[o++] = i;
      __syncthreads();
    }
    const int n = n_sel_sh;
    const int off = ds.off;
    // choose_control_points: centroid and PW0^T PW0, one lane per sum
    if (tid < 3) {
      double c = 0;
      for (int i = 0; i < n; ++i) c += (double)(&d.pt[off + sel[i]].x)[tid];
      w[oCws + tid] = c / n;
    }
    __syncthreads();
    if (tid < 9) {
      const int a = tid / 3, b = tid % 3;
      if (a <= b) {
        double s2 = 0.0;
        for (int i = 0; i < n; ++i) {
          const float4 p = d.pt[off + sel[i]];
          const double pa = (double)(&p.x)[a] - w[oCws + a], pb = (double)(&p.x)[b] - w[oCws + b];
          s2 += pa * pb;
        }
        w[oJac + 3 * a + b] = s2; w[oJac + 3 * b + a] = s2;
      }
    }
    __syncthreads();
    if (tid == 0) control_points(w, n);
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {  // compute_barycentric_coordinates
      const float4 p = d.pt[off + sel[i]];
      const double d0 = (double)p.x - w[oCws], d1 = (double)p.y - w[oCws + 1], d2 = (double)p.z - w[oCws + 2];
      double a[4];
      for (int j = 0; j < 3; ++j) a[1 + j] = w[oCi + 3 * j] * d0 + w[oCi + 3 * j + 1] * d1 + w[oCi + 3 * j + 2] * d2;
      a[0] = 1.0 - a[1] - a[2] - a[3];
      for (int j = 0; j < 4; ++j) al[4 * (size_t)i + j] = a[j];
    }
    __syncthreads();
    // cvMulTransposed(M): one lane per entry of the upper triangle, rows in order (2i, 2i + 1)
    if (tid < 144) {
      const int a = tid / 12, b = tid % 12;
      if (a <= b) {
        const int qa = a / 3, ca = a % 3, qb = b / 3, cb = b % 3;
        double s2 = 0.0;
        for (int i = 0; i < n; ++i) {
          const float2 u = d.uv[off + sel[i]];
          const double aa = al[4 * (size_t)i + qa], ab = al[4 * (size_t)i + qb];
          const double m1a = ca == 0 ? aa * ds.fu : (ca == 1 ? 0.0 : aa * (ds.uc - (double)u.x));
          const double m1b = cb == 0 ? ab * ds.fu : (cb == 1 ? 0.0 : ab * (ds.uc - (double)u.x));
          const double m2a = ca == 0 ? 0.0 : (ca == 1 ? aa * ds.fv : aa * (ds.vc - (double)u.y));
          const double m2b = cb == 0 ? 0.0 : (cb == 1 ? ab * ds.fv : ab * (ds.vc - (double)u.y));
          s2 += m1a * m1b;
          s2 += m2a * m2b;
        }
        mtm[a * 12 + b] = s2; mtm[b * 12 + a] = s2;
      }
    }
    __syncthreads();
    if (tid == 0) {                          // the basis (DEVIATION 2), then the betas
      if (n == 4) {                          // a best set of exactly 4: the minimal-set QR basis, as for a hypothesis
        auto alpha = [&](int i, int q) { return al[4 * (size_t)i + q]; };
        auto uu = [&](int i) { return (double)d.uv[off + sel[i]].x; };
        auto vv_ = [&](int i) { return (double)d.uv[off + sel[i]].y; };
        null4_qr(w, alpha, uu, vv_, ds);
      } else {                               // 12x12 Jacobi: distinct eigenvalues
        SP A{mtm, 1}, V{vv, 1}, ord = w.at(oOrd);
        jacobi(A, V, 12);
        order_abs(A, 12, ord);
        for (int i = 0; i < 4; ++i) canonical_col(V, 12, (int)ord[i], w.at(oBasis + 12 * i));
      }
      fill_L_rho(w);
      const double a0[4] = {al[0], al[1], al[2], al[3]};
      betas_and_ccs(w, a0);
    }
    __syncthreads();
    // compute_R_and_t for the three beta sets: pc0 (9 lanes), abt (27 lanes), then R / t, then the reprojection sums
    if (tid < 9) {
      const int set = tid / 3, j = tid % 3;
      const double* c = &w_[oCcs + 12 * set];
      double s2 = 0.0;
      for (int i = 0; i < n; ++i) {
        const double* a = al + 4 * (size_t)i;
        s2 += a[0] * c[j] + a[1] * c[3 + j] + a[2] * c[6 + j] + a[3] * c[9 + j];
      }
      vv[tid] = s2 / n;                      // pc0 of the set (the eigenvectors are in the basis by now)
    }
    __syncthreads();
    if (tid < 27) {
      const int set = tid / 9, j = (tid % 9) / 3, cc = tid % 3;
      const double* c = &w_[oCcs + 12 * set];
      double s2 = 0.0;
      for (int i = 0; i < n; ++i) {
        const double* a = al + 4 * (size_t)i;
        const double pc = a[0] * c[j] + a[1] * c[3 + j] + a[2] * c[6 + j] + a[3] * c[9 + j];
        const double pw = (double)(&d.pt[off + sel[i]].x)[cc];
        s2 += (pc - vv[3 * set + j]) * (pw - w[oCws + cc]);
      }
      mtm[tid] = s2;                         // abt of the three sets (M^T M is no longer needed)
    }
    __syncthreads();
    if (tid == 0)
      for (int set = 0; set < 3; ++set) {
        SP abt{mtm + 9 * set, 1}, pc0{vv + 3 * set, 1};
        rotation(w, set, abt, pc0);
      }
    __syncthreads();
    for (int i = tid; i < n; i += kThreads) {
      const float4 p = d.pt[off + sel[i]];
      const float2 u = d.uv[off + sel[i]];
      const double px = p.x, py = p.y, pz = p.z;
      for (int set = 0; set < 3; ++set) {
        const double* R = &w_[oR + 9 * set];
        const double* t = &w_[oT + 3 * set];
        const double Xc = R[0] * px + R[1] * py + R[2] * pz + t[0];
        const double Yc = R[3] * px + R[4] * py + R[5] * pz + t[1];
        const double iz = 1.0 / (R[6] * px + R[7] * py + R[8] * pz + t[2]);
        const double ue = ds.uc + ds.fu * Xc * iz, ve = ds.vc + ds.fv * Yc * iz;
        term[3 * (size_t)i + set] = sqrt(((double)u.x - ue) * ((double)u.x - ue) + ((double)u.y - ve) * ((double)u.y - ve));
      }
    }
    __syncthreads();
    if (tid < 3) {
      double s2 = 0.0;
      for (int i = 0; i < n; ++i) s2 += term[3 * (size_t)i + tid];
      vv[9 + tid] = s2 / n;
    }
    __syncthreads();
    if (tid == 0) {
      int b = 0;
      if (vv[10] < vv[9]) b = 1;
      if (vv[11] < vv[9 + b]) b = 2;
      for (int q = 0; q < 9; ++q) rt_sh[q] = w_[oR + 9 * b + q];
      for (int q = 0; q < 3; ++q) rt_sh[9 + q] = w_[oT + 3 * b + q];
    }
    __syncthreads();
    {
      double rt[12];
      for (int q = 0; q < 12; ++q) rt[q] = rt_sh[q];
      int c = 0;
      for (int i = tid; i < ds.n; i += kThreads) c += is_inlier(rt, d.pt[ds.off + i], d.uv[ds.off + i], ds.fu, ds.fv, ds.uc, ds.vc);
      c = lld_wave::sum(c);
      if ((tid & 63) == 0) cnt_sh[tid >> 6] = c;
      __syncthreads();
      if (tid == 0) {
        int tot = 0;
        for (int q = 0; q < kThreads / 64; ++q) tot += cnt_sh[q];
        job.n_inliers = tot;
        job.ok = tot > ds.min_inliers ? 1 : 0;
        for (int q = 0; q < 12; ++q) job.rt[q] = rt[q];
      }
      __syncthreads();
    }
  }
}

// One workgroup per solver: iterate()'s order replayed over the window.
__global__ __launch_bounds__(kThreads) void pnp_resolve(Dev d) {
  const int s = blockIdx.x;
  const int h0 = d.hyp_off[s];
  if (d.hyp_off[s + 1] == h0) return;        // not active
  if (d.live && !d.live[s]) return;
  __shared__ double rt_sh[12];
  __shared__ int mode_sh;                    // 0: no pose, 1: refined (job rt), 2: best
  const PnpDesc ds = d.desc[s];
  PnpState& st = d.st[s];
  PnpRes& res = d.res[s];
  const int tid = threadIdx.x;
  if (tid == 0) {
    int mode = 0, run = st.window, n_in = 0;
    for (int k = 0; k < st.window; ++k) {
      HypRec& h = d.hyp[h0 + k];
      if (h.job < 0) continue;
      if (h.record) {                        // mvbBestInliers, mnBestInliers, mBestTcw
        st.best = h.n_inliers;
        const double* rt = d.rt + 12 * (size_t)(h0 + k);
        for (int q = 0; q < 12; ++q) { st.best_rt[q] = rt[q]; st.best_tcw[q] = (float)rt[q]; }
      }
      const PnpJob& j = d.job[h.job];
      if (j.ok == 1) {
        mode = 1; run = k + 1; n_in = j.n_inliers;
        for (int q = 0; q < 12; ++q) rt_sh[q] = j.rt[q];
        break;
      }
    }
    st.run = run;
    st.n_iter += run;
    int no_more = 0;
    if (ds.n < ds.min_inliers) {
      no_more = 1;
    } else if (mode == 0 && st.n_iter >= ds.max_its) {
      no_more = 1;
      if (st.best >= ds.min_inliers) {
        mode = 2; n_in = st.best;
        for (int q = 0; q < 12; ++q) rt_sh[q] = st.best_rt[q];
      }
    }
    res.has_pose = mode != 0;
    res.n_inliers = n_in;
    res.no_more = no_more;
    res.iterations = st.n_iter;
    res.best_inliers = st.best;
    for (int q = 0; q < 12; ++q)
      res.tcw[q] = mode == 0 ? 0.0f : (mode == 1 ? (float)rt_sh[(q % 4) == 3 ? 9 + q / 4 : 3 * (q / 4) + q % 4]
                                                 : st.best_tcw[(q % 4) == 3 ? 9 + q / 4 : 3 * (q / 4) + q % 4]);
    mode_sh = mode;
    st.rng.rewind(4 * run);                  // the stream after the draws made: 4 per iteration run
  }
  __syncthreads();
  double rt[12];                             // read only when a pose is returned
  for (int q = 0; q < 12; ++q) rt[q] = rt_sh[q];
  scatter_inliers<kThreads>(d.flags + ds.kp_off, ds.n_kp, mode_sh != 0, d.kp + ds.off, ds.n, [&](int i) {
    return is_inlier(rt, d.pt[ds.off + i], d.uv[ds.off + i], ds.fu, ds.fv, ds.uc, ds.vc);
  });
}

}  // namespace

// ------------------------------------------------------------------ host side
struct lld_pnp_batch {
  lld_ctx* ctx = nullptr;
  int n = 0, max_n = 0, max_its_all = 0;
  std::vector<PnpDesc> desc;
  std::vector<int32_t> kp_off;
  int64_t n_kp_total = 0;
  void* dmem = nullptr;                      // points, descriptors, state, results, flags
  void* dcall = nullptr; size_t dcall_bytes = 0;
  Dev dev{};
  int last_slots = 0;
  std::vector<int32_t> last_off;             // this call's hyp_off (host copy)
  int grid_refine = 0;
};

extern "C" void lld_pnp_params_default(lld_pnp_params* p) {
  if (!p) return;
  p->probability = 0.99; p->min_inliers = 10; p->max_iterations = 300; p->min_set = 4; p->epsilon = 0.5f; p->th2 = 5.991f;
}

static int pnp_check_problem(const lld_pnp_problem& q) {
  if (q.n < 0 || q.n_keypoints < 0) return LLD_ERR_INVALID;
  if (q.n > LLD_PNP_MAX_CORRESPONDENCES || q.n_keypoints > LLD_PNP_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  if (q.n > 0 && (!q.xyz || !q.uv || !q.sigma2 || !q.kp_index)) return LLD_ERR_INVALID;
  if (!(q.fx > 0.0f) || !(q.fy > 0.0f)) return LLD_ERR_INVALID;
  return indices_unique_in_range(q.kp_index, q.n, q.n_keypoints) ? LLD_OK : LLD_ERR_INVALID;
}

static int pnp_check_params(const lld_pnp_params& p) {
  if (p.min_set != 4) return LLD_ERR_UNSUPPORTED;
  if (p.max_iterations < 1 || p.max_iterations > LLD_PNP_MAX_ITERATIONS) return LLD_ERR_INVALID;
  if (!(p.probability > 0.0 && p.probability < 1.0) || !(p.epsilon > 0.0f && p.epsilon <= 1.0f) || !(p.th2 > 0.0f)) return LLD_ERR_INVALID;
  return LLD_OK;
}

static int pnp_upload(lld_pnp_batch* b, const lld_pnp_problem* problems, const lld_pnp_params* params, std::vector<PnpState>& st,
                      int64_t ntot);
static int pnp_alloc(lld_pnp_batch* b, std::vector<PnpState>& st, int64_t ntot);

// SetRansacParameters (:121-157), literally, and the solver's stream: what the constructor and SetRansacParameters leave besides the correspondences
static void pnp_describe(lld_pnp_batch* b, int s, int N, int n_keypoints, float fx, float fy, float cx, float cy, uint32_t seed, const lld_pnp_params* params,
                         int64_t* ntot, PnpState* st) {
  PnpDesc& ds = b->desc[s];
  std::memset(&ds, 0, sizeof(ds));
  ds.off = (int32_t)*ntot; ds.n = N; ds.n_kp = n_keypoints; ds.kp_off = (int32_t)b->n_kp_total;
  b->kp_off[s] = ds.kp_off;
  const float eps0 = params->epsilon;
  int nMinInliers = N * eps0;                                   // float product, truncated
  if (nMinInliers < params->min_inliers) nMinInliers = params->min_inliers;
  if (nMinInliers < params->min_set) nMinInliers = params->min_set;
  float eps = eps0;
  if (N > 0 && eps < (float)nMinInliers / N) eps = (float)nMinInliers / N;
  ds.min_inliers = nMinInliers;
  ds.max_its = ransac_max_iterations(params->probability, eps, nMinInliers, N, params->max_iterations);
  ds.fu = fx; ds.fv = fy; ds.uc = cx; ds.vc = cy;
  std::memset(st, 0, sizeof(PnpState));
  srand_state(seed, st->rng.ring, &st->rng.head);
  st->carried_job = -1;
  *ntot += N;
  b->n_kp_total += n_keypoints;
  b->max_n = std::max(b->max_n, N);
  b->max_its_all = std::max(b->max_its_all, ds.max_its);
}

extern "C" int lld_pnp_batch_create(lld_ctx* ctx, int32_t n, const lld_pnp_problem* problems, const lld_pnp_params* params,
                                    lld_pnp_batch** out) {
  if (!ctx || !problems || !params || !out || n < 1) return LLD_ERR_INVALID;
  *out = nullptr;
  if (n > LLD_PNP_MAX_SOLVERS) return LLD_ERR_UNSUPPORTED;
  if (int st = pnp_check_params(*params)) return st;
  for (int s = 0; s < n; ++s)
    if (int st = pnp_check_problem(problems[s])) return st;
  auto* b = new lld_pnp_batch();
  b->ctx = ctx; b->n = n;
  b->desc.resize(n); b->kp_off.resize(n);
  int64_t ntot = 0;
  std::vector<PnpState> st(n);
  for (int s = 0; s < n; ++s) {
    const lld_pnp_problem& q = problems[s];
    pnp_describe(b, s, q.n, q.n_keypoints, q.fx, q.fy, q.cx, q.cy, q.seed, params, &ntot, &st[s]);
  }
  if (int rc = pnp_upload(b, problems, params, st, ntot)) {   // nothing half-built survives a failure
    lld_pnp_batch_destroy(b);
    return rc;
  }
  *out = b;
  return LLD_OK;
}

static int pnp_upload(lld_pnp_batch* b, const lld_pnp_problem* problems, const lld_pnp_params* params, std::vector<PnpState>& st,
                      int64_t ntot) {
  lld_ctx* ctx = b->ctx;
  const int n = b->n;
  std::vector<float4> pt(ntot);
  std::vector<float2> uv(ntot);
  std::vector<int32_t> kp(ntot);
  for (int s = 0; s < n; ++s) {
    const lld_pnp_problem& q = problems[s];
    const int64_t o = b->desc[s].off;
    for (int i = 0; i < q.n; ++i) {
      pt[o + i] = make_float4(q.xyz[3 * i], q.xyz[3 * i + 1], q.xyz[3 * i + 2], q.sigma2[i] * params->th2);   // mvMaxError (float)
      uv[o + i] = make_float2(q.uv[2 * i], q.uv[2 * i + 1]);
      kp[o + i] = q.kp_index[i];
    }
  }
  if (int rc = pnp_alloc(b, st, ntot)) return rc;
  hipStream_t stream = ctx->stream;
  const Dev& d = b->dev;
  if (ntot) {
    LLD_HIP_TRY(hipMemcpyAsync((void*)d.pt, pt.data(), sizeof(float4) * ntot, hipMemcpyHostToDevice, stream));
    LLD_HIP_TRY(hipMemcpyAsync((void*)d.uv, uv.data(), sizeof(float2) * ntot, hipMemcpyHostToDevice, stream));
    LLD_HIP_TRY(hipMemcpyAsync((void*)d.kp, kp.data(), sizeof(int32_t) * ntot, hipMemcpyHostToDevice, stream));
    LLD_HIP_TRY(hipStreamSynchronize(stream));                  // (the staging vectors are this function's)
  }
  return LLD_OK;
}

// The batch's slab and everything in it but the correspondences: descriptors, streams, zeroed results and flags.
static int pnp_alloc(lld_pnp_batch* b, std::vector<PnpState>& st, int64_t ntot) {
  lld_ctx* ctx = b->ctx;
  const int n = b->n;
  size_t bytes = lld_slab::pad(sizeof(float4) * std::max<int64_t>(ntot, 1)) + lld_slab::pad(sizeof(float2) * std::max<int64_t>(ntot, 1)) +
                 lld_slab::pad(sizeof(int32_t) * std::max<int64_t>(ntot, 1)) + lld_slab::pad(sizeof(PnpDesc) * n) +
                 lld_slab::pad(sizeof(PnpState) * n) + lld_slab::pad(sizeof(PnpRes) * n) + lld_slab::pad(std::max<int64_t>(b->n_kp_total, 1));
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&b->dmem, bytes) != hipSuccess) { b->dmem = nullptr; return LLD_ERR_ALLOC; }
  lld_slab sl; sl.base = (char*)b->dmem; sl.size = bytes;
  Dev& d = b->dev;
  d.pt = sl.take<float4>(std::max<int64_t>(ntot, 1));
  d.uv = sl.take<float2>(std::max<int64_t>(ntot, 1));
  d.kp = sl.take<int32_t>(std::max<int64_t>(ntot, 1));
  d.desc = sl.take<PnpDesc>(n);
  d.st = sl.take<PnpState>(n);
  d.res = sl.take<PnpRes>(n);
  d.flags = sl.take<uint8_t>(std::max<int64_t>(b->n_kp_total, 1));
  d.n = n; d.max_n = std::max(b->max_n, 1);
  hipStream_t stream = ctx->stream;
  std::vector<PnpRes> res(n);
  std::memset(res.data(), 0, sizeof(PnpRes) * n);
  LLD_HIP_TRY(hipMemcpyAsync((void*)d.desc, b->desc.data(), sizeof(PnpDesc) * n, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemcpyAsync(d.st, st.data(), sizeof(PnpState) * n, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemcpyAsync(d.res, res.data(), sizeof(PnpRes) * n, hipMemcpyHostToDevice, stream));
  LLD_HIP_TRY(hipMemsetAsync(d.flags, 0, std::max<int64_t>(b->n_kp_total, 1), stream));
  LLD_HIP_TRY(hipStreamSynchronize(stream));
  LLD_HIP_TRY(hipFuncSetAttribute((const void*)pnp_hyp, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)(sizeof(double) * kHypScratch * kHypLanes)));
  return LLD_OK;
}

extern "C" void lld_pnp_batch_destroy(lld_pnp_batch* b) {
  if (!b) return;
  if (b->ctx) (void)hipSetDevice(b->ctx->device);
  if (b->dmem) (void)hipFree(b->dmem);
  if (b->dcall) (void)hipFree(b->dcall);
  delete b;
}

// iterate(n_iterations) on the active solvers; n_iterations = 0: each solver's own mRansacMaxIts (find()).
static int pnp_iterate(lld_pnp_batch* b, int32_t n_iterations, const uint8_t* active, const uint8_t* live_d = nullptr) {
  LLD_HIP_TRY(hipSetDevice(b->ctx->device));
  const int n = b->n;
  const std::vector<int32_t> off = ransac_call_offsets(n, active, [&](int s) { return std::max(n_iterations, b->desc[s].max_its); });
  const int slots = off[n];
  // the previous call's hypotheses stay readable only until this call touches the per-call buffers
  b->last_off.clear();
  b->last_slots = 0;
  if (slots == 0) { b->last_off = off; return LLD_OK; }
  const int grid_refine = std::min(std::max(b->ctx->n_cu, 1), slots + n);
  size_t need = lld_slab::pad(sizeof(int32_t) * (n + 1)) + lld_slab::pad(sizeof(int32_t) * 4 * (size_t)slots) +
                lld_slab::pad(sizeof(double) * 12 * (size_t)slots) + lld_slab::pad(sizeof(HypRec) * (size_t)slots) +
                lld_slab::pad(sizeof(PnpJob) * ((size_t)slots + n)) + lld_slab::pad(sizeof(double) * 8 * (size_t)grid_refine * b->dev.max_n) +
                lld_slab::pad(sizeof(int32_t) * (size_t)grid_refine * b->dev.max_n);
  if (int rc = lld_grow_device(&b->dcall, &b->dcall_bytes, need)) {
    if (rc == LLD_ERR_ALLOC) b->dev.hyp_off = nullptr;
    return rc;
  }
  lld_slab sl; sl.base = (char*)b->dcall; sl.size = need;
  Dev d = b->dev;
  int32_t* hoff = sl.take<int32_t>(n + 1);
  d.hyp_off = hoff;
  d.idx = sl.take<int32_t>(4 * (size_t)slots);
  d.rt = sl.take<double>(12 * (size_t)slots);
  d.hyp = sl.take<HypRec>(slots);
  d.job = sl.take<PnpJob>((size_t)slots + n);
  d.scratch = sl.take<double>(8 * (size_t)grid_refine * d.max_n);
  d.scratch_idx = sl.take<int32_t>((size_t)grid_refine * d.max_n);
  d.n_iterations = n_iterations;
  d.live = live_d;
  b->dev = d;
  b->grid_refine = grid_refine;
  hipStream_t stream = b->ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(hoff, off.data(), sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice, stream));
  pnp_sample<<<(n + 63) / 64, 64, 0, stream>>>(d);
  pnp_hyp<<<(slots + kHypLanes - 1) / kHypLanes, kHypLanes, sizeof(double) * kHypScratch * kHypLanes, stream>>>(d, slots);
  pnp_count<<<(slots + 3) / 4, 256, 0, stream>>>(d, slots);
  pnp_records<<<(n + 63) / 64, 64, 0, stream>>>(d);
  pnp_refine<<<grid_refine, kThreads, 0, stream>>>(d, slots + n);
  pnp_resolve<<<n, kThreads, 0, stream>>>(d);
  LLD_HIP_TRY(hipGetLastError());
  b->last_off = off;
  b->last_slots = slots;
  return LLD_OK;
}

extern "C" int lld_pnp_batch_iterate(lld_pnp_batch* b, int32_t n_iterations, const uint8_t* active) {
  if (!b) return LLD_ERR_INVALID;
  if (n_iterations < 1) return LLD_ERR_INVALID;
  if (n_iterations > LLD_PNP_MAX_ITERATIONS) return LLD_ERR_UNSUPPORTED;
  return pnp_iterate(b, n_iterations, active);
}

namespace lld_pnp {

int batch_create_dev(lld_ctx* ctx, int32_t n, const int32_t* n_corr, int32_t n_keypoints, float fx, float fy, float cx, float cy, const uint32_t* seed,
                     const lld_pnp_params* params, lld_pnp_batch** out, SlabDev* slab, int32_t* off) {
  if (!ctx || !n_corr || !seed || !params || !out || !slab || !off || n < 1) return LLD_ERR_INVALID;
  *out = nullptr;
  if (n > LLD_PNP_MAX_SOLVERS || n_keypoints > LLD_PNP_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  if (int st = pnp_check_params(*params)) return st;
  if (n_keypoints < 0 || !(fx > 0.0f) || !(fy > 0.0f)) return LLD_ERR_INVALID;
  for (int s = 0; s < n; ++s) if (n_corr[s] < 0 || n_corr[s] > n_keypoints) return LLD_ERR_INVALID;
  auto* b = new lld_pnp_batch();
  b->ctx = ctx; b->n = n;
  b->desc.resize(n); b->kp_off.resize(n);
  int64_t ntot = 0;
  std::vector<PnpState> st(n);
  for (int s = 0; s < n; ++s) pnp_describe(b, s, n_corr[s], n_keypoints, fx, fy, cx, cy, seed[s], params, &ntot, &st[s]);
  if (int rc = pnp_alloc(b, st, ntot)) { lld_pnp_batch_destroy(b); return rc; }
  for (int s = 0; s < n; ++s) off[s] = b->desc[s].off;
  slab->pt = const_cast<float4*>(b->dev.pt); slab->uv = const_cast<float2*>(b->dev.uv); slab->kp = const_cast<int32_t*>(b->dev.kp);
  *out = b;
  return LLD_OK;
}

int batch_iterate_live(lld_pnp_batch* b, int32_t n_iterations, const uint8_t* live_d) {
  if (!b || n_iterations < 1) return LLD_ERR_INVALID;
  if (n_iterations > LLD_PNP_MAX_ITERATIONS) return LLD_ERR_UNSUPPORTED;
  return pnp_iterate(b, n_iterations, nullptr, live_d);
}

const PnpRes* batch_results_dev(const lld_pnp_batch* b) { return b->dev.res; }
const uint8_t* batch_flags_dev(const lld_pnp_batch* b, int32_t solver) { return b->dev.flags + b->kp_off[solver]; }

}  // namespace lld_pnp

extern "C" int lld_pnp_batch_find(lld_pnp_batch* b, const uint8_t* active) {
  if (!b) return LLD_ERR_INVALID;
  return pnp_iterate(b, 0, active);
}

extern "C" int lld_pnp_batch_download(lld_pnp_batch* b, lld_pnp_result* outs) {
  if (!b || !outs) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t stream = b->ctx->stream;
  std::vector<PnpRes> res(b->n);
  std::vector<uint8_t> flags(std::max<int64_t>(b->n_kp_total, 1));
  LLD_HIP_TRY(hipMemcpyAsync(res.data(), b->dev.res, sizeof(PnpRes) * b->n, hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipMemcpyAsync(flags.data(), b->dev.flags, flags.size(), hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipStreamSynchronize(stream));
  for (int s = 0; s < b->n; ++s) {
    lld_pnp_result& o = outs[s];
    const PnpRes& r = res[s];
    for (int q = 0; q < 12; ++q) o.Tcw[q] = r.tcw[q];
    o.has_pose = r.has_pose; o.n_inliers = r.n_inliers; o.no_more = r.no_more; o.iterations = r.iterations;
    o.best_inliers = r.best_inliers; o.n_keypoints = b->desc[s].n_kp;
    if (o.inlier) std::memcpy(o.inlier, flags.data() + b->kp_off[s], b->desc[s].n_kp);
  }
  return LLD_OK;
}

extern "C" int lld_pnp_batch_hypotheses(lld_pnp_batch* b, int32_t solver, int32_t capacity, lld_pnp_hypothesis* out,
                                        int32_t* n_window, int32_t* n_run) {
  if (!b || solver < 0 || solver >= b->n || capacity < 0 || (capacity > 0 && !out) || !n_window || !n_run) return LLD_ERR_INVALID;
  *n_window = 0; *n_run = 0;
  if (b->last_off.empty() || b->last_off[solver + 1] == b->last_off[solver]) return LLD_OK;
  LLD_HIP_TRY(hipSetDevice(b->ctx->device));
  hipStream_t stream = b->ctx->stream;
  PnpState st;
  LLD_HIP_TRY(hipMemcpyAsync(&st, b->dev.st + solver, sizeof(PnpState), hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipStreamSynchronize(stream));
  const int W = st.window, h0 = b->last_off[solver], m = std::min(W, capacity);
  *n_window = W; *n_run = st.run;
  if (m == 0) return LLD_OK;
  std::vector<HypRec> hr(m);
  std::vector<double> rt(12 * (size_t)m);
  std::vector<PnpJob> jobs(b->last_off[solver + 1] - h0 + 1);
  LLD_HIP_TRY(hipMemcpyAsync(hr.data(), b->dev.hyp + h0, sizeof(HypRec) * m, hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipMemcpyAsync(rt.data(), b->dev.rt + 12 * (size_t)h0, sizeof(double) * 12 * m, hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipMemcpyAsync(jobs.data(), b->dev.job + h0 + solver, sizeof(PnpJob) * jobs.size(), hipMemcpyDeviceToHost, stream));
  LLD_HIP_TRY(hipStreamSynchronize(stream));
  for (int k = 0; k < m; ++k) {
    lld_pnp_hypothesis& o = out[k];
    o.n_inliers = hr[k].n_inliers;
    o.record = hr[k].record;
    o.refine = -1; o.refined_inliers = 0;
    if (hr[k].job >= 0) {
      const PnpJob& j = jobs[hr[k].job - (h0 + solver)];
      o.refine = j.ok; o.refined_inliers = j.n_inliers;
    }
    for (int q = 0; q < 9; ++q) o.R[q] = rt[12 * (size_t)k + q];
    for (int q = 0; q < 3; ++q) o.t[q] = rt[12 * (size_t)k + 9 + q];
  }
  return LLD_OK;
}

extern "C" int lld_pnp_find(lld_ctx* ctx, const lld_pnp_problem* problem, const lld_pnp_params* params, lld_pnp_result* out) {
  if (!ctx || !problem || !params || !out) return LLD_ERR_INVALID;
  lld_pnp_batch* b = nullptr;
  if (int st = lld_pnp_batch_create(ctx, 1, problem, params, &b)) return st;
  int st = lld_pnp_batch_find(b, nullptr);   // find() = iterate(mRansacMaxIts)
  if (st == LLD_OK) st = lld_pnp_batch_download(b, out);
  lld_pnp_batch_destroy(b);
  return st;
}
