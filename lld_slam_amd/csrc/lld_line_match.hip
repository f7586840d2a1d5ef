// lld_line_match.hip — the line matchers (gfx950): kernels, one launcher per matcher on device arrays, and the host-array entry points.
//
//   line_candidates / line_resolve   TwoFrameLineMatcher::MatchLines (src/TwoFrameLineMatcher.cc:26-77) with CheckLinePair's gates (:79-109) or
//                                    a caller's gate matrix: lld_line_match_greedy, lld_line_match_stereo, line_stereo_launch_dev
//   line_track_gate + the two above  Tracking::AddLinesFrom (src/Tracking.cc:996-1124): lld_line_track_match, line_track_launch_dev
//   line_lastkf                      Tracking::MatchLinesLastKF (src/Tracking.cc:1449-1611): lld_line_match_last_frame, line_lastkf_launch_dev
// Every matcher is launched from ONE function that sees device pointers only; a host entry point validates, stages its arrays through an
// UploadBlock (one H2D copy), calls that launcher and copies the results back (one D2H copy, one wait).  The resident frame chain
// (lld_frame_track.hip, lld_frame_lines.hip) calls the same launchers through lld_track_internal.h.
#include <cmath>

#include "lld_common.h"
#include "lld_track_internal.h"
#include "lld_upload_block.h"

namespace {

// ------------------------------------------------------------------ TwoFrameLineMatcher::MatchLines (src/TwoFrameLineMatcher.cc:26-77)
// The reference walks the left lines in order; each takes the untaken, gated right line with the smallest distance below tau
// (strict '<' while scanning in index order = lexicographic (distance, index) minimum).  Only `taken` is order dependent, so:
//   line_candidates_kernel  one wavefront per LEFT line: gates + float-L2 distances of its row, then the row's kLineTopK smallest
//                           (distance, index) candidates by repeated wavefront argmin - all left lines in parallel;
//   line_resolve_kernel     the order-dependent assignment by fixed-point rounds over all left lines at once (see there).
constexpr int kLineTopK = 8;
struct LineCand { double d[kLineTopK]; int idx[kLineTopK]; int n, pad; };
constexpr double kInfD = 1.7976931348623157e308;

// Geometric gates of TwoFrameLineMatcher::CheckLinePair (src/TwoFrameLineMatcher.cc:79-109) for the stereo pair of one frame.
// T = identity, T_right = [I | (b,0,0)] (GetTForRight, src/LineMatching.cc:228-237).
// The 3x3 system of vgl::TriangulateLine (src/vgl.cc:78-108) has rows n1, n2, d = n1 x n2 / |n1 x n2|, so its determinant is
// |n1 x n2| > 0 once the 0.975 parallelism test passed (rank 3 always) and X0 = (b1 (d x n1)) / det in closed form.  The 3x2
// least squares of vgl::ReprojectLinePointTo3D (src/vgl.cc:336-346) is solved the way the reference solves it, by a column-pivoted
// Householder QR (reproject_param_qr): its normal equations square the condition number, and when the viewing ray of an end point is
// parallel to the triangulated line to ~1e-8 (two unrelated segments: one pair in ~1e8) they return a line parameter of the wrong
// sign, and the depth test `p.z < 0` with it (found by tools/fuzz_matchers.py, FUZZ_BIG=1, seed 9, scene 13712).
struct LineGateParams { double K[9]; double b; double min_len; int is_stereo; };

// Eigen::ColPivHouseholderQR::solve of the 3x2 system [a | c] (depth, param)^T = r, restated as oracle/lldo_linematch.cpp restates it
// (pivot on the larger column norm, makeHouseholderInPlace, rank by |R_kk| > 2 eps max|R_kk|, dropped unknowns = 0); returns the
// line parameter.  No contraction: the same operations as the host code, one rounding each.
__device__ __forceinline__ double reproject_param_qr(const double a[3], const double c[3], const double r[3]) {
#pragma clang fp contract(off)
  double A[3][2] = {{a[0], c[0]}, {a[1], c[1]}, {a[2], c[2]}};
  double b[3] = {r[0], r[1], r[2]};
  int perm[2] = {0, 1};
  double diag[2] = {0.0, 0.0}, maxpivot = 0.0;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    int best = k; double best_norm = -1.0;
    for (int cc = k; cc < 2; cc++) {
      double sn = 0.0; for (int rr = k; rr < 3; rr++) sn += A[rr][cc] * A[rr][cc];
      if (sn > best_norm) { best_norm = sn; best = cc; }
    }
    if (best != k) { for (int rr = 0; rr < 3; rr++) { const double t = A[rr][k]; A[rr][k] = A[rr][best]; A[rr][best] = t; } const int t = perm[k]; perm[k] = perm[best]; perm[best] = t; }
    const double c0 = A[k][k];
    double tail = 0.0; for (int rr = k + 1; rr < 3; rr++) tail += A[rr][k] * A[rr][k];
    double beta = c0, tau = 0.0; double v[3] = {0.0, 0.0, 0.0};
    if (tail > 2.2250738585072014e-308) {
      beta = sqrt(c0 * c0 + tail);
      if (c0 >= 0) beta = -beta;
      for (int rr = k + 1; rr < 3; rr++) v[rr] = A[rr][k] / (c0 - beta);
      tau = (beta - c0) / beta;
      for (int cc = k + 1; cc < 2; cc++) {
        double w = A[k][cc]; for (int rr = k + 1; rr < 3; rr++) w += v[rr] * A[rr][cc];
        A[k][cc] -= tau * w; for (int rr = k + 1; rr < 3; rr++) A[rr][cc] -= tau * w * v[rr];
      }
      double w = b[k]; for (int rr = k + 1; rr < 3; rr++) w += v[rr] * b[rr];
      b[k] -= tau * w; for (int rr = k + 1; rr < 3; rr++) b[rr] -= tau * w * v[rr];
    }
    A[k][k] = beta; for (int rr = k + 1; rr < 3; rr++) A[rr][k] = 0.0;
    diag[k] = fabs(beta);
    if (diag[k] > maxpivot) maxpivot = diag[k];
  }
  const double threshold = 2.220446049250313e-16 * 2.0;                         // NumTraits::epsilon() * diagonalSize()
  int rank = 0;
  for (int k = 0; k < 2; k++) if (diag[k] > threshold * maxpivot) rank++;
  double y[2] = {0.0, 0.0};
  for (int k = rank - 1; k >= 0; k--) {
    double sacc = b[k]; for (int cc = k + 1; cc < rank; cc++) sacc -= A[k][cc] * y[cc];
    y[k] = sacc / A[k][k];
  }
  double x[2] = {0.0, 0.0};
  for (int k = 0; k < 2; k++) x[perm[k]] = (k < rank) ? y[k] : 0.0;
  return x[1];
}

__device__ __forceinline__ void normalized_line_eq(const float* kl, const double* K, double* l) {
  const double sx = kl[0], sy = kl[1], ex = kl[2], ey = kl[3];
  const double ix = sy - ey, iy = ex - sx, iz = sx * ey - sy * ex;             // (sx,sy,1) x (ex,ey,1)
  const double a = K[0] * ix + K[3] * iy + K[6] * iz, b = K[1] * ix + K[4] * iy + K[7] * iz, c = K[2] * ix + K[5] * iy + K[8] * iz;
  const double n = sqrt(a * a + b * b);
  l[0] = a / n; l[1] = b / n; l[2] = c / n;
}

__device__ __forceinline__ bool line_pair_gate(const LineGateParams& P, const float* k1, int o1, const float* k2, int o2) {
  if (P.is_stereo && o1 != o2) return false;
  const double d1x = (double)k1[0] - (double)k1[2], d1y = (double)k1[1] - (double)k1[3];
  const double d2x = (double)k2[0] - (double)k2[2], d2y = (double)k2[1] - (double)k2[3];
  if (sqrt(d1x * d1x + d1y * d1y) < P.min_len || sqrt(d2x * d2x + d2y * d2y) < P.min_len) return false;
  double n1[3], n2[3];
  normalized_line_eq(k1, P.K, n1); normalized_line_eq(k2, P.K, n2);
  const double nn1 = sqrt(n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2]), nn2 = sqrt(n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2]);
  if (fabs(n1[0] * n2[0] + n1[1] * n2[1] + n1[2] * n2[2]) / nn1 / nn2 > 0.975) return false;
  double d[3] = {n1[1] * n2[2] - n1[2] * n2[1], n1[2] * n2[0] - n1[0] * n2[2], n1[0] * n2[1] - n1[1] * n2[0]};
  const double det = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  d[0] /= det; d[1] /= det; d[2] /= det;
  const double b1 = n2[0] * P.b;                                               // n2 . t2, t2 = (b,0,0); n1 . t1 = 0
  const double X0[3] = {b1 * (d[1] * n1[2] - d[2] * n1[1]) / det, b1 * (d[2] * n1[0] - d[0] * n1[2]) / det, b1 * (d[0] * n1[1] - d[1] * n1[0]) / det};
  if (sqrt(X0[0] * X0[0] + X0[1] * X0[1] + X0[2] * X0[2]) < 0.5) return false;
  const double c[3] = {-(P.K[0] * d[0] + P.K[1] * d[1] + P.K[2] * d[2]), -(P.K[3] * d[0] + P.K[4] * d[1] + P.K[5] * d[2]),
                       -(P.K[6] * d[0] + P.K[7] * d[1] + P.K[8] * d[2])};
  const double r[3] = {P.K[0] * X0[0] + P.K[1] * X0[1] + P.K[2] * X0[2], P.K[3] * X0[0] + P.K[4] * X0[1] + P.K[5] * X0[2],
                       P.K[6] * X0[0] + P.K[7] * X0[1] + P.K[8] * X0[2]};
  bool front = true;
  for (int e = 0; e < 2; e++) {
    const double a[3] = {(double)k1[2 * e], (double)k1[2 * e + 1], 1.0};
    const double p = reproject_param_qr(a, c, r);                               // line parameter of the re-projected endpoint
    if (X0[2] + p * d[2] < 0) front = false;
  }
  return front;
}

// grid nq, block 64; dynamic LDS: nt doubles (the row's admissible distances) + dim floats (the left descriptor).
// kGeom: the gate is CheckLinePair's geometry (written to gate_mat); otherwise gate_in is the caller's matrix (or NULL = all pass).
template <bool kGeom>
__global__ __launch_bounds__(64) void line_candidates_kernel(LineGateParams P, const float* __restrict__ left, const int* __restrict__ loct,
                                                            const float* __restrict__ right, const int* __restrict__ roct,
                                                            const float* __restrict__ q, const float* __restrict__ t, int dim, int nt,
                                                            const uint8_t* __restrict__ gate_in, double tau, uint8_t* __restrict__ gate_mat,
                                                            double* __restrict__ dmat, LineCand* __restrict__ cand) {
  extern __shared__ __attribute__((aligned(16))) double lds_row[];
  double* drow = lds_row;
  float* qrow = reinterpret_cast<float*>(drow + nt);
  const int j = blockIdx.x, lane = threadIdx.x;
  for (int i = lane; i < dim; i += 64) qrow[i] = q[(size_t)j * dim + i];
  __syncthreads();
  float k1[4] = {0.f, 0.f, 0.f, 0.f}; int o1 = 0;
  if (kGeom) { for (int e = 0; e < 4; e++) k1[e] = left[4 * j + e]; o1 = loct[j]; }
  for (int oi = lane; oi < nt; oi += 64) {
    bool g;
    if (kGeom) { float k2[4]; for (int e = 0; e < 4; e++) k2[e] = right[4 * oi + e]; g = line_pair_gate(P, k1, o1, k2, roct[oi]); gate_mat[(size_t)j * nt + oi] = g ? 1 : 0; }
    else g = !gate_in || gate_in[(size_t)j * nt + oi] != 0;
    double dist = kInfD;
    if (g) {                                                           // LineMatcher::MatchLineDescriptors: float difference, double accumulation
      const float* tr = t + (size_t)oi * dim;
      double acc = 0.0;
      for (int i = 0; i < dim; i++) { const float df = qrow[i] - tr[i]; acc = fma((double)df, (double)df, acc); }
      dist = sqrt(acc);
    }
    dmat[(size_t)j * nt + oi] = dist;
    drow[oi] = (g && dist < tau) ? dist : kInfD;
  }
  __syncthreads();
  // the kLineTopK smallest (distance, index) pairs of the row, in order: every round takes the smallest pair greater than the last
  double pd = -1.0; int pi = -1, n = 0;
  double my_d = kInfD; int my_i = -1;
  for (int r = 0; r < kLineTopK; r++) {
    double bd = kInfD; int bi = 0x7fffffff;
    for (int oi = lane; oi < nt; oi += 64) {
      const double d = drow[oi];
      if (d < tau && (d > pd || (d == pd && oi > pi)) && d < bd) { bd = d; bi = oi; }    // ascending oi per lane: lowest index on ties
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(bd, off); const int oidx = __shfl_xor(bi, off);
      if (od < bd || (od == bd && oidx < bi)) { bd = od; bi = oidx; }
    }
    if (bi == 0x7fffffff) break;
    if (lane == r) { my_d = bd; my_i = bi; }
    pd = bd; pi = bi; n++;
  }
  if (lane < kLineTopK) { cand[j].d[lane] = my_d; cand[j].idx[lane] = my_i; }
  if (lane == 0) { cand[j].n = n; cand[j].pad = 0; }
}

// The greedy, order-dependent assignment ("left line j takes its best right line that no EARLIER left line took").  Two regimes:
//   * fixed-point rounds, as the guided ORB search resolves its occupancy (lld_orb_search.hip): a round lets every line pick, in parallel, the
//     first entry of its short list that no line with a smaller index picked in the round before; blk[c] = the smallest index that picks c.
//     Line 0 is final after one round, line j after j + 1 at the latest, and a round that changes nothing has reached the sequential answer.
//     AddLinesFrom's sparse candidate sets converge in 3 - 6 rounds of a few hundred cycles (the one-wavefront walk of rounds 2 - 5 paid
//     ~400 cycles per LINE: 45 us for 260 map lines, now 5);
//   * where the rounds do NOT converge quickly - the stereo matcher with its wide tau: unrelated lines take over partners of later lines and
//     the corrections ripple down one line per round (300 x 300: ~300 rounds, 340 us) - the kernel stops after kResolveRounds rounds and ONE
//     wavefront walks the rest in order: every line below the smallest index that changed in the last round is final (its inputs, the picks of
//     the lines before it, did not change, nor did its own), so the walk starts there with their picks as the taken set.
// A list that is full and completely taken falls back to a scan of the stored row like the reference does.  One workgroup; LDS: blk[nt] + pick[nq].
constexpr int kResolveThreads = 256;
constexpr int kResolveRounds = 8;
inline size_t line_resolve_lds(int nq, int nt) { return ((size_t)nq + (size_t)nt) * 4 + 16; }
static int line_resolve_prepare(int nq, int nt);      // raises the kernel's dynamic-LDS ceiling when blk + pick need more than the default (defined after the kernel)
__global__ __launch_bounds__(kResolveThreads) void line_resolve_kernel(const LineCand* __restrict__ cand, const double* __restrict__ dmat, const uint8_t* __restrict__ gate,
                                                                      int nq, int nt, double tau, int* __restrict__ matches, double* __restrict__ match_dist,
                                                                      lld_track::LineApplyDev ap, const double* __restrict__ map_x0, const double* __restrict__ map_dir) {
  extern __shared__ __attribute__((aligned(16))) int res_lds[];
  __shared__ int changed_min, scan_min;
  __shared__ int clist[kResolveThreads][kLineTopK + 1];  // the ordered walk's candidate lists, a chunk of lines at a time
  int* blk = res_lds; int* pick = res_lds + nt;
  const int tid = threadIdx.x;
  constexpr int kFree = 0x7fffffff;
  for (int i = tid; i < nt; i += kResolveThreads) blk[i] = kFree;
  for (int j = tid; j < nq; j += kResolveThreads) pick[j] = -1;
  if (tid == 0) { changed_min = kFree; scan_min = kFree; }
  __syncthreads();
  int walk_from = kFree;                                  // < kFree: lines from this index on are walked in order
  for (int round = 0;; round++) {
    for (int j = tid; j < nq; j += kResolveThreads) {
      const LineCand& C = cand[j];
      const int n = C.n;
      int bi = -1;
      for (int k = 0; k < n; k++) { const int c = C.idx[k]; if (blk[c] >= j) { bi = c; break; } }
      // every listed candidate taken and the list was cut: this line needs a scan of its stored row, which only the ordered walk does
      // (with the wavefront's 64 lanes and the FINAL taken set); the line and everything after it is left to the walk
      if (bi < 0 && n == kLineTopK) atomicMin(&scan_min, j);
      if (bi != pick[j]) { pick[j] = bi; atomicMin(&changed_min, j); }
    }
    __syncthreads();
    const int first_changed = changed_min, first_scan = scan_min;
    if (first_changed == kFree || first_changed >= first_scan) { walk_from = first_scan; break; }     // converged (below the first line that needs a row scan)
    if (round + 1 >= kResolveRounds) walk_from = min(first_changed, first_scan);
    __syncthreads();
    for (int i = tid; i < nt; i += kResolveThreads) blk[i] = kFree;
    if (tid == 0) { changed_min = kFree; scan_min = kFree; }
    __syncthreads();
    for (int j = tid; j < nq; j += kResolveThreads) { const int c = pick[j]; if (c >= 0) atomicMin(&blk[c], j); }
    __syncthreads();
    if (walk_from != kFree) break;
  }
  if (walk_from != kFree) {
    // the taken set of the walk: the (final) picks of the lines below walk_from
    __syncthreads();
    for (int i = tid; i < nt; i += kResolveThreads) blk[i] = kFree;
    __syncthreads();
    for (int j = tid; j < min(walk_from, nq); j += kResolveThreads) { const int c = pick[j]; if (c >= 0) blk[c] = j; }
    for (int j0 = walk_from; j0 < nq; j0 += kResolveThreads) {
      const int nj = min(kResolveThreads, nq - j0);
      __syncthreads();
      if (tid < nj) {
        const LineCand& C = cand[j0 + tid];
#pragma unroll
        for (int k = 0; k < kLineTopK; k++) clist[tid][k] = C.idx[k];
        clist[tid][kLineTopK] = C.n;
      }
      __syncthreads();
      if (tid < 64) {
        const int lane = tid;
        for (int jj = 0; jj < nj; jj++) {
          const int j = j0 + jj;
          const int n = clist[jj][kLineTopK];
          const int my_i = lane < n ? clist[jj][lane] : 0;
          const bool free_ = lane < n && blk[my_i] == kFree;
          const unsigned long long mask = __ballot(free_);
          int bi = -1;
          if (mask) bi = __builtin_amdgcn_readlane(my_i, __ffsll((long long)mask) - 1);
          else if (n == kLineTopK) {
            double sd = kInfD; int si = kFree;
            for (int oi = lane; oi < nt; oi += 64) {
              if (blk[oi] != kFree) continue;
              if (gate && !gate[(size_t)j * nt + oi]) continue;
              const double d = dmat[(size_t)j * nt + oi];
              if (d < tau && d < sd) { sd = d; si = oi; }
            }
            for (int off = 32; off > 0; off >>= 1) {
              const double od = __shfl_xor(sd, off); const int oidx = __shfl_xor(si, off);
              if (od < sd || (od == sd && oidx < si)) { sd = od; si = oidx; }
            }
            if (si != kFree) bi = si;
          }
          if (lane == 0) { pick[j] = bi; if (bi >= 0) blk[bi] = j; }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // (one wavefront: its LDS operations retire in order; this keeps the compiler from moving the next reads up)
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  }
  __syncthreads();
  for (int j = tid; j < nq; j += kResolveThreads) {
    const int bi = pick[j];
    matches[j] = bi;
    if (match_dist) match_dist[j] = bi >= 0 ? dmat[(size_t)j * nt + bi] : kInfD;
    // the device-resident chain (lld_frame_track_*): the frame line takes the map line here (every frame line has at most one taker)
    if (ap.ln_has && bi >= 0) {
      ap.ln_has[bi] = 1; ap.ln_id[bi] = ap.map_id[j];
      for (int c = 0; c < 3; c++) { ap.ln_x0[3 * bi + c] = map_x0[3 * j + c]; ap.ln_dir[3 * bi + c] = map_dir[3 * j + c]; }
      const int at = atomicAdd(ap.n_tracked, 1);
      if (at < ap.tracked_cap) ap.tracked[at] = ap.map_id[j];
    }
  }
}

static int line_resolve_prepare(int nq, int nt) {
  const size_t lds = line_resolve_lds(nq, nt);
  if (lds > LLD_LINE_LDS_CEILING) return LLD_ERR_UNSUPPORTED;                // (about 38 000 lines on both sides together)
  if (lds > 48 * 1024) LLD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&line_resolve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return LLD_OK;
}

// ------------------------------------------------------------------ Tracking::AddLinesFrom (src/Tracking.cc:996-1124)
// Gate matrix of the map-line -> frame-line association: row = map line, column = line of the current frame.  Everything that depends
// on the map line only is computed once per row (projected image lines in the left / right camera for vgl::LineReprojErrorL1, the Hough
// cell neighbourhood of SubselectWithGrid, the depth test of the main points); a column contributes its cell, its occupancy, its stereo
// partner and four dot products.  The greedy, order-dependent part is line_resolve_kernel's, as for TwoFrameLineMatcher.
constexpr int kHoughDist = 50, kHoughAng = 50;           // FRAME_DIST_CELLS, FRAME_ANG_CELLS (include/Frame.h:45-46)
#define LLD_HOUGH_PI 3.14159265                          /* the literal of src/LineMatching.cc:61 */
struct HoughCell { int dist_ind, ang_ind, shift_dist, shift_ang; };
// centre cell + shifts of GetHoughCoordinates (src/LineMatching.cc:63-110) for the homogeneous image line leq (pixels)
__host__ __device__ inline HoughCell hough_cell(double lx, double ly, double lz, double sx, double sy) {
  lx /= sx; ly /= sy;
  const double n = sqrt(lx * lx + ly * ly);
  lx /= n; ly /= n; lz /= n;
  if (ly < 0) { lx = -lx; ly = -ly; lz = -lz; }
  HoughCell c;
  // a degenerate line (coincident end points): the reference would index its grid with the integer cast of a NaN; the build treats it as the line y = 0
  if (!(lx - lx == 0.0) || !(ly - ly == 0.0) || !(lz - lz == 0.0)) { lx = 0.0; ly = 1.0; lz = 0.0; }      // x - x == 0 only for a finite x
  const double dist_level = fabs(lz / (sqrt(2.0))) * kHoughDist;
  int di = (int)floor(dist_level + 0.5);
  di = di < kHoughDist - 1 ? di : kHoughDist - 1; di = di > 0 ? di : 0;
  c.dist_ind = di; c.shift_dist = (dist_level - di < 0) ? 1 : -1;
  const double ang = atan2(ly, lx);
  const double ang_level = ang / LLD_HOUGH_PI * kHoughAng;
  int ai = (int)floor(ang_level + 0.5);
  ai = ai < kHoughAng - 1 ? ai : kHoughAng - 1; ai = ai > 0 ? ai : 0;
  c.ang_ind = ai; c.shift_ang = (ang_level - ai < 0) ? 1 : -1;
  return c;
}
using LineTrackParams = lld_track::LineTrackDevParams;      // the camera of AddLinesFrom: by value, or read from device memory (P_dev)

// one thread per frame line: its grid cell (the fill the reference lacks: the centre cell of the line through the left KeyLine)
__global__ void line_cells_kernel(const float* __restrict__ lines, int n, double sx, double sy, int* __restrict__ cell) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double xs = lines[4 * i], ys = lines[4 * i + 1], xe = lines[4 * i + 2], ye = lines[4 * i + 3];
  const HoughCell c = hough_cell(ys - ye, xe - xs, xs * ye - ys * xe, sx, sy);          // GetLineEq: (xs,ys,1) x (xe,ye,1)
  cell[i] = c.dist_ind * kHoughAng + c.ang_ind;
}

__device__ __forceinline__ void track_map_point(const LineTrackParams& P, const double* t, const double* X, double* o) {   // vgl::MapPoint: R^T (X - t)
  const double d0 = X[0] - t[0], d1 = X[1] - t[1], d2 = X[2] - t[2];
  for (int c = 0; c < 3; c++) o[c] = P.R[0 * 3 + c] * d0 + P.R[1 * 3 + c] * d1 + P.R[2 * 3 + c] * d2;
}
__device__ __forceinline__ void track_k_mul(const double* K, const double* X, double* o) {
  for (int r = 0; r < 3; r++) o[r] = K[3 * r] * X[0] + K[3 * r + 1] * X[1] + K[3 * r + 2] * X[2];
}
// image line of the 3D line (X0, dir) in the camera with centre t: K MapPoint(X0) x K MapPoint(X0 + dir), first two components normalised
__device__ __forceinline__ void track_image_line(const LineTrackParams& P, const double* t, const double* X0, const double* dir, double* l) {
  double a[3], b[3], Xa[3], Xb[3];
  const double X0d[3] = {X0[0] + dir[0], X0[1] + dir[1], X0[2] + dir[2]};
  track_map_point(P, t, X0, a); track_map_point(P, t, X0d, b);
  track_k_mul(P.K, a, Xa); track_k_mul(P.K, b, Xb);
  {
    // no fused multiply-add here: a map line with a zero direction has Xa == Xb and the reference's cross product is exactly zero (the line
    // becomes NaN and, `NaN > thr` being false, passes the reprojection gate); a contracted a*b - c*d would leave a rounding residue instead
#pragma clang fp contract(off)
    l[0] = Xa[1] * Xb[2] - Xa[2] * Xb[1]; l[1] = Xa[2] * Xb[0] - Xa[0] * Xb[2]; l[2] = Xa[0] * Xb[1] - Xa[1] * Xb[0];
  }
  const double n = sqrt(l[0] * l[0] + l[1] * l[1]);
  l[0] /= n; l[1] /= n; l[2] /= n;
}

// grid n_map, block 64
__global__ __launch_bounds__(64) void line_track_gate_kernel(LineTrackParams P, const double* __restrict__ x0, const double* __restrict__ dir,
                                                            const double* __restrict__ x1, const double* __restrict__ x2, const uint8_t* __restrict__ skip,
                                                            int n_cur, const float* __restrict__ left, const int* __restrict__ loct,
                                                            const float* __restrict__ right, const int* __restrict__ lmatch,
                                                            const uint8_t* __restrict__ occupied, const int* __restrict__ cell, uint8_t* __restrict__ gate,
                                                            const LineTrackParams* __restrict__ P_dev) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (P_dev) P = *P_dev;                                                      // the pose came out of a kernel (lld_frame_track_*): camera in device memory
  uint8_t* grow = gate + (size_t)i * n_cur;
  bool row_ok = !(skip && skip[i]);
  double X1c[3], X2c[3];
  track_map_point(P, P.t, x1 + 3 * i, X1c); track_map_point(P, P.t, x2 + 3 * i, X2c);
  if (X1c[2] < 0 || X2c[2] < 0) row_ok = false;                               // Tracking.cc:1066-1074
  double ll[3], lr[3];
  track_image_line(P, P.t, x0 + 3 * i, dir + 3 * i, ll);
  track_image_line(P, P.tr, x0 + 3 * i, dir + 3 * i, lr);
  // SubselectWithGrid: the cell neighbourhood of the projected line (GetHoughCoordinates with step 3: six consecutive angle cells
  // around the centre, modulo the grid, and up to six distance cells, the last distance row excluded as in the reference)
  const HoughCell hc = hough_cell(ll[0], ll[1], ll[2], P.sx, P.sy);
  const int ang_min = hc.ang_ind < hc.ang_ind + hc.shift_ang ? hc.ang_ind : hc.ang_ind + hc.shift_ang;
  const int dist_min = hc.dist_ind < hc.dist_ind + hc.shift_dist ? hc.dist_ind : hc.dist_ind + hc.shift_dist;
  for (int si = lane; si < n_cur; si += 64) {
    bool g = row_ok && !(occupied && occupied[si]);
    const int ri = lmatch[si];
    if (ri < 0 && !P.monocular) g = false;
    if (g && P.use_grid) {
      const int cd = cell[si] / kHoughAng, ca = cell[si] - cd * kHoughAng;
      int da = ca - (ang_min - 2); da %= kHoughAng; if (da < 0) da += kHoughAng;
      const bool in_ang = da < 6;
      const bool in_dist = cd >= dist_min - 2 && cd <= dist_min + 3 && cd >= 0 && cd < kHoughDist - 1;
      g = in_ang && in_dist;
    }
    if (g) {
      double thr = P.thr_base;                                                // GetReprojThrPyramid
      for (int o = 0; o < loct[si]; o++) thr *= 1.44;
      const float* kl = left + 4 * si;
      const double se = fabs((double)kl[0] * ll[0] + (double)kl[1] * ll[1] + ll[2]) + fabs((double)kl[2] * ll[0] + (double)kl[3] * ll[1] + ll[2]);
      double se2 = 0.0;
      if (!P.monocular) {
        const float* kr = right + 4 * ri;
        se2 = fabs((double)kr[0] * lr[0] + (double)kr[1] * lr[1] + lr[2]) + fabs((double)kr[2] * lr[0] + (double)kr[3] * lr[1] + lr[2]);
      }
      if (se > thr || se2 > thr) g = false;                                   // Tracking.cc:1085
    }
    grow[si] = g ? 1 : 0;
  }
}

// ------------------------------------------------------------------ Tracking::MatchLinesLastKF (src/Tracking.cc:1449-1611)
struct LastKfParams { double K[9]; double R[9], t[3], tr[3]; double Rl[9], tl[3], tlr[3]; double thr_base, md_thr, sx, sy; int use_grid; };
__device__ __forceinline__ void d3_cross(const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
__device__ __forceinline__ double d3_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void d3_rmul(const double* R, const double* v, double* o) { for (int r = 0; r < 3; r++) o[r] = R[3 * r] * v[0] + R[3 * r + 1] * v[1] + R[3 * r + 2] * v[2]; }
__device__ __forceinline__ void d3_rtmul(const double* R, const double* v, double* o) { for (int c = 0; c < 3; c++) o[c] = R[c] * v[0] + R[3 + c] * v[1] + R[6 + c] * v[2]; }
// vgl::TriangulateLine (src/vgl.cc:78-108) for two cameras with one rotation R (camera-to-world) and centres t1, t2.  The 3x3 system with
// rows n1, n2, d = n1 x n2 / |n1 x n2| has determinant |n1 x n2| > 0 once the parallelism test passed, so Eigen's rank() < 3 cannot fire
// and the solution is Cramer's rule with b = (n1.t1, n2.t2, 0).
__device__ __forceinline__ bool tri_line(const double* R, const double* t1, const double* t2, const double* l1, const double* l2, double* X0, double* dir) {
  double n1[3], n2[3];
  d3_rmul(R, l1, n1); d3_rmul(R, l2, n2);
  if (fabs(d3_dot(n1, n2)) / sqrt(d3_dot(n1, n1)) / sqrt(d3_dot(n2, n2)) > 0.975) return false;
  d3_cross(n1, n2, dir);
  const double dn = sqrt(d3_dot(dir, dir));
  dir[0] /= dn; dir[1] /= dn; dir[2] /= dn;
  double c23[3], c31[3];
  d3_cross(n2, dir, c23); d3_cross(dir, n1, c31);
  const double det = d3_dot(n1, c23), b1 = d3_dot(n1, t1), b2 = d3_dot(n2, t2);
  for (int k = 0; k < 3; k++) X0[k] = (b1 * c23[k] + b2 * c31[k]) / det;
  return true;
}
// symmetric 3x3 eigen-decomposition (cyclic Jacobi): A -> eigenvalues w[3], eigenvectors as the columns of V
__device__ __forceinline__ void sym3_eig(double A[3][3], double V[3][3], double* w) {
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 12; sweep++) {
    for (int p = 0; p < 2; p++) for (int q = p + 1; q < 3; q++) {
      if (A[p][q] == 0.0) continue;
      const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
      const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
      const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
      for (int k = 0; k < 3; k++) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - sn * akq; A[k][q] = sn * akp + c * akq; }
      for (int k = 0; k < 3; k++) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - sn * aqk; A[q][k] = sn * apk + c * aqk; }
      for (int k = 0; k < 3; k++) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = c * vkp - sn * vkq; V[k][q] = sn * vkp + c * vkq; }
    }
  }
  for (int i = 0; i < 3; i++) w[i] = A[i][i];
}
// vgl::MultiTriangulateLine (src/vgl.cc:28-76) for four views.  The direction is the eigenvector of the smallest eigenvalue of M^T M (the
// right singular vector of the smallest singular value of the normal matrix M), its largest component positive.  The reference solves
// M X0 = b by a pivoted QR and then removes X0's component along that direction: with M^T M = sum lambda_k v_k v_k^T this is
// X0 = sum over the two LARGER eigenpairs of v_k (v_k . M^T b) / lambda_k - the ill-conditioned third term never formed.
__device__ __forceinline__ bool multi_tri_line(const double* const* Rs, const double* const* ts, const double (*leqs)[3], double* X0, double* dir) {
  double nrm[4][3];
  for (int i = 0; i < 4; i++) {
    const double ln = sqrt(d3_dot(leqs[i], leqs[i]));
    const double u[3] = {leqs[i][0] / ln, leqs[i][1] / ln, leqs[i][2] / ln};
    d3_rmul(Rs[i], u, nrm[i]);
  }
  for (int i = 1; i < 4; i++) if (fabs(d3_dot(nrm[0], nrm[i])) / sqrt(d3_dot(nrm[0], nrm[0])) / sqrt(d3_dot(nrm[i], nrm[i])) > 0.975) return false;
  double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, Mtb[3] = {0, 0, 0};
  for (int i = 0; i < 4; i++) {
    const double bi = d3_dot(nrm[i], ts[i]);
    for (int r = 0; r < 3; r++) { Mtb[r] += nrm[i][r] * bi; for (int c = 0; c < 3; c++) A[r][c] += nrm[i][r] * nrm[i][c]; }
  }
  double V[3][3], w[3];
  sym3_eig(A, V, w);
  int m = 0; for (int i = 1; i < 3; i++) if (w[i] < w[m]) m = i;
  double d[3] = {V[0][m], V[1][m], V[2][m]};
  const double dn = sqrt(d3_dot(d, d));
  int big = 0; if (fabs(d[1]) > fabs(d[big])) big = 1; if (fabs(d[2]) > fabs(d[big])) big = 2;
  const double sg = d[big] < 0 ? -1.0 / dn : 1.0 / dn;
  for (int k = 0; k < 3; k++) { dir[k] = d[k] * sg; X0[k] = 0.0; }
  for (int e = 0; e < 3; e++) {
    if (e == m) continue;
    const double v[3] = {V[0][e], V[1][e], V[2][e]};
    const double cf = d3_dot(v, Mtb) / w[e];
    for (int k = 0; k < 3; k++) X0[k] += cf * v[k];
  }
  return true;
}
// the line parameter of vgl::ReprojectLinePointTo3D (src/vgl.cc:336-346) through the normal equations of its 3x2 least squares
__device__ __forceinline__ double reproject_param(const double* K, const double* X0rot, const double* dirRot, double px, double py) {
  double c[3], r[3];
  for (int q = 0; q < 3; q++) { c[q] = -(K[3 * q] * dirRot[0] + K[3 * q + 1] * dirRot[1] + K[3 * q + 2] * dirRot[2]); r[q] = K[3 * q] * X0rot[0] + K[3 * q + 1] * X0rot[1] + K[3 * q + 2] * X0rot[2]; }
  const double aa = px * px + py * py + 1.0, ac = px * c[0] + py * c[1] + c[2], ar = px * r[0] + py * r[1] + r[2];
  const double cc = d3_dot(c, c), cr = d3_dot(c, r);
  return (aa * cr - ac * ar) / (aa * cc - ac * ac);
}
__device__ __forceinline__ void image_line_of(const double* K, const double* R, const double* t, const double* X0, const double* dir, double* l) {
  double a[3], b[3], Xa[3], Xb[3];
  const double d0[3] = {X0[0] - t[0], X0[1] - t[1], X0[2] - t[2]}, d1[3] = {X0[0] + dir[0] - t[0], X0[1] + dir[1] - t[1], X0[2] + dir[2] - t[2]};
  d3_rtmul(R, d0, a); d3_rtmul(R, d1, b);
  for (int r = 0; r < 3; r++) { Xa[r] = K[3 * r] * a[0] + K[3 * r + 1] * a[1] + K[3 * r + 2] * a[2]; Xb[r] = K[3 * r] * b[0] + K[3 * r + 1] * b[1] + K[3 * r + 2] * b[2]; }
  d3_cross(Xa, Xb, l);
  const double n = sqrt(l[0] * l[0] + l[1] * l[1]);
  l[0] /= n; l[1] /= n; l[2] /= n;
}

// grid n_cur, block 64; dynamic LDS: dim floats (the current line's descriptor)
// kDev: both frames are resident (lld_frame_new_map_lines): the two cameras are the LineTrackParams their chains left in device memory
// (cur_cam also brings K, sx, sy); P then carries thr_base, md_thr and use_grid only.
template <bool kDev>
__global__ __launch_bounds__(64) void line_lastkf_kernel(LastKfParams P, int n_cur, const float* __restrict__ cur_left, const float* __restrict__ cur_right,
                                                        const int* __restrict__ cur_lm, const uint8_t* __restrict__ cur_occ, const float* __restrict__ cur_desc,
                                                        int n_last, const float* __restrict__ last_left, const int* __restrict__ last_oct,
                                                        const float* __restrict__ last_right, const int* __restrict__ last_lm,
                                                        const uint8_t* __restrict__ last_skip, const float* __restrict__ last_desc, const int* __restrict__ last_cell,
                                                        int dim, int* __restrict__ match_last, uint8_t* __restrict__ created, double* __restrict__ x0_out,
                                                        double* __restrict__ dir_out, const LineTrackParams* __restrict__ cur_cam,
                                                        const LineTrackParams* __restrict__ last_cam) {
  extern __shared__ __attribute__((aligned(16))) float qrow[];
  const int i = blockIdx.x, lane = threadIdx.x;
  if (kDev) {
    for (int k = 0; k < 9; k++) { P.K[k] = cur_cam->K[k]; P.R[k] = cur_cam->R[k]; P.Rl[k] = last_cam->R[k]; }
    for (int k = 0; k < 3; k++) { P.t[k] = cur_cam->t[k]; P.tr[k] = cur_cam->tr[k]; P.tl[k] = last_cam->t[k]; P.tlr[k] = last_cam->tr[k]; }
    P.sx = cur_cam->sx; P.sy = cur_cam->sy;
  }
  if (lane == 0) { match_last[i] = -1; created[i] = 0; for (int k = 0; k < 3; k++) { x0_out[3 * i + k] = 0.0; dir_out[3 * i + k] = 0.0; } }
  if (cur_occ && cur_occ[i]) return;
  const int ri = cur_lm[i];
  if (ri < 0) return;
  for (int k = lane; k < dim; k += 64) qrow[k] = cur_desc[(size_t)i * dim + k];
  __syncthreads();
  double l1[3], l2[3], X0[3], ld[3];
  normalized_line_eq(cur_left + 4 * i, P.K, l1); normalized_line_eq(cur_right + 4 * ri, P.K, l2);
  if (!tri_line(P.R, P.t, P.tr, l1, l2, X0, ld)) return;
  double ll[3], lr[3];
  image_line_of(P.K, P.Rl, P.tl, X0, ld, ll);
  image_line_of(P.K, P.Rl, P.tlr, X0, ld, lr);
  const HoughCell hc = hough_cell(ll[0], ll[1], ll[2], P.sx, P.sy);
  const int ang_min = hc.ang_ind < hc.ang_ind + hc.shift_ang ? hc.ang_ind : hc.ang_ind + hc.shift_ang;
  const int dist_min = hc.dist_ind < hc.dist_ind + hc.shift_dist ? hc.dist_ind : hc.dist_ind + hc.shift_dist;
  double bd = kInfD; int bi = 0x7fffffff;
  for (int li = lane; li < n_last; li += 64) {
    const int pri = last_lm[li];
    if (pri < 0) continue;
    if (last_skip && last_skip[li]) continue;
    if (P.use_grid) {
      const int cd = last_cell[li] / kHoughAng, ca = last_cell[li] - cd * kHoughAng;
      int da = ca - (ang_min - 2); da %= kHoughAng; if (da < 0) da += kHoughAng;
      if (!(da < 6 && cd >= dist_min - 2 && cd <= dist_min + 3 && cd >= 0 && cd < kHoughDist - 1)) continue;
    }
    double thr = P.thr_base;
    for (int o = 0; o < last_oct[li]; o++) thr *= 1.44;
    const float* kl = last_left + 4 * li; const float* kr = last_right + 4 * pri;
    const double se = fabs((double)kl[0] * ll[0] + (double)kl[1] * ll[1] + ll[2]) + fabs((double)kl[2] * ll[0] + (double)kl[3] * ll[1] + ll[2]);
    const double se2 = fabs((double)kr[0] * lr[0] + (double)kr[1] * lr[1] + lr[2]) + fabs((double)kr[2] * lr[0] + (double)kr[3] * lr[1] + lr[2]);
    if (se > thr && se2 > thr) continue;                                    // Tracking.cc:1526
    const float* tr = last_desc + (size_t)li * dim;
    double acc = 0.0;
    for (int k = 0; k < dim; k++) { const float df = tr[k] - qrow[k]; acc = fma((double)df, (double)df, acc); }
    const double dist = sqrt(acc);
    if (dist < bd) { bd = dist; bi = li; }                                  // ascending li per lane: the lowest index wins ties
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(bd, off); const int oidx = __shfl_xor(bi, off);
    if (od < bd || (od == bd && oidx < bi)) { bd = od; bi = oidx; }
  }
  if (lane != 0 || bi == 0x7fffffff || bd > P.md_thr) return;
  match_last[i] = bi;
  const int pri = last_lm[bi];
  double leqs[4][3];
  for (int k = 0; k < 3; k++) { leqs[0][k] = l1[k]; leqs[1][k] = l2[k]; }
  normalized_line_eq(last_left + 4 * bi, P.K, leqs[2]); normalized_line_eq(last_right + 4 * pri, P.K, leqs[3]);
  const double* Rs[4] = {P.R, P.R, P.Rl, P.Rl}; const double* ts[4] = {P.t, P.tr, P.tl, P.tlr};
  if (!multi_tri_line(Rs, ts, leqs, X0, ld)) return;
  // ReprojectKeyLineTo3D of the current left KeyLine in the current pose
  double X0rot[3], dirRot[3];
  { const double dd[3] = {X0[0] - P.t[0], X0[1] - P.t[1], X0[2] - P.t[2]}; d3_rtmul(P.R, dd, X0rot); d3_rtmul(P.R, ld, dirRot); }
  const float* kc = cur_left + 4 * i;
  const double p_s = reproject_param(P.K, X0rot, dirRot, kc[0], kc[1]), p_e = reproject_param(P.K, X0rot, dirRot, kc[2], kc[3]);
  const double p1[3] = {X0[0] + p_s * ld[0], X0[1] + p_s * ld[1], X0[2] + p_s * ld[2]}, p2[3] = {X0[0] + p_e * ld[0], X0[1] + p_e * ld[1], X0[2] + p_e * ld[2]};
  bool behind = false;
  for (int v = 0; v < 4; v++) {
    const double a1[3] = {p1[0] - ts[v][0], p1[1] - ts[v][1], p1[2] - ts[v][2]}, a2[3] = {p2[0] - ts[v][0], p2[1] - ts[v][1], p2[2] - ts[v][2]};
    const double z1 = Rs[v][2] * a1[0] + Rs[v][5] * a1[1] + Rs[v][8] * a1[2], z2 = Rs[v][2] * a2[0] + Rs[v][5] * a2[1] + Rs[v][8] * a2[2];
    if (z1 < 0 || z2 < 0) behind = true;
  }
  if (behind) return;
  created[i] = 1;
  for (int k = 0; k < 3; k++) { x0_out[3 * i + k] = X0[k]; dir_out[3 * i + k] = ld[k]; }
}

// ================================================================ launchers: device pointers in, kernels on the stream; nothing is copied, nothing waits.
// Their callers have asked line_limits_check and do not come here with an empty side.
using lld_track::LastKfDev; using lld_track::LineApplyDev; using lld_track::LineFrameDev; using lld_track::LineMapDev; using lld_track::LineStereoDev;
using lld_track::Span; using lld_track::UploadBlock; using lld_track::al;

// Gate matrix [rows][cols], distances [rows][cols] and candidate lists [rows] of one match.  A host entry point places the gate where its
// download wants it; the resident routes carve all three out of one buffer of line_work_bytes.
struct LineWork { uint8_t* gate; double* dmat; LineCand* cand; };
LineWork line_work_carve(void* d_work, int rows, int cols) {
  const size_t pairs = (size_t)rows * (size_t)cols;
  char* w = static_cast<char*>(d_work);
  return {reinterpret_cast<uint8_t*>(w), reinterpret_cast<double*>(w + al(pairs)), reinterpret_cast<LineCand*>(w + al(pairs) + al(pairs * 8))};
}

LineGateParams line_gate_params(const lld_line_stereo_params& prm) {
  LineGateParams P; std::memset(&P, 0, sizeof P);
  for (int i = 0; i < 9; i++) P.K[i] = prm.K[i];
  P.b = prm.b; P.min_len = (double)prm.min_line_length; P.is_stereo = prm.is_stereo;
  return P;
}

// The candidate lists of all rows (in.nl of them against in.nr columns), then the greedy resolve.  kGeom: the gate is CheckLinePair's geometry of
// in.left / in.right under P, written to W.gate; otherwise W.gate is the gate to read (null: every pair passes) and neither P nor the lines are looked at.
template <bool kGeom>
int line_match_launch(hipStream_t st, const LineGateParams& P, const LineStereoDev& in, double tau, const LineWork& W, int32_t* matches, double* match_dist,
                      const LineApplyDev& apply, const double* map_x0, const double* map_dir) {
  const int rows = in.nl, cols = in.nr;
  const size_t lds = (size_t)cols * 8 + (size_t)in.dim * 4 + 16;              // one row of distances + the row's descriptor
  if (lds > 48 * 1024) LLD_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&line_candidates_kernel<kGeom>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(line_candidates_kernel<kGeom>, dim3(rows), dim3(64), lds, st, P, in.left, in.loct, in.right, in.roct, in.dl, in.dr, in.dim, cols,
                     kGeom ? nullptr : W.gate, tau, kGeom ? W.gate : nullptr, W.dmat, W.cand);
  if (const int rs = line_resolve_prepare(rows, cols)) return rs;
  hipLaunchKernelGGL(line_resolve_kernel, dim3(1), dim3(kResolveThreads), line_resolve_lds(rows, cols), st, W.cand, W.dmat, W.gate, rows, cols, tau, matches, match_dist,
                     apply, map_x0, map_dir);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

// Tracking::AddLinesFrom: the gate of every (map line, frame line) pair, then the match on it.  The camera is P, or *P_dev where a kernel left it in device memory.
int line_track_launch(hipStream_t st, const LineTrackParams& P, const LineTrackParams* P_dev, const LineMapDev& map, const LineFrameDev& cur, double md_thr,
                      const LineWork& W, int32_t* matches, double* match_dist, const LineApplyDev& apply) {
  hipLaunchKernelGGL(line_track_gate_kernel, dim3(map.n), dim3(64), 0, st, P, map.x0, map.dir, map.x1, map.x2, map.skip, cur.n_cur, cur.left, cur.loct, cur.right,
                     cur.lmatch, cur.occupied, cur.cell, W.gate, P_dev);
  // `md > mdThr` rejects (Tracking.cc:1099): distances up to and including md_thr pass, where the stereo matcher's tau is strict
  const double tau = std::nextafter(md_thr, kInfD);
  const LineStereoDev in{map.n, cur.n_cur, cur.dim, nullptr, nullptr, nullptr, nullptr, map.desc, cur.desc};
  return line_match_launch<false>(st, LineGateParams{}, in, tau, W, matches, match_dist, apply, map.x0, map.dir);   // (x0, dir: what `apply` hands the frame)
}

// Tracking::MatchLinesLastKF.  kDev: the cameras are in.cur_cam / in.last_cam in device memory and P carries thr_base, md_thr and use_grid only.
template <bool kDev>
int line_lastkf_launch(hipStream_t st, const LastKfParams& P, const LastKfDev& in, int32_t* match_last, uint8_t* created, double* x0, double* dir) {
  hipLaunchKernelGGL(line_lastkf_kernel<kDev>, dim3(in.cur.n_cur), dim3(64), (size_t)in.cur.dim * 4 + 16, st, P, in.cur.n_cur, in.cur.left, in.cur.right, in.cur.lmatch,
                     in.cur.occupied, in.cur.desc, in.last.n_cur, in.last.left, in.last.loct, in.last.right, in.last.lmatch, in.last_skip, in.last.desc, in.last.cell,
                     in.cur.dim, match_last, created, x0, dir, in.cur_cam, in.last_cam);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

// ---------------------------------------------------------------- what the host entry points share around their UploadBlock
// pinned staging for what travels (the uploads, then the results) and device memory for the whole block
int line_block_bind(lld_ctx* ctx, UploadBlock& B) {
  void* hb; int st = lld_ctx_pinned(ctx, B.travel_bytes(), &hb); if (st) return st;
  void* db; st = lld_ctx_scratch(ctx, B.size + 256, &db); if (st) return st;
  B.bind(static_cast<char*>(hb), static_cast<char*>(db));
  return LLD_OK;
}
int line_block_fetch(lld_ctx* ctx, const UploadBlock& B) {
  LLD_HIP_TRY(hipMemcpyAsync(B.h + B.up_bytes, B.d + B.up_bytes, B.down_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LLD_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return LLD_OK;
}
template <class T> void line_result(const UploadBlock& B, const Span<T>& s, T* dst) { if (dst) std::memcpy(dst, B.host(s), s.n * sizeof(T)); }
void line_fill_unmatched(int n, int32_t* matches, double* match_dist) {
  for (int i = 0; i < n; i++) { matches[i] = -1; if (match_dist) match_dist[i] = kInfD; }
}

// Shared body of lld_line_match_greedy (geom == NULL, gate_in optional) and lld_line_match_stereo (geom, the four line arrays, gate_out optional).
int line_match_core(lld_ctx* ctx, const lld_line_stereo_params* geom, const float* left_lines, const int32_t* left_octave, const float* dl, int nq,
                    const float* right_lines, const int32_t* right_octave, const float* dr, int nt, int dim, const uint8_t* gate_in, double tau,
                    int32_t* matches, double* match_dist, uint8_t* gate_out) {
  if (const int st = lld_track::line_limits_check(nq, nt, dim)) return st;
  if (nq == 0) return LLD_OK;
  if (nt == 0) { line_fill_unmatched(nq, matches, match_dist); return LLD_OK; }
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const size_t pairs = (size_t)nq * nt, nq_geom = geom ? nq : 0, nt_geom = geom ? nt : 0;
  UploadBlock B;
  const auto q = B.take<float>(nq, dim), t = B.take<float>(nt, dim), ll = B.take<float>(nq_geom, 4), rl = B.take<float>(nt_geom, 4);
  const auto lo = B.take<int32_t>(nq_geom), ro = B.take<int32_t>(nt_geom);
  const auto gin = B.take<uint8_t>(!geom && gate_in ? pairs : 0);
  B.end_upload();
  const auto m = B.take<int32_t>(nq); const auto d = B.take<double>(nq);
  B.end_download();
  const auto gmat = B.take<uint8_t>(geom ? pairs : 0);
  if (geom && gate_out) B.end_download();                                      // CheckLinePair's matrix travels back only when the caller wants it
  const auto dmat = B.take<double>(pairs); const auto cand = B.take<LineCand>(nq);
  if (const int st = line_block_bind(ctx, B)) return st;
  B.stage(q, dl); B.stage(t, dr); B.stage(ll, left_lines); B.stage(rl, right_lines); B.stage(lo, left_octave); B.stage(ro, right_octave); B.stage(gin, gate_in);
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, ctx->stream));
  LineStereoDev in{nq, nt, dim, nullptr, nullptr, nullptr, nullptr, B.dev(q), B.dev(t)};
  int st;
  if (geom) {
    in.left = B.dev(ll); in.loct = B.dev(lo); in.right = B.dev(rl); in.roct = B.dev(ro);
    st = line_match_launch<true>(ctx->stream, line_gate_params(*geom), in, tau, LineWork{B.dev(gmat), B.dev(dmat), B.dev(cand)}, B.dev(m), B.dev(d), LineApplyDev{}, nullptr, nullptr);
  } else {
    st = line_match_launch<false>(ctx->stream, LineGateParams{}, in, tau, LineWork{gate_in ? B.dev(gin) : nullptr, B.dev(dmat), B.dev(cand)}, B.dev(m), B.dev(d), LineApplyDev{},
                                  nullptr, nullptr);
  }
  if (st) return st;
  if (const int fs = line_block_fetch(ctx, B)) return fs;
  line_result(B, m, matches); line_result(B, d, match_dist); line_result(B, gmat, gate_out);
  return LLD_OK;
}

}  // namespace

namespace lld_track {

int line_limits_check(int rows, int cols, int dim) {
  if (dim > LLD_LINE_DIM_MAX) return LLD_ERR_UNSUPPORTED;
  if (rows <= 0 || cols <= 0) return LLD_OK;
  if ((size_t)cols * 8 + (size_t)dim * 4 > LLD_LINE_LDS_CEILING) return LLD_ERR_UNSUPPORTED;     // one row of distances lives in LDS (cols <= ~19 000)
  if (line_resolve_lds(rows, cols) > LLD_LINE_LDS_CEILING) return LLD_ERR_UNSUPPORTED;           // blk + pick of the resolve (about 38 000 lines on both sides together)
  return LLD_OK;
}
size_t line_work_bytes(int rows, int cols) {                                  // (what line_work_carve lays out, and the slack every scratch block here gets)
  const size_t pairs = (size_t)rows * (size_t)cols;
  return al(pairs) + al(pairs * 8) + al((size_t)rows * sizeof(LineCand)) + 256;
}
int line_cells_dev(hipStream_t st, const float* d_left, int n, double sx, double sy, int32_t* d_cell) {
  if (n > 0) hipLaunchKernelGGL(line_cells_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_left, n, sx, sy, d_cell);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}
// the resident routes: every operand already in HBM, the work triple carved out of d_work
int line_track_launch_dev(hipStream_t st, const LineTrackDevParams* params_d, const LineMapDev& map, const LineFrameDev& cur, double md_thr, void* d_work,
                          int32_t* matches_d, const LineApplyDev& apply) {
  if (map.n <= 0 || cur.n_cur <= 0) return LLD_OK;                            // (nothing to associate: the caller does not read matches_d then)
  if (const int cs = line_limits_check(map.n, cur.n_cur, cur.dim)) return cs;
  return line_track_launch(st, LineTrackParams{}, params_d, map, cur, md_thr, line_work_carve(d_work, map.n, cur.n_cur), matches_d, nullptr, apply);
}
int line_stereo_launch_dev(hipStream_t st, const lld_line_stereo_params& prm, const LineStereoDev& in, void* d_work, int32_t* matches_d, double* match_dist_d) {
  if (in.nl <= 0 || in.nr <= 0) return LLD_OK;
  if (const int cs = line_limits_check(in.nl, in.nr, in.dim)) return cs;
  return line_match_launch<true>(st, line_gate_params(prm), in, prm.tau, line_work_carve(d_work, in.nl, in.nr), matches_d, match_dist_d, LineApplyDev{}, nullptr, nullptr);
}
int line_lastkf_launch_dev(hipStream_t st, const LastKfDev& in, double thr_base, double md_thr, int use_grid, int32_t* match_last, uint8_t* created, double* x0, double* dir) {
  if (in.cur.n_cur <= 0) return LLD_OK;
  LastKfParams P; std::memset(&P, 0, sizeof P);
  P.thr_base = thr_base; P.md_thr = md_thr; P.use_grid = use_grid;
  return line_lastkf_launch<true>(st, P, in, match_last, created, x0, dir);
}

}  // namespace lld_track

extern "C" {

int lld_line_match_greedy(lld_ctx* ctx, const float* dl, int nq, const float* dr, int nt, int dim, const uint8_t* gate, double tau,
                          int32_t* matches, double* match_dist) {
  if (!ctx || !dl || !dr || nq < 0 || nt < 0 || dim <= 0 || !matches) return LLD_ERR_INVALID;
  return line_match_core(ctx, nullptr, nullptr, nullptr, dl, nq, nullptr, nullptr, dr, nt, dim, gate, tau, matches, match_dist, nullptr);
}

int lld_line_match_stereo(lld_ctx* ctx, const lld_line_stereo_params* params, const float* left_lines, const int32_t* left_octave,
                          const float* dl, int nq, const float* right_lines, const int32_t* right_octave, const float* dr, int nt, int dim,
                          int32_t* matches, double* match_dist, uint8_t* gate_out) {
  if (!ctx || !params || nq < 0 || nt < 0 || dim <= 0 || !matches) return LLD_ERR_INVALID;
  if (nq > 0 && (!left_lines || !left_octave || !dl)) return LLD_ERR_INVALID;
  if (nt > 0 && (!right_lines || !right_octave || !dr)) return LLD_ERR_INVALID;
  return line_match_core(ctx, params, left_lines, left_octave, dl, nq, right_lines, right_octave, dr, nt, dim, nullptr, params->tau, matches, match_dist, gate_out);
}

int lld_line_hough_cells(const float* lines, int n, double sx, double sy, int32_t* cell) {
  if (n < 0 || (n > 0 && (!lines || !cell)) || !(sx > 0) || !(sy > 0)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) {
    const double xs = lines[4 * i], ys = lines[4 * i + 1], xe = lines[4 * i + 2], ye = lines[4 * i + 3];
    const HoughCell c = hough_cell(ys - ye, xe - xs, xs * ye - ys * xe, sx, sy);
    cell[i] = c.dist_ind * kHoughAng + c.ang_ind;
  }
  return LLD_OK;
}

int lld_line_track_match(lld_ctx* ctx, const lld_line_track_params* prm, int n_map, const double* map_x0, const double* map_dir, const double* map_x1,
                         const double* map_x2, const uint8_t* map_skip, const float* map_desc, int n_cur, const float* left_lines,
                         const int32_t* left_octave, int n_right, const float* right_lines, const int32_t* line_matches, const uint8_t* occupied,
                         const float* cur_desc, int dim, int32_t* matches, double* match_dist, uint8_t* gate_out) {
  if (!ctx || !prm || n_map < 0 || n_cur < 0 || n_right < 0 || dim <= 0 || !matches) return LLD_ERR_INVALID;
  if (n_map > 0 && (!map_x0 || !map_dir || !map_x1 || !map_x2 || !map_desc)) return LLD_ERR_INVALID;
  if (n_cur > 0 && (!left_lines || !left_octave || !line_matches || !cur_desc)) return LLD_ERR_INVALID;
  if (!prm->monocular && n_right > 0 && !right_lines) return LLD_ERR_INVALID;
  if (!(prm->sx > 0) || !(prm->sy > 0)) return LLD_ERR_INVALID;
  for (int si = 0; si < n_cur; si++) {
    if (left_octave[si] < 0 || left_octave[si] > 64) return LLD_ERR_INVALID;
    if (line_matches[si] >= n_right) return LLD_ERR_INVALID;
  }
  if (const int st = lld_track::line_limits_check(n_map, n_cur, dim)) return st;
  if (n_map == 0) return LLD_OK;
  if (n_cur == 0) { line_fill_unmatched(n_map, matches, match_dist); return LLD_OK; }
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const size_t pairs = (size_t)n_map * n_cur;
  UploadBlock B;
  const auto q = B.take<float>(n_map, dim), t = B.take<float>(n_cur, dim);
  const auto x0 = B.take<double>(n_map, 3), dr = B.take<double>(n_map, 3), x1 = B.take<double>(n_map, 3), x2 = B.take<double>(n_map, 3);
  const auto sk = B.take<uint8_t>(n_map), oc = B.take<uint8_t>(n_cur);
  // (a frame without right lines has no stereo partner either: the gate kernel reads right_lines at line_matches >= 0 only, so n_right == 0 needs no bytes)
  const auto ll = B.take<float>(n_cur, 4), rl = B.take<float>(n_right, 4); const auto lo = B.take<int32_t>(n_cur), lm = B.take<int32_t>(n_cur);
  B.end_upload();
  const auto m = B.take<int32_t>(n_map); const auto d = B.take<double>(n_map);
  B.end_download();
  const auto gate = B.take<uint8_t>(pairs);
  if (gate_out) B.end_download();                                             // the gate matrix travels back only when the caller wants it
  const auto cell = B.take<int32_t>(n_cur); const auto dmat = B.take<double>(pairs); const auto cand = B.take<LineCand>(n_map);
  if (const int st = line_block_bind(ctx, B)) return st;
  B.stage(q, map_desc); B.stage(t, cur_desc); B.stage(x0, map_x0); B.stage(dr, map_dir); B.stage(x1, map_x1); B.stage(x2, map_x2); B.stage(sk, map_skip);
  B.stage(ll, left_lines); B.stage(lo, left_octave); B.stage(rl, right_lines); B.stage(lm, line_matches); B.stage(oc, occupied);
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, ctx->stream));
  LineTrackParams P; std::memset(&P, 0, sizeof P);
  for (int i = 0; i < 9; i++) P.K[i] = prm->K[i];
  for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) P.R[3 * r + c] = prm->T_curr[4 * r + c]; P.t[r] = prm->T_curr[4 * r + 3]; }
  for (int r = 0; r < 3; r++) P.tr[r] = P.t[r] + P.R[3 * r] * prm->b;            // GetTForRight: t + R (b, 0, 0)
  P.thr_base = prm->thr_reproj_base; P.sx = prm->sx; P.sy = prm->sy; P.monocular = prm->monocular; P.use_grid = prm->use_grid;
  int st = lld_track::line_cells_dev(ctx->stream, B.dev(ll), n_cur, P.sx, P.sy, B.dev(cell)); if (st) return st;
  const LineMapDev map{n_map, B.dev(x0), B.dev(dr), B.dev(x1), B.dev(x2), B.dev(sk), B.dev(q)};
  const LineFrameDev cur{n_cur, B.dev(ll), B.dev(lo), B.dev(rl), B.dev(lm), B.dev(oc), B.dev(cell), B.dev(t), dim};
  st = line_track_launch(ctx->stream, P, nullptr, map, cur, prm->md_thr, LineWork{B.dev(gate), B.dev(dmat), B.dev(cand)}, B.dev(m), B.dev(d), LineApplyDev{}); if (st) return st;
  if (const int fs = line_block_fetch(ctx, B)) return fs;
  line_result(B, m, matches); line_result(B, d, match_dist); line_result(B, gate, gate_out);
  return LLD_OK;
}

int lld_line_match_last_frame(lld_ctx* ctx, const lld_line_lastkf_params* prm, int n_cur, const float* cur_left, int n_cur_right, const float* cur_right,
                              const int32_t* cur_line_matches, const uint8_t* cur_occupied, const float* cur_desc, int n_last, const float* last_left,
                              const int32_t* last_left_octave, int n_last_right, const float* last_right, const int32_t* last_line_matches,
                              const uint8_t* last_skip, const float* last_desc, int dim, int32_t* match_last, uint8_t* created, double* x0, double* dir) {
  if (!ctx || !prm || n_cur < 0 || n_last < 0 || n_cur_right < 0 || n_last_right < 0 || dim <= 0 || !match_last || !created || !x0 || !dir) return LLD_ERR_INVALID;
  if (n_cur > 0 && (!cur_left || !cur_line_matches || !cur_desc)) return LLD_ERR_INVALID;
  if (n_last > 0 && (!last_left || !last_left_octave || !last_line_matches || !last_desc)) return LLD_ERR_INVALID;
  if ((n_cur_right > 0 && !cur_right) || (n_last_right > 0 && !last_right)) return LLD_ERR_INVALID;
  if (!(prm->sx > 0) || !(prm->sy > 0)) return LLD_ERR_INVALID;
  for (int i = 0; i < n_cur; i++) if (cur_line_matches[i] >= n_cur_right) return LLD_ERR_INVALID;
  for (int i = 0; i < n_last; i++) if (last_line_matches[i] >= n_last_right || last_left_octave[i] < 0 || last_left_octave[i] > 64) return LLD_ERR_INVALID;
  if (dim > LLD_LINE_LASTKF_DIM_MAX) return LLD_ERR_UNSUPPORTED;              // no resolve here: the kernel's LDS holds one descriptor only
  if (n_cur == 0) return LLD_OK;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  // (the kernel reads a right line at a line match >= 0 only and walks the last frame's arrays up to n_last: an empty array needs no bytes)
  UploadBlock B;
  const auto cl = B.take<float>(n_cur, 4), cr = B.take<float>(n_cur_right, 4), cd = B.take<float>(n_cur, dim); const auto clm = B.take<int32_t>(n_cur); const auto co = B.take<uint8_t>(n_cur);
  const auto ll = B.take<float>(n_last, 4), lr = B.take<float>(n_last_right, 4), ld = B.take<float>(n_last, dim); const auto lo = B.take<int32_t>(n_last), llm = B.take<int32_t>(n_last);
  const auto ls = B.take<uint8_t>(n_last);
  B.end_upload();
  const auto m = B.take<int32_t>(n_cur); const auto c = B.take<uint8_t>(n_cur); const auto x = B.take<double>(n_cur, 3), dd = B.take<double>(n_cur, 3);
  B.end_download();
  const auto cell = B.take<int32_t>(n_last);
  if (const int st = line_block_bind(ctx, B)) return st;
  B.stage(cl, cur_left); B.stage(cr, cur_right); B.stage(clm, cur_line_matches); B.stage(co, cur_occupied); B.stage(cd, cur_desc);
  B.stage(ll, last_left); B.stage(lo, last_left_octave); B.stage(lr, last_right); B.stage(llm, last_line_matches); B.stage(ls, last_skip); B.stage(ld, last_desc);
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, ctx->stream));
  LastKfParams P; std::memset(&P, 0, sizeof P);
  for (int i = 0; i < 9; i++) P.K[i] = prm->K[i];
  for (int r = 0; r < 3; r++) { for (int c3 = 0; c3 < 3; c3++) { P.R[3 * r + c3] = prm->T_curr[4 * r + c3]; P.Rl[3 * r + c3] = prm->T_last[4 * r + c3]; } P.t[r] = prm->T_curr[4 * r + 3]; P.tl[r] = prm->T_last[4 * r + 3]; }
  for (int r = 0; r < 3; r++) { P.tr[r] = P.t[r] + P.R[3 * r] * prm->b; P.tlr[r] = P.tl[r] + P.Rl[3 * r] * prm->b; }      // GetTForRight
  P.thr_base = prm->thr_reproj_base; P.md_thr = prm->md_thr; P.sx = prm->sx; P.sy = prm->sy; P.use_grid = prm->use_grid;
  int st = lld_track::line_cells_dev(ctx->stream, B.dev(ll), n_last, P.sx, P.sy, B.dev(cell)); if (st) return st;
  const LastKfDev in{{n_cur, B.dev(cl), nullptr, B.dev(cr), B.dev(clm), B.dev(co), nullptr, B.dev(cd), dim},
                     {n_last, B.dev(ll), B.dev(lo), B.dev(lr), B.dev(llm), nullptr, B.dev(cell), B.dev(ld), dim}, B.dev(ls), nullptr, nullptr};
  st = line_lastkf_launch<false>(ctx->stream, P, in, B.dev(m), B.dev(c), B.dev(x), B.dev(dd)); if (st) return st;
  if (const int fs = line_block_fetch(ctx, B)) return fs;
  line_result(B, m, match_last); line_result(B, c, created); line_result(B, x, x0); line_result(B, dd, dir);
  return LLD_OK;
}

}  // extern "C"
