// lld_orb_search.hip — guided ORB search on the device: one kernel runs the whole body of an ORBmatcher::Search* /
// Fuse / Frame::ComputeStereoMatches routine (reference lines cited at each rule below).
//
// One workgroup owns one (query set, keypoint set) problem and one LANE owns one query (a query has only tens of candidates, so
// the search is latency-bound: 1024 queries in flight per workgroup hide it; a batch puts one problem on each CU):
//   * the frame's 64x48 keypoint grid (Frame::AssignFeaturesToGrid, src/Frame.cc:294-313) is rebuilt in LDS by a counting
//     sort, so a window query touches only the grid columns GetFeaturesInArea (src/Frame.cc:391-444) would visit;
//   * the keypoint records and (when they fit) the descriptors stay in LDS for all rounds;
//   * every candidate gets the 64-bit key  dist<<32 | visit-order ; the lane keeps the two smallest keys, which is exactly the
//     reference's strict-'<' best / second-best bookkeeping (first visited wins ties) without visiting in order;
//   * the order-dependent rule "keypoint already taken by an earlier query" (the reference writes mvpMapPoints / vpMatched
//     inside its loop) is solved by fixed-point rounds: round r sees the keypoints claimed in round r-1 by queries with a
//     smaller index; when a round changes no match the result is the sequential one (query i is final after i+1 rounds at
//     the latest, in practice 2-4 rounds);
//   * float gates use explicit round-to-nearest intrinsics so no FMA contraction can change a comparison.
#include "lld_common.h"
#include "lld_project_math.h"
#include "lld_track_internal.h"
#include "lld_wave.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kHisto = 30;                 // HISTO_LENGTH, src/ORBmatcher.cc:39
constexpr unsigned long long kNone = ~0ull;

struct TKey {        // one keypoint of the searched frame, LDS resident
  float x, y, ur;
  int32_t meta;      // octave [0,4) | index [4,16) | cell+1 [16,29) (0 = outside the grid) | occupied bit 29
};
__device__ __forceinline__ int tk_oct(int m) { return m & 15; }
__device__ __forceinline__ int tk_idx(int m) { return (m >> 4) & 4095; }
__device__ __forceinline__ int tk_cell(int m) { return ((m >> 16) & 8191) - 1; }
__device__ __forceinline__ bool tk_occ(int m) { return (m >> 29) & 1; }

struct QRec {        // one query, packed on the host
  float u, v, radius, ur, stereo_radius, angle;
  float ea, eb, ec;
  int32_t level_min, level_max;
  int32_t flags;     // 1 valid | 2 blocks | 4 stereo (bStereo1)
  int32_t cs, ce;    // CSR range
  int32_t pad0, pad1;
};

struct Problem {
  int nt, nq;
  const uint32_t* t_desc; const float* t_xy; const int32_t* t_octave; const float* t_uright; const float* t_angle; const uint8_t* t_occupied;
  const uint32_t* q_desc; const QRec* q; const int32_t* cand_idx;
  float min_x, min_y, winv, hinv; int cols, rows;
  int n_levels; float scale[LLD_ORB_MAX_LEVELS], sigma2[LLD_ORB_MAX_LEVELS], inv_sigma2[LLD_ORB_MAX_LEVELS];
  float disp_min, disp_max, epi_x, epi_y; int only_stereo; int image_rows;
  int candidates, gates, tie_last, accept_max, ratio_mode; float nnratio; int sequential, check_orientation;
  int32_t* match; int32_t* best_dist; int32_t* second_dist; uint8_t* removed; int32_t* owner; int32_t* summary;   // summary: n_matches, rounds
  int desc_in_lds, want_owner;
  unsigned long long* cache;   // [nq][kTopK] device scratch of sequential problems: the smallest candidate keys of round 1
  // device-resident chains (lld_frame_track_*): the whole search is skipped unless (*run_if < run_if_below) == (run_if_want != 0)
  const int32_t* run_if; int run_if_below, run_if_want;
  const uint8_t* t_occ_obs;    // non-null: a keypoint is occupied only if t_occupied[k] AND t_occ_obs[k] (its MapPoint has observations, ORBmatcher.cc:98-100, :1409-1411)
  // ... and hands the frame what it matched: CurrentFrame.mvpMapPoints[bestIdx] = pMP (src/ORBmatcher.cc:124, :1427) for every keypoint the search
  // leaves with an owner, if it accepted at least ap_min_matches (Tracking.cc:907: a first search below 20 is thrown away and repeated wider)
  uint8_t* ap_has; float* ap_world; int32_t* ap_id; uint8_t* ap_obs;
  const float* ap_q_pos; const int32_t* ap_q_id; const uint8_t* ap_q_obs;
  int32_t* ap_counts; int ap_min_matches, ap_is_retry;      // ap_counts: [0] n of the first search, [1] n of the search whose matches were taken, [2] retry used
};

// a descriptor (eight words, 16-byte aligned: the frame's array and its copy in LDS) as the two uint4 it is read as
__device__ __forceinline__ const uint4* as_uint4(const uint32_t* desc) { return reinterpret_cast<const uint4*>(desc); }

__device__ __forceinline__ void top2_insert(unsigned long long c, unsigned long long& b1, unsigned long long& b2) {
  if (c < b1) { b2 = b1; b1 = c; } else if (c < b2) { b2 = c; }
}

// the kTopK smallest keys, ascending
constexpr int kTopK = 8;
__device__ __forceinline__ void topk_insert(unsigned long long k, unsigned long long (&c)[kTopK]) {
  if (k < c[kTopK - 1]) {
    c[kTopK - 1] = k;
#pragma unroll
    for (int i = kTopK - 1; i > 0; i--) {
      const unsigned long long lo = c[i] < c[i - 1] ? c[i] : c[i - 1], hi = c[i] < c[i - 1] ? c[i - 1] : c[i];
      c[i - 1] = lo; c[i] = hi;
    }
  }
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
  const int lo = __shfl_xor((int)(v & 0xffffffffu), m), hi = __shfl_xor((int)(v >> 32), m);
  return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}

// Per-candidate skip rules that do not depend on how the candidate was produced.
__device__ __forceinline__ bool gates_pass(const Problem& P, const QRec& Q, const TKey& T, int q, const int* blk, bool use_blk, const float* lvl /* LDS: scale[16], sigma2[16], inv_sigma2[16] */) {
  const int m = T.meta;
  if (tk_occ(m)) return false;
  if (use_blk && blk[tk_idx(m)] < q) return false;
  const int oct = tk_oct(m);
  if (P.gates & LLD_ORB_GATE_LEVEL) {                                     // Frame.cc:422-430, ORBmatcher.cc:386,907
    if (oct < Q.level_min) return false;
    if (Q.level_max >= 0 && oct > Q.level_max) return false;
  }
  if (P.gates & LLD_ORB_GATE_STEREO) {                                    // ORBmatcher.cc:90-95, 1400-1406
    if (T.ur > 0.f && fabsf(__fsub_rn(Q.ur, T.ur)) > Q.stereo_radius) return false;
  }
  if (P.gates & LLD_ORB_GATE_CHI2) {                                      // ORBmatcher.cc:912-936
    const float ex = __fsub_rn(Q.u, T.x), ey = __fsub_rn(Q.v, T.y);
    float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
    if (T.ur >= 0.f) {
      const float er = __fsub_rn(Q.ur, T.ur);
      e2 = __fadd_rn(e2, __fmul_rn(er, er));
      if ((double)__fmul_rn(e2, lvl[32 + oct]) > 7.8) return false;
    } else {
      if ((double)__fmul_rn(e2, lvl[32 + oct]) > 5.99) return false;
    }
  }
  if (P.gates & LLD_ORB_GATE_EPIPOLAR) {                                  // ORBmatcher.cc:720-751, 138-157
    const bool s1 = (Q.flags & 4) != 0, s2 = T.ur >= 0.f;
    if (P.only_stereo && !s2) return false;
    if (!s1 && !s2) {
      const float dx = __fsub_rn(P.epi_x, T.x), dy = __fsub_rn(P.epi_y, T.y);
      if (__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) < __fmul_rn(100.f, lvl[oct])) return false;
    }
    const float num = __fadd_rn(__fadd_rn(__fmul_rn(Q.ea, T.x), __fmul_rn(Q.eb, T.y)), Q.ec);
    const float den = __fadd_rn(__fmul_rn(Q.ea, Q.ea), __fmul_rn(Q.eb, Q.eb));
    if (den == 0.f) return false;
    const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
    if (!((double)dsqr < 3.84 * (double)lvl[16 + oct])) return false;
  }
  return true;
}

// the reference's OpenCV calls on float data, glibc's logf and MapPoint::PredictScale: lld_project_math.h (lld_map_fuse.hip projects with them too)
using lld_proj::cv_transform; using lld_proj::cv_dot3; using lld_proj::cv_norm3; using lld_proj::glibc_logf; using lld_proj::predict_scale;

// Frame::isInFrustum (src/Frame.cc:333-389) for one MapPoint per lane, written straight into the query record of the search
// kernel.  Float / double mixture as the reference's OpenCV calls (see include/lld_amd.h); every float operation is an explicit
// round-to-nearest intrinsic, so nothing is contracted into an FMA.
struct FrustumArgs {
  lld_frame_view V;
  int n;
  const float* pos; const float* nrm; const float* maxd; const float* mind; const uint8_t* has_obs; const uint8_t* skip;
  float scale[LLD_ORB_MAX_LEVELS];
  float cos_limit, th;
  QRec* q; uint8_t* in_view; float* uvr; int32_t* level; float* view_cos;
  const lld_frame_view* view_d;          // non-null: the view lives in device memory (the pose was optimised on the device)
  int32_t* n_in_view;                    // non-null: += the number of points inside the frustum
};

__device__ __forceinline__ bool frustum_one(const FrustumArgs& F, int i) {
  QRec Q; memset(&Q, 0, sizeof(Q));
  Q.level_min = -1; Q.level_max = -1;
  Q.flags = (!F.has_obs || F.has_obs[i]) ? 2 : 0;
  bool ok = !(F.skip && F.skip[i]);
  float u = 0.f, v = 0.f, ur = 0.f, vc = 0.f; int lvl = 0;
  do {
    if (!ok) break;
    const float P[3] = {F.pos[3 * i], F.pos[3 * i + 1], F.pos[3 * i + 2]};
    float Pc[3]; cv_transform(F.V, P, Pc);
    ok = false;
    if (Pc[2] < 0.0f) break;
    const float invz = __fdiv_rn(1.0f, Pc[2]);
    u = __fadd_rn(__fmul_rn(__fmul_rn(F.V.fx, Pc[0]), invz), F.V.cx);
    v = __fadd_rn(__fmul_rn(__fmul_rn(F.V.fy, Pc[1]), invz), F.V.cy);
    if (u < F.V.min_x || u > F.V.max_x) break;
    if (v < F.V.min_y || v > F.V.max_y) break;
    const float maxDistance = __fmul_rn(1.2f, F.maxd[i]), minDistance = __fmul_rn(0.8f, F.mind[i]);
    const float PO[3] = {__fsub_rn(P[0], F.V.Ow[0]), __fsub_rn(P[1], F.V.Ow[1]), __fsub_rn(P[2], F.V.Ow[2])};
    const float dist = cv_norm3(PO);
    if (dist < minDistance || dist > maxDistance) break;
    vc = (float)__ddiv_rn(cv_dot3(PO, F.nrm + 3 * i), (double)dist);             // PO.dot(Pn)/dist
    if (vc < F.cos_limit) break;
    lvl = predict_scale(F.maxd[i], dist, F.V);
    ur = __fsub_rn(u, __fmul_rn(F.V.bf, invz));
    ok = true;
  } while (false);
  if (ok) {
    float r = ((double)vc > 0.998) ? 2.5f : 4.0f;                                // RadiusByViewingCos, src/ORBmatcher.cc:131-137
    if (F.th != 1.0f) r = __fmul_rn(r, F.th);
    const float radius = __fmul_rn(r, F.scale[lvl]);
    Q.u = u; Q.v = v; Q.radius = radius; Q.ur = ur; Q.stereo_radius = radius;
    Q.level_min = lvl - 1; Q.level_max = lvl;
    Q.flags |= 1;
  }
  F.q[i] = Q;
  if (F.in_view) F.in_view[i] = ok ? 1 : 0;
  if (F.uvr) { F.uvr[3 * i] = u; F.uvr[3 * i + 1] = v; F.uvr[3 * i + 2] = ur; }
  if (F.level) F.level[i] = lvl;
  if (F.view_cos) F.view_cos[i] = vc;
  return ok;
}
__global__ __launch_bounds__(256) void frustum_kernel(FrustumArgs F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  if (i < F.n) {
    if (F.view_d) F.V = *F.view_d;
    ok = frustum_one(F, i);
  }
  if (F.n_in_view) {                                                            // nToMatch (src/Tracking.cc:1647), one atomic per wavefront
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(F.n_in_view, __popcll(m));
  }
}

// Projection loop of ORBmatcher::SearchByProjection(Current, Last, th, bMono) (src/ORBmatcher.cc:1352-1386), one lane per keypoint of
// the last frame, written straight into the query record of the search kernel.
struct LastFrameArgs {
  lld_frame_view V;
  int n, direction;
  const float* pos; const uint8_t* valid; const int32_t* octave; const float* angle; const uint8_t* has_obs;
  float scale[LLD_ORB_MAX_LEVELS];
  float th;
  QRec* q; float* uvr;
  const lld_frame_view* view_d;
  const int32_t* run_if; int run_if_below, run_if_want;
};

__device__ __forceinline__ void project_last_one(const LastFrameArgs& F, int i) {
  QRec Q; memset(&Q, 0, sizeof(Q));
  Q.level_min = -1; Q.level_max = -1;
  Q.flags = (!F.has_obs || F.has_obs[i]) ? 2 : 0;
  Q.angle = F.angle ? F.angle[i] : 0.f;
  float u = 0.f, v = 0.f, ur = 0.f;
  if (F.valid[i]) {
    const float P[3] = {F.pos[3 * i], F.pos[3 * i + 1], F.pos[3 * i + 2]};
    float Pc[3]; cv_transform(F.V, P, Pc);                                       // x3Dc = Rcw*x3Dw+tcw
    const float invzc = (float)__ddiv_rn(1.0, (double)Pc[2]);                   // const float invzc = 1.0/x3Dc.at<float>(2);
    if (!(invzc < 0.f)) {
      u = __fadd_rn(__fmul_rn(__fmul_rn(F.V.fx, Pc[0]), invzc), F.V.cx);
      v = __fadd_rn(__fmul_rn(__fmul_rn(F.V.fy, Pc[1]), invzc), F.V.cy);
      if (!(u < F.V.min_x || u > F.V.max_x) && !(v < F.V.min_y || v > F.V.max_y)) {
        const int oct = F.octave[i];
        const float radius = __fmul_rn(F.th, F.scale[oct]);
        ur = __fsub_rn(u, __fmul_rn(F.V.bf, invzc));                             // :1402
        Q.u = u; Q.v = v; Q.radius = radius; Q.ur = ur; Q.stereo_radius = radius;
        if (F.direction > 0) { Q.level_min = oct; Q.level_max = -1; }            // GetFeaturesInArea(u,v,radius,nLastOctave)
        else if (F.direction < 0) { Q.level_min = 0; Q.level_max = oct; }        // (u,v,radius,0,nLastOctave)
        else { Q.level_min = oct - 1; Q.level_max = oct + 1; }
        Q.flags |= 1;
      }
    }
  }
  F.q[i] = Q;
  if (F.uvr) { F.uvr[3 * i] = u; F.uvr[3 * i + 1] = v; F.uvr[3 * i + 2] = ur; }
}
__global__ __launch_bounds__(256) void project_last_frame_kernel(LastFrameArgs F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F.n) return;
  if (F.run_if && ((*F.run_if < F.run_if_below) != (F.run_if_want != 0))) return;
  if (F.view_d) F.V = *F.view_d;
  project_last_one(F, i);
}

__global__ __launch_bounds__(kThreads) void orb_search_kernel(const Problem* __restrict__ problems) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const Problem& P = problems[blockIdx.x];
  if (P.run_if && ((*P.run_if < P.run_if_below) != (P.run_if_want != 0))) return;
  const int nt = P.nt, nq = P.nq, tid = threadIdx.x;
  const int n_cells = P.cols * P.rows;
  const bool grid = P.candidates == LLD_ORB_CAND_GRID, rows = P.candidates == LLD_ORB_CAND_ROWS;
  const bool bucketed = grid || rows;                                           // keypoints sorted by grid cell / by image row
  TKey* tk = reinterpret_cast<TKey*>(lds_raw);                                  // [nt]   (bucketed: sorted by cell)
  uint32_t* dsc = reinterpret_cast<uint32_t*>(tk + nt);                         // [nt][8] descriptors in tk order (when they fit)
  int* blk = reinterpret_cast<int*>(dsc + (P.desc_in_lds ? (size_t)nt * 8 : 0));  // [nt]   first blocking query per keypoint index
  int* cell_start = blk + nt;                                                   // [n_cells + 1]
  int* hist = cell_start + n_cells + 1;                                         // [32]
  int* ctl = hist + 32;                                                         // [8]: 0 changed, 1 accepted, 2 removed, 3..5 kept bins
  int* scan = ctl + 8;                                                          // [kThreads]
  float* lvl = reinterpret_cast<float*>(scan + kThreads);                       // [48] level tables: scale, sigma2, 1/sigma2
  int* holder = reinterpret_cast<int*>(lvl + 48);                               // [nt]   sequential == 2: the query that holds keypoint k (vnMatches21)
  unsigned long long* lkeys = reinterpret_cast<unsigned long long*>((reinterpret_cast<uintptr_t>(holder + nt) + 15) & ~uintptr_t(15));   // [64][kTopK], 16-byte aligned

  // ---------------------------------------------------------------- keypoints into LDS (+ grid counting sort)
  auto load_key = [&](int k, int& cell) -> TKey {
    TKey T; T.x = P.t_xy[2 * k]; T.y = P.t_xy[2 * k + 1]; T.ur = P.t_uright ? P.t_uright[k] : -1.f;
    cell = -1;
    if (grid) {                                                                 // Frame::PosInGrid, src/Frame.cc:446-456
      const int px = (int)roundf(__fmul_rn(__fsub_rn(T.x, P.min_x), P.winv)), py = (int)roundf(__fmul_rn(__fsub_rn(T.y, P.min_y), P.hinv));
      if (px >= 0 && px < P.cols && py >= 0 && py < P.rows) cell = px * P.rows + py;
    } else if (rows) {                                                          // bucket = (octave, image row) of the keypoint (search aid only)
      cell = min(P.t_octave[k], P.cols - 1) * P.rows + min(max((int)floorf(T.y), 0), P.rows - 1);
    }
    T.meta = (P.t_octave[k] & 15) | (k << 4) | ((cell + 1) << 16) | ((P.t_occupied && P.t_occupied[k] && (!P.t_occ_obs || P.t_occ_obs[k])) ? (1 << 29) : 0);
    return T;
  };
  auto place = [&](int pos, int k, const TKey& T) {
    tk[pos] = T;
    if (P.desc_in_lds) {
      const uint4* src = reinterpret_cast<const uint4*>(P.t_desc + 8 * (size_t)k);
      uint4* dst = reinterpret_cast<uint4*>(dsc + 8 * (size_t)pos);
      dst[0] = src[0]; dst[1] = src[1];
    }
  };
  for (int c = tid; c <= n_cells; c += kThreads) cell_start[c] = 0;
  for (int k = tid; k < nt; k += kThreads) blk[k] = 0x7fffffff;
  if (tid < 32) hist[tid] = 0;
  if (tid < 8) ctl[tid] = 0;
  if (tid < LLD_ORB_MAX_LEVELS) { lvl[tid] = P.scale[tid]; lvl[16 + tid] = P.sigma2[tid]; lvl[32 + tid] = P.inv_sigma2[tid]; }
  __syncthreads();
  for (int k = tid; k < nt; k += kThreads) {
    int cell; const TKey T = load_key(k, cell);
    if (!bucketed) place(k, k, T);
    else if (cell >= 0) atomicAdd(&cell_start[cell], 1);
  }
  __syncthreads();
  if (bucketed) {
    // scan of the cell counts (each thread owns a contiguous run of cells) into cell ENDS, then an unordered placement that
    // counts every cell's end down to its start - one array serves as counter, cursor and final cell_start (end of cell c =
    // start of cell c + 1).  The position inside a cell is irrelevant: ties are broken by the key, not by the visit position.
    const int per = (n_cells + kThreads - 1) / kThreads, c0 = min(tid * per, n_cells), c1 = min(c0 + per, n_cells);
    int sum = 0;
    for (int c = c0; c < c1; c++) sum += cell_start[c];
    // block-wide exclusive prefix of the per-thread sums: shuffle scan inside the wavefront + the 16 wavefront totals
    int incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(incl, off); if ((tid & 63) >= off) incl += t; }
    if ((tid & 63) == 63) scan[tid >> 6] = incl;
    __syncthreads();
    int run = incl - sum, total = 0;
    for (int w = 0; w < kThreads / 64; w++) { const int t = scan[w]; if (w < (tid >> 6)) run += t; total += t; }
    for (int c = c0; c < c1; c++) { run += cell_start[c]; cell_start[c] = run; }
    if (tid == kThreads - 1) cell_start[n_cells] = total;
    __syncthreads();
    for (int k = tid; k < nt; k += kThreads) {
      int cell; const TKey T = load_key(k, cell);
      if (cell >= 0) place(atomicSub(&cell_start[cell], 1) - 1, k, T);
    }
  }
  for (int q = tid; q < nq; q += kThreads) P.match[q] = -2;
  __syncthreads();

  // every candidate of query q that passes the gates, its kTopK smallest keys (distance, then visit order) into c.  `steal`: the
  // SearchForInitialization rule - a keypoint held by an earlier query with a distance <= this one is no candidate (blk = vMatchedDistance)
  auto scan_candidates = [&](int q, const QRec& Q, unsigned long long (&c)[kTopK], bool use_blk, bool steal) {
#pragma unroll
        for (int i = 0; i < kTopK; i++) c[i] = kNone;
        uint32_t qd[8];
        {
          const uint4 a = *reinterpret_cast<const uint4*>(P.q_desc + 8 * (size_t)q), b = *reinterpret_cast<const uint4*>(P.q_desc + 8 * (size_t)q + 4);
          qd[0] = a.x; qd[1] = a.y; qd[2] = a.z; qd[3] = a.w; qd[4] = b.x; qd[5] = b.y; qd[6] = b.z; qd[7] = b.w;
        }
        auto visit = [&](int pos, const TKey& T, unsigned key) {
          if (!gates_pass(P, Q, T, q, blk, use_blk, lvl)) return;
          const int d = P.desc_in_lds ? lld_wave::hamming256(qd, as_uint4(dsc + 8 * (size_t)pos)) : lld_wave::hamming256(qd, as_uint4(P.t_desc + 8 * (size_t)tk_idx(T.meta)));
          if (steal && blk[tk_idx(T.meta)] <= d) return;                                                           // ORBmatcher.cc:443-444
          if (P.tie_last) key = ~key;
          topk_insert(((unsigned long long)d << 32) | key, c);
        };
        if (grid) {
          // GetFeaturesInArea cell range, src/Frame.cc:396-410 (float arithmetic, floor/ceil, clamps and early returns)
          const int minCX = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(Q.u, P.min_x), Q.radius), P.winv)));
          const int maxCX = min(P.cols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(Q.u, P.min_x), Q.radius), P.winv)));
          const int minCY = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(Q.v, P.min_y), Q.radius), P.hinv)));
          const int maxCY = min(P.rows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(Q.v, P.min_y), Q.radius), P.hinv)));
          if (minCX < P.cols && maxCX >= 0 && minCY < P.rows && maxCY >= 0 && maxCY >= minCY) {
            for (int ix = minCX; ix <= maxCX; ix++) {
              const int j0 = cell_start[ix * P.rows + minCY], j1 = cell_start[ix * P.rows + maxCY + 1];   // one column = one contiguous run
              for (int j = j0; j < j1; j++) {
                const TKey T = tk[j];
                if (!(fabsf(__fsub_rn(T.x, Q.u)) < Q.radius && fabsf(__fsub_rn(T.y, Q.v)) < Q.radius)) continue;   // Frame.cc:433-437
                visit(j, T, ((unsigned)tk_cell(T.meta) << 12) | (unsigned)tk_idx(T.meta));
              }
            }
          }
        } else if (P.candidates == LLD_ORB_CAND_CSR) {
          for (int p = Q.cs; p < Q.ce; p++) {
            const int k = P.cand_idx[p];
            visit(k, tk[k], (unsigned)(p - Q.cs));
          }
        } else if (rows) {
          // Frame::ComputeStereoMatches: vRowIndices[vL] holds right keypoint iR iff floor(yR-r) <= (int)vL <= ceil(yR+r), r = 2*scale[octave]
          // (src/Frame.cc:546-556).  Only the row buckets that can satisfy this are scanned; the exact test follows.
          const float minU = __fsub_rn(Q.u, P.disp_max), maxU = __fsub_rn(Q.u, P.disp_min);                       // Frame.cc:574-575
          const long long row = (long long)Q.v;                                                                    // vRowIndices[vL], :569
          if (!(maxU < 0.f) && (P.image_rows <= 0 || (row >= 0 && row < P.image_rows))) {                          // :577-578; a row outside the image has no candidates
            // buckets are (octave, row): only the octaves the level gate admits are scanned, each with its own row margin
            int o_lo = 0, o_hi = P.cols - 1;
            if (P.gates & LLD_ORB_GATE_LEVEL) { o_lo = min(max(Q.level_min, 0), P.cols - 1); if (Q.level_max >= 0) o_hi = min(Q.level_max, P.cols - 1); }
            for (int o = o_lo; o <= o_hi; o++) {
              float rmax = __fmul_rn(2.0f, lvl[o]);
              if (o == P.cols - 1) for (int l = o + 1; l < LLD_ORB_MAX_LEVELS; l++) rmax = fmaxf(rmax, __fmul_rn(2.0f, lvl[l]));   // clamped octaves
              const long long margin = (long long)ceilf(rmax) + 2;
              const int lo = (int)min(max(row - margin, 0ll), (long long)P.rows - 1), hi = (int)min(max(row + margin, 0ll), (long long)P.rows - 1);
              for (int j = cell_start[o * P.rows + lo]; j < cell_start[o * P.rows + hi + 1]; j++) {
                const TKey T = tk[j];
                const float r = __fmul_rn(2.0f, lvl[tk_oct(T.meta)]);
                const long long maxr = (long long)ceilf(__fadd_rn(T.y, r)), minr = (long long)floorf(__fsub_rn(T.y, r));
                if (row < minr || row > maxr) continue;
                if (!(T.x >= minU && T.x <= maxU)) continue;                                                       // :594-596
                visit(j, T, (unsigned)tk_idx(T.meta));
              }
            }
          }
        } else {
          for (int k = 0; k < nt; k++) visit(k, tk[k], (unsigned)k);
        }
  };

  // ---------------------------------------------------------------- fixed-point rounds, one lane per query
  int rounds = 0;
  for (;;) {
    rounds++;
    for (int q = tid; q < nq; q += kThreads) {
      const QRec Q = P.q[q];
      unsigned long long b1 = kNone, b2 = kNone;
      auto decode = [&](unsigned long long c) -> int {
        unsigned key = (unsigned)(c & 0xffffffffu);
        if (P.tie_last) key = ~key;
        if (grid) return (int)(key & 4095u);
        if (P.candidates == LLD_ORB_CAND_CSR) return P.cand_idx[Q.cs + (int)key];
        return (int)key;
      };
      if (Q.flags & 1) {
        // The candidates of a query, sorted by key, do not depend on the round; only which of them are blocked does.  Round 1
        // keeps the kTopK smallest keys; later rounds take the first two unblocked ones from that list and rescan only when
        // the list was full and fewer than two of its entries are still free.
        unsigned long long c[kTopK];
#pragma unroll
        for (int i = 0; i < kTopK; i++) c[i] = kNone;
        auto pick = [&]() {
          int found = 0; b1 = kNone; b2 = kNone;
          auto take = [&](unsigned long long k) {
            if (k != kNone && !(P.sequential && blk[decode(k)] < q)) {
              b1 = found == 0 ? k : b1; b2 = found == 1 ? k : b2;          // selects, so that b1 / b2 stay in registers
              found++;
            }
          };
#pragma unroll
          for (int i = 0; i < kTopK; i++) take(c[i]);
          return found;
        };
        bool need_scan = rounds == 1;
        if (rounds > 1) {
#pragma unroll
          for (int i = 0; i < kTopK; i += 2) {
            const ulonglong2 t2 = *reinterpret_cast<const ulonglong2*>(P.cache + kTopK * (size_t)q + i);
            c[i] = t2.x; c[i + 1] = t2.y;
          }
          need_scan = pick() < 2 && c[kTopK - 1] != kNone;
        }
        if (need_scan) {
          scan_candidates(q, Q, c, rounds > 1, false);
        if (rounds == 1 && P.sequential) {
#pragma unroll
          for (int i = 0; i < kTopK; i += 2) *reinterpret_cast<ulonglong2*>(P.cache + kTopK * (size_t)q + i) = make_ulonglong2(c[i], c[i + 1]);
        }
        pick();
        }
      }
      int m = -1, bd = 256, sd = 256;
      if (b1 != kNone) {
        bd = (int)(b1 >> 32);
        const int bi = decode(b1);
        bool ok = bd <= P.accept_max;
        if (b2 != kNone) sd = (int)(b2 >> 32);
        if (ok && P.ratio_mode == 1) ok = (float)bd < __fmul_rn(P.nnratio, (float)sd);                            // ORBmatcher.cc:226-228
        if (ok && P.ratio_mode == 2) {                                                                            // :118-121
          const int lvl1 = P.t_octave[bi], lvl2 = (b2 != kNone) ? P.t_octave[decode(b2)] : -1;
          if (lvl1 == lvl2 && (float)bd > __fmul_rn(P.nnratio, (float)sd)) ok = false;
        }
        if (ok) m = bi;
      }
      if (P.match[q] != m) { P.match[q] = m; ctl[0] = 1; }
      P.best_dist[q] = bd; P.second_dist[q] = sd;
    }
    __syncthreads();
    const int changed = ctl[0];
    __syncthreads();
    if (P.sequential == 2) {
      // ---- ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:417-476): the one order-dependent rule that is not an occupancy.  A
      // candidate is skipped when an EARLIER query holds it with a distance <= this one (vMatchedDistance[i2] <= dist, :443), and an
      // accepted query takes the keypoint away from its holder (:458-465).  Round 1 above left every query's kTopK smallest candidates
      // (distance, then visit order) in P.cache; wavefront 0 walks the queries in order with lane i on list entry i: the first two
      // entries still free are bestDist / bestDist2.  Only when fewer than two of a FULL list are free is the window scanned again (by
      // one lane, with the rule applied).  blk = vMatchedDistance (INT_MAX so far), holder = vnMatches21; the rotation histogram
      // counts every acceptance, also those stolen later (rotHist is never cleaned, :466-476).
      for (int k = tid; k < nt; k += kThreads) holder[k] = -1;
      __syncthreads();
      if (tid < 64) {
        // No global load sits on the query-to-query chain: a chunk of 64 queries is loaded lane-wise (lane l: flags and list of query
        // q0 + l), the walk takes query i's values out of lane i's registers with v_readlane, results stay in lane registers until the
        // chunk is done, and the rotation bins (which need both angles) are counted afterwards by all lanes from the recorded acceptances.
        auto dec = [&](unsigned long long c) -> int { const unsigned kk = (unsigned)(c & 0xffffffffu); return grid ? (int)(kk & 4095u) : (int)kk; };
        auto rl64 = [&](unsigned long long v, int lane) -> unsigned long long {
          const int lo = __builtin_amdgcn_readlane((int)(v & 0xffffffffu), lane), hi = __builtin_amdgcn_readlane((int)(v >> 32), lane);
          return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
        };
        // the window of query q once more, with the take-over rule, by the whole wavefront: lanes stride over the candidates of a grid
        // column (or over all keypoints), keep their two smallest keys, and a butterfly merges the 64 pairs
        auto wave_rescan = [&](int q, unsigned long long& r1, unsigned long long& r2) {
          const QRec Q = P.q[q];
          uint32_t qd[8];
          {
            const uint4 a = *reinterpret_cast<const uint4*>(P.q_desc + 8 * (size_t)q), b = *reinterpret_cast<const uint4*>(P.q_desc + 8 * (size_t)q + 4);
            qd[0] = a.x; qd[1] = a.y; qd[2] = a.z; qd[3] = a.w; qd[4] = b.x; qd[5] = b.y; qd[6] = b.z; qd[7] = b.w;
          }
          unsigned long long t1 = kNone, t2 = kNone;
          auto visit = [&](int pos, const TKey& T, unsigned key) {
            if (!gates_pass(P, Q, T, q, blk, false, lvl)) return;
            const int d = P.desc_in_lds ? lld_wave::hamming256(qd, as_uint4(dsc + 8 * (size_t)pos)) : lld_wave::hamming256(qd, as_uint4(P.t_desc + 8 * (size_t)tk_idx(T.meta)));
            if (blk[tk_idx(T.meta)] <= d) return;                                                                  // ORBmatcher.cc:443-444
            top2_insert(((unsigned long long)d << 32) | key, t1, t2);
          };
          if (grid) {
            const int minCX = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(Q.u, P.min_x), Q.radius), P.winv)));
            const int maxCX = min(P.cols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(Q.u, P.min_x), Q.radius), P.winv)));
            const int minCY = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(Q.v, P.min_y), Q.radius), P.hinv)));
            const int maxCY = min(P.rows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(Q.v, P.min_y), Q.radius), P.hinv)));
            if (minCX < P.cols && maxCX >= 0 && minCY < P.rows && maxCY >= 0 && maxCY >= minCY) {
              for (int ix = minCX; ix <= maxCX; ix++) {
                const int j0 = cell_start[ix * P.rows + minCY], j1 = cell_start[ix * P.rows + maxCY + 1];
                for (int j = j0 + tid; j < j1; j += 64) {
                  const TKey T = tk[j];
                  if (!(fabsf(__fsub_rn(T.x, Q.u)) < Q.radius && fabsf(__fsub_rn(T.y, Q.v)) < Q.radius)) continue;
                  visit(j, T, ((unsigned)tk_cell(T.meta) << 12) | (unsigned)tk_idx(T.meta));
                }
              }
            }
          } else {
            for (int k = tid; k < nt; k += 64) visit(k, tk[k], (unsigned)k);
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o1 = shfl_xor_u64(t1, off), o2 = shfl_xor_u64(t2, off);
            const unsigned long long lo = t1 < o1 ? t1 : o1, hi = t1 < o1 ? o1 : t1, s2 = t2 < o2 ? t2 : o2;
            t1 = lo; t2 = hi < s2 ? hi : s2;
          }
          r1 = t1; r2 = t2;
        };
        for (int q0 = 0; q0 < nq; q0 += 64) {
          const int ql = q0 + tid;
          int fl = 0;
          {
            unsigned long long kk[kTopK];
#pragma unroll
            for (int t = 0; t < kTopK; t++) kk[t] = kNone;
            if (ql < nq) {
              fl = P.q[ql].flags;
#pragma unroll
              for (int t = 0; t < kTopK; t += 2) {
                const ulonglong2 t2 = *reinterpret_cast<const ulonglong2*>(P.cache + kTopK * (size_t)ql + t);
                kk[t] = t2.x; kk[t + 1] = t2.y;
              }
            }
#pragma unroll
            for (int t = 0; t < kTopK; t += 2) *reinterpret_cast<ulonglong2*>(lkeys + kTopK * tid + t) = make_ulonglong2(kk[t], kk[t + 1]);
          }
          int m_l = -1, bd_l = 256, sd_l = 256, acc_l = -1;                      // this lane's query: match, distances, keypoint accepted at its turn
          const int cnt = min(64, nq - q0);
          const int tl = tid < kTopK ? tid : 0;
          unsigned long long key_n = lkeys[tl];                                 // query 0 of the chunk; the next one is always in flight
          for (int i = 0; i < cnt; i++) {
            unsigned long long key = tid < kTopK ? key_n : kNone;
            const bool full = __builtin_amdgcn_readlane((int)(key_n >> 32), kTopK - 1) != -1 || __builtin_amdgcn_readlane((int)key_n, kTopK - 1) != -1;
            key_n = lkeys[kTopK * min(i + 1, 63) + tl];
            const int flags = __builtin_amdgcn_readlane(fl, i);
            if (!(flags & 1)) continue;
            const int q = q0 + i;
            const int kp = key != kNone ? dec(key) : 0;
            const int vmd = blk[kp], hold = holder[kp];                         // vMatchedDistance and vnMatches21 of this lane's candidate
            const bool free_ = key != kNone && vmd > (int)(key >> 32);
            const unsigned long long fm = __ballot(free_) & ((1ull << kTopK) - 1);
            unsigned long long b1 = kNone, b2 = kNone;
            int prev = -1;
            if (__popcll(fm) < 2 && full) {
              rounds++;                                                         // reported: 1 + the number of rescans
              wave_rescan(q, b1, b2);
              if (b1 != kNone) prev = holder[dec(b1)];
            } else {
              const unsigned long long fm2 = fm & (fm - 1);
              if (fm) { const int l1 = __ffsll((long long)fm) - 1; b1 = rl64(key, l1); prev = __builtin_amdgcn_readlane(hold, l1); }
              if (fm2) b2 = rl64(key, __ffsll((long long)fm2) - 1);
            }
            int m = -1, bd = 256, sd = 256;
            if (b1 != kNone) {
              bd = (int)(b1 >> 32);
              const int bi = dec(b1);
              bool ok = bd <= P.accept_max;
              if (b2 != kNone) sd = (int)(b2 >> 32);
              if (ok && P.ratio_mode == 1) ok = (float)bd < __fmul_rn(P.nnratio, (float)sd);                      // ORBmatcher.cc:456
              if (ok) m = bi;
            }
            if (m >= 0) {                                                       // uniform: every lane holds the same m
              if (prev >= q0) { if (tid == prev - q0) m_l = -1; }               // :460-461, the holder is in this chunk
              else if (prev >= 0 && tid == 0) P.match[prev] = -1;
              if (tid == 0) { holder[m] = q; blk[m] = bd; }
            }
            if (tid == i) { m_l = m; bd_l = bd; sd_l = sd; acc_l = m; }
          }
          if (ql < nq) {
            P.match[ql] = m_l; P.best_dist[ql] = bd_l; P.second_dist[ql] = sd_l;
            P.cache[kTopK * (size_t)ql] = (unsigned long long)(long long)acc_l;   // the list is spent: its first word records the acceptance
          }
        }
      }
      __syncthreads();
      if (P.check_orientation) {                                                // rotHist of every acceptance (:468-476)
        for (int q = tid; q < nq; q += kThreads) {
          const int acc = (int)(long long)P.cache[kTopK * (size_t)q];
          if (acc < 0 || !(P.q[q].flags & 1)) continue;
          float rot = __fsub_rn(P.q[q].angle, P.t_angle[acc]);
          if (rot < 0.f) rot = __fadd_rn(rot, 360.0f);
          int bin = (int)roundf(__fmul_rn(rot, 1.0f / kHisto));
          if (bin == kHisto) bin = 0;
          atomicAdd(&hist[min(max(bin, 0), kHisto - 1)], 1);
        }
      }
      __syncthreads();
      break;
    }
    if (!P.sequential || !changed) break;
    if (tid == 0) ctl[0] = 0;
    for (int k = tid; k < nt; k += kThreads) blk[k] = 0x7fffffff;
    __syncthreads();
    for (int q = tid; q < nq; q += kThreads) {
      const int m = P.match[q];
      if (m >= 0 && (P.q[q].flags & 2)) atomicMin(&blk[m], q);
    }
    __syncthreads();
  }

  // ---------------------------------------------------------------- rotation histogram, owners, counts
  int* owner = blk;                                                             // blockers are dead now
  for (int k = tid; k < nt; k += kThreads) owner[k] = -1;
  __syncthreads();
  for (int q = tid; q < nq; q += kThreads) {
    const int m = P.match[q];
    int bin = 255;
    if (m >= 0) {
      atomicAdd(&ctl[1], 1);
      atomicMax(&owner[m], q);
      if (P.check_orientation) {                                                // ORBmatcher.cc:1431-1440
        float rot = __fsub_rn(P.q[q].angle, P.t_angle[m]);
        if (rot < 0.f) rot = __fadd_rn(rot, 360.0f);
        bin = (int)roundf(__fmul_rn(rot, 1.0f / kHisto));
        if (bin == kHisto) bin = 0;
        bin = min(max(bin, 0), kHisto - 1);                                     // the reference asserts the range
        if (P.sequential != 2) atomicAdd(&hist[bin], 1);                        // (steal mode counted every acceptance in its pass)
      }
    }
    P.removed[q] = (uint8_t)bin;
  }
  __syncthreads();
  if (tid == 0) {
    int ind1 = -1, ind2 = -1, ind3 = -1;
    if (P.check_orientation) {                                                  // ComputeThreeMaxima, ORBmatcher.cc:1601-1642
      int max1 = 0, max2 = 0, max3 = 0;
      for (int i = 0; i < kHisto; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
      }
      if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
      else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    }
    ctl[3] = ind1; ctl[4] = ind2; ctl[5] = ind3;
  }
  __syncthreads();
  for (int q = tid; q < nq; q += kThreads) {
    const int bin = P.removed[q];
    uint8_t rem = 0;
    if (P.check_orientation && bin != 255 && bin != ctl[3] && bin != ctl[4] && bin != ctl[5]) {
      rem = 1;
      atomicAdd(&ctl[2], 1);
      owner[P.match[q]] = -2;                                                   // slot NULLed, ORBmatcher.cc:1452-1460
    }
    P.removed[q] = rem;
  }
  __syncthreads();
  if (P.want_owner) for (int k = tid; k < nt; k += kThreads) P.owner[k] = owner[k];
  if (tid == 0) { P.summary[0] = ctl[1] - ctl[2]; P.summary[1] = rounds; }
  if (P.ap_has) {
    const int n_matches = ctl[1] - ctl[2];
    const bool take = n_matches >= P.ap_min_matches;
    if (tid == 0) {
      if (!P.ap_is_retry) { P.ap_counts[0] = n_matches; if (take) { P.ap_counts[1] = n_matches; P.ap_counts[2] = 0; } }
      else { P.ap_counts[1] = n_matches; P.ap_counts[2] = 1; }
    }
    if (take) {
      for (int k = tid; k < nt; k += kThreads) {
        const int q = owner[k];
        if (q < 0) continue;
        P.ap_has[k] = 1; P.ap_id[k] = P.ap_q_id[q]; P.ap_obs[k] = P.ap_q_obs ? P.ap_q_obs[q] : 1;
        P.ap_world[3 * k] = P.ap_q_pos[3 * q]; P.ap_world[3 * k + 1] = P.ap_q_pos[3 * q + 1]; P.ap_world[3 * k + 2] = P.ap_q_pos[3 * q + 2];
      }
    }
  }
}

// Projection loop of ORBmatcher::Fuse(KeyFrame*, vpMapPoints, th) (src/ORBmatcher.cc:841-890), one lane per MapPoint.
struct FuseArgs {
  lld_frame_view V;
  int n;
  const float* pos; const float* nrm; const float* maxd; const float* mind; const uint8_t* skip;
  float scale[LLD_ORB_MAX_LEVELS];
  float th;
  QRec* q; float* uvr;
};

__global__ __launch_bounds__(256) void project_fuse_kernel(FuseArgs F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F.n) return;
  QRec Q; memset(&Q, 0, sizeof(Q));
  Q.level_min = -1; Q.level_max = -1;
  float u = 0.f, v = 0.f, ur = 0.f;
  do {
    if (F.skip && F.skip[i]) break;
    const float P[3] = {F.pos[3 * i], F.pos[3 * i + 1], F.pos[3 * i + 2]};
    float Pc[3]; cv_transform(F.V, P, Pc);
    if (Pc[2] < 0.0f) break;
    const float invz = __fdiv_rn(1.0f, Pc[2]);
    const float x = __fmul_rn(Pc[0], invz), y = __fmul_rn(Pc[1], invz);
    u = __fadd_rn(__fmul_rn(F.V.fx, x), F.V.cx);
    v = __fadd_rn(__fmul_rn(F.V.fy, y), F.V.cy);
    if (!(u >= F.V.min_x && u < F.V.max_x && v >= F.V.min_y && v < F.V.max_y)) break;      // KeyFrame::IsInImage
    ur = __fsub_rn(u, __fmul_rn(F.V.bf, invz));
    const float maxDistance = __fmul_rn(1.2f, F.maxd[i]), minDistance = __fmul_rn(0.8f, F.mind[i]);
    const float PO[3] = {__fsub_rn(P[0], F.V.Ow[0]), __fsub_rn(P[1], F.V.Ow[1]), __fsub_rn(P[2], F.V.Ow[2])};
    const float dist3D = cv_norm3(PO);
    if (dist3D < minDistance || dist3D > maxDistance) break;
    if (cv_dot3(PO, F.nrm + 3 * i) < __dmul_rn(0.5, (double)dist3D)) break;                   // PO.dot(Pn)<0.5*dist3D
    const int lvl = predict_scale(F.maxd[i], dist3D, F.V);
    Q.u = u; Q.v = v; Q.ur = ur; Q.radius = __fmul_rn(F.th, F.scale[lvl]);
    Q.level_min = lvl - 1; Q.level_max = lvl;
    Q.flags = 1;
  } while (false);
  F.q[i] = Q;
  if (F.uvr) { F.uvr[3 * i] = u; F.uvr[3 * i + 1] = v; F.uvr[3 * i + 2] = ur; }
}

// Projection loops of the relocalisation / loop-closing matchers (lld_orb_search_projected), one lane per MapPoint; `routine` selects
// the reference's sequence of tests and its float arithmetic (see include/lld_amd.h).
struct ProjGenArgs {
  lld_frame_view V;
  int n, routine;
  float sR[9], t2[3];
  const float* pos; const float* nrm; const float* maxd; const float* mind; const uint8_t* skip; const float* angle;
  float scale[LLD_ORB_MAX_LEVELS];
  float th;
  QRec* q; float* uv; int32_t* level;
};

// (scale: the level table, F.scale for a kernel whose argument F is)
__device__ __forceinline__ void project_general_one(const ProjGenArgs& F, const float* scale, int i) {
  QRec Q; memset(&Q, 0, sizeof(Q));
  Q.level_min = -1; Q.level_max = -1;
  Q.angle = F.angle ? F.angle[i] : 0.f;
  float u = 0.f, v = 0.f; int lvl = 0;
  do {
    if (F.skip && F.skip[i]) break;
    const float P[3] = {F.pos[3 * i], F.pos[3 * i + 1], F.pos[3 * i + 2]};
    float Pc[3]; cv_transform(F.V, P, Pc);                                       // Rcw*p3Dw+tcw: one cv::gemm
    if (F.routine == LLD_ORB_PROJ_SIM3_DIR) {                                    // p3Dc2 = sR21*p3Dc1 + t21: a second cv::gemm
      float P2[3];
#pragma unroll
      for (int r = 0; r < 3; r++)
        P2[r] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn((double)F.sR[3 * r], (double)Pc[0]), __dmul_rn((double)F.sR[3 * r + 1], (double)Pc[1])),
                                           __dmul_rn((double)F.sR[3 * r + 2], (double)Pc[2])), (double)F.t2[r]);
      Pc[0] = P2[0]; Pc[1] = P2[1]; Pc[2] = P2[2];
    }
    float dist;
    if (F.routine == LLD_ORB_PROJ_RELOC) {
      const float invzc = (float)__ddiv_rn(1.0, (double)Pc[2]);                 // const float invzc = 1.0/x3Dc.at<float>(2);  (no depth test, :1499-1503)
      u = __fadd_rn(__fmul_rn(__fmul_rn(F.V.fx, Pc[0]), invzc), F.V.cx);
      v = __fadd_rn(__fmul_rn(__fmul_rn(F.V.fy, Pc[1]), invzc), F.V.cy);
      if (u < F.V.min_x || u > F.V.max_x) break;
      if (v < F.V.min_y || v > F.V.max_y) break;
    } else {
      if (Pc[2] < 0.0f) break;
      // `1/z` is a float division in :328, `1.0/z` a double one rounded to float in :1019, :1168, :1246
      const float invz = F.routine == LLD_ORB_PROJ_KF_SIM3 ? __fdiv_rn(1.0f, Pc[2]) : (float)__ddiv_rn(1.0, (double)Pc[2]);
      const float x = __fmul_rn(Pc[0], invz), y = __fmul_rn(Pc[1], invz);
      u = __fadd_rn(__fmul_rn(F.V.fx, x), F.V.cx);
      v = __fadd_rn(__fmul_rn(F.V.fy, y), F.V.cy);
      if (!(u >= F.V.min_x && u < F.V.max_x && v >= F.V.min_y && v < F.V.max_y)) break;      // KeyFrame::IsInImage
    }
    const float maxDistance = __fmul_rn(1.2f, F.maxd[i]), minDistance = __fmul_rn(0.8f, F.mind[i]);
    if (F.routine == LLD_ORB_PROJ_SIM3_DIR) dist = cv_norm3(Pc);                  // cv::norm(p3Dc2)
    else {
      const float PO[3] = {__fsub_rn(P[0], F.V.Ow[0]), __fsub_rn(P[1], F.V.Ow[1]), __fsub_rn(P[2], F.V.Ow[2])};
      dist = cv_norm3(PO);
      if (dist < minDistance || dist > maxDistance) break;
      if (F.routine != LLD_ORB_PROJ_RELOC && cv_dot3(PO, F.nrm + 3 * i) < __dmul_rn(0.5, (double)dist)) break;   // PO.dot(Pn)<0.5*dist
    }
    if (dist < minDistance || dist > maxDistance) break;
    lvl = predict_scale(F.maxd[i], dist, F.V);
    Q.u = u; Q.v = v; Q.radius = __fmul_rn(F.th, scale[lvl]);
    Q.level_min = lvl - 1; Q.level_max = F.routine == LLD_ORB_PROJ_RELOC ? lvl + 1 : lvl;
    Q.flags = 1 | 2;                                                              // valid; a match blocks the keypoint for later points (routines with occupancy)
  } while (false);
  F.q[i] = Q;
  if (F.uv) { F.uv[2 * i] = u; F.uv[2 * i + 1] = v; }
  if (F.level) F.level[i] = lvl;
}
__global__ __launch_bounds__(256) void project_general_kernel(ProjGenArgs F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= F.n) return;
  project_general_one(F, F.scale, i);
}

// LLD_ORB_PROJ_RELOC for slot blockIdx.y of Tracking::Relocalization's side-by-side candidates (lld_frame_reloc.hip): the slot's own MapPoints,
// skip bytes (bad or already found), view (device memory: the pose was optimised on the device) and predicate.
struct ProjRelocSlotsArgs { const lld_track::RelocProjSlot* slots; float scale[LLD_ORB_MAX_LEVELS]; float th; };
__global__ __launch_bounds__(256) void project_reloc_slots_kernel(ProjRelocSlotsArgs A) {
  const lld_track::RelocProjSlot S = A.slots[blockIdx.y];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S.n || *S.run == 0) return;
  ProjGenArgs F;
  F.V = *S.view; F.n = S.n; F.routine = LLD_ORB_PROJ_RELOC;
  F.pos = S.pos; F.nrm = nullptr; F.maxd = S.maxd; F.mind = S.mind; F.skip = S.skip; F.angle = S.angle;
  F.th = A.th; F.q = static_cast<QRec*>(S.qrec); F.uv = nullptr; F.level = nullptr;
  project_general_one(F, A.scale, i);
}

constexpr size_t kLdsLimit = 160 * 1024 - 512;
constexpr int kRowBuckets = 512;           // ROWS mode: one bucket per (octave, image row); rows beyond are clamped into the last bucket of the octave

size_t lds_bytes(int nt, int n_cells, bool grid, bool desc) {
  return (size_t)nt * sizeof(TKey) + (desc ? (size_t)nt * 32 : 0) + (size_t)nt * 4 + (size_t)(n_cells + 1) * 4 + 32 * 4 + 8 * 4 + kThreads * 4 +
         48 * 4 + (size_t)nt * 4 + 64 * 8 * 8 + 32;
}

int validate(const lld_orb_search* s, const lld_orb_search_result* out) {
  if (!s || !out) return LLD_ERR_INVALID;
  const int nt = s->nt, nq = s->nq;
  if (nt < 0 || nq < 0) return LLD_ERR_INVALID;
  if (nt > LLD_ORB_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  if (!out->match || !out->best_dist || !out->second_dist || !out->removed) return LLD_ERR_INVALID;
  if (nq > 0 && !s->q_desc) return LLD_ERR_INVALID;
  if (nt > 0 && (!s->t_desc || !s->t_xy || !s->t_octave)) return LLD_ERR_INVALID;
  if (s->candidates < LLD_ORB_CAND_ALL || s->candidates > LLD_ORB_CAND_ROWS) return LLD_ERR_INVALID;
  if (s->ratio_mode < 0 || s->ratio_mode > 2) return LLD_ERR_INVALID;
  if (s->sequential < 0 || s->sequential > 2) return LLD_ERR_INVALID;
  if (s->sequential == 2 && (s->tie_last || s->ratio_mode == 2 || (s->candidates != LLD_ORB_CAND_GRID && s->candidates != LLD_ORB_CAND_ALL))) return LLD_ERR_INVALID;
  const bool grid = s->candidates == LLD_ORB_CAND_GRID;
  if (grid && (!s->q_uv || !s->q_radius || s->grid_cols <= 0 || s->grid_rows <= 0 || s->grid_cols * s->grid_rows > 8191)) return LLD_ERR_INVALID;
  if (s->candidates == LLD_ORB_CAND_CSR && (!s->cand_range || s->n_cand < 0 || (s->n_cand > 0 && !s->cand_idx))) return LLD_ERR_INVALID;
  if (s->candidates == LLD_ORB_CAND_ROWS && (!s->q_uv || !s->level_scale)) return LLD_ERR_INVALID;
  if ((s->gates & LLD_ORB_GATE_LEVEL) && (!s->q_level_min || !s->q_level_max)) return LLD_ERR_INVALID;
  if ((s->gates & LLD_ORB_GATE_STEREO) && (!s->q_uright || !s->q_stereo_radius)) return LLD_ERR_INVALID;
  if ((s->gates & LLD_ORB_GATE_CHI2) && (!s->q_uv || !s->q_uright || !s->level_inv_sigma2)) return LLD_ERR_INVALID;
  if ((s->gates & LLD_ORB_GATE_EPIPOLAR) && (!s->q_epiline || !s->q_stereo || !s->level_scale || !s->level_sigma2)) return LLD_ERR_INVALID;
  if (s->check_orientation && (!s->q_angle || (nt > 0 && !s->t_angle))) return LLD_ERR_INVALID;
  if (s->n_levels < 0 || s->n_levels > LLD_ORB_MAX_LEVELS) return LLD_ERR_UNSUPPORTED;
  for (int k = 0; k < nt; k++) if (s->t_octave[k] < 0 || s->t_octave[k] >= LLD_ORB_MAX_LEVELS) return LLD_ERR_INVALID;
  if (s->candidates == LLD_ORB_CAND_CSR) {
    for (int q = 0; q < nq; q++)
      if (s->cand_range[2 * q] < 0 || s->cand_range[2 * q + 1] < s->cand_range[2 * q] || s->cand_range[2 * q + 1] > s->n_cand) return LLD_ERR_INVALID;
    for (int p = 0; p < s->n_cand; p++) if (s->cand_idx[p] < 0 || s->cand_idx[p] >= nt) return LLD_ERR_INVALID;
  }
  return LLD_OK;
}

inline size_t al(size_t b) { return (b + 63) & ~size_t(63); }

using lld_track::FrustumOut;
using lld_track::LastFrameDev;
using lld_track::MapPointsDev;
using lld_track::SearchOut;

// ---------------------------------------------------------------- the launch of orb_search_kernel
// The descriptors join the keypoint records in LDS when everything still fits.
struct LdsPlan { bool desc_in_lds; size_t bytes; };
LdsPlan lds_plan(int nt, int n_cells, bool bucketed) {
  const bool desc = lds_bytes(nt, n_cells, bucketed, true) <= kLdsLimit;
  return {desc, lds_bytes(nt, n_cells, bucketed, desc)};
}

// One workgroup per problem of problems_d[n]; `lds` is the largest LdsPlan::bytes among them.
int launch_search(lld_ctx* ctx, hipStream_t st, const void* problems_d, int n, size_t lds) {
  if (!ctx->orb_lds_raised) { LLD_HIP_TRY(hipFuncSetAttribute((const void*)orb_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLimit)); ctx->orb_lds_raised = true; }
  hipLaunchKernelGGL(orb_search_kernel, dim3(n), dim3(kThreads), lds, st, static_cast<const Problem*>(problems_d));
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

// ---------------------------------------------------------------- the searched frame
// A level table as the kernels index it: the caller's first n_levels entries, 1 above them and for a table that was not given.
void copy_levels(float (&dst)[LLD_ORB_MAX_LEVELS], const float* src, int n_levels) {
  for (int l = 0; l < LLD_ORB_MAX_LEVELS; l++) dst[l] = (src && l < n_levels) ? src[l] : 1.f;
}

// What the entry points that take a frame by its keypoints (and lld_frame_create, which keeps them) refuse.  host_arrays: the keypoint
// arrays of `s` are the caller's and get read; false when they are resident on the device and `s` carries only the constants.
int check_keypoints(const lld_orb_search* s, bool host_arrays, bool need_angle) {
  const int nt = s->nt;
  if (nt < 0) return LLD_ERR_INVALID;
  if (nt > LLD_ORB_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  if (host_arrays && nt > 0 && (!s->t_desc || !s->t_xy || !s->t_octave || (need_angle && !s->t_angle))) return LLD_ERR_INVALID;
  if (!s->level_scale || s->n_levels <= 0 || s->n_levels > LLD_ORB_MAX_LEVELS) return LLD_ERR_INVALID;
  if (s->grid_cols <= 0 || s->grid_rows <= 0 || s->grid_cols * s->grid_rows > 8191) return LLD_ERR_INVALID;
  if (host_arrays) for (int k = 0; k < nt; k++) if (s->t_octave[k] < 0 || s->t_octave[k] >= LLD_ORB_MAX_LEVELS) return LLD_ERR_INVALID;
  return LLD_OK;
}

using lld_track::KeypointsDev;             // the keypoint side of a search: into the upload region of the call, or into a resident lld_frame
using lld_track::resident_keypoints;

// Where a caller's keypoint arrays travel in an upload region: desc | xy | octave | uright | angle, the last two only when wanted.
struct KeypointsUp {
  size_t desc, xy, octave, uright, angle; bool has_uright, has_angle;
  void reserve(size_t& off, size_t nt, bool with_uright, bool with_angle) {
    auto add = [&](size_t b) { const size_t o = off; off += al(b); return o; };
    has_uright = with_uright; has_angle = with_angle;
    desc = add(nt * 32); xy = add(nt * 8); octave = add(nt * 4); uright = has_uright ? add(nt * 4) : 0; angle = has_angle ? add(nt * 4) : 0;
  }
  void stage(char* h, const lld_orb_search& s) const {
    const size_t nt = s.nt;
    if (!nt) return;
    std::memcpy(h + desc, s.t_desc, nt * 32); std::memcpy(h + xy, s.t_xy, nt * 8); std::memcpy(h + octave, s.t_octave, nt * 4);
    if (has_uright) std::memcpy(h + uright, s.t_uright, nt * 4);
    if (has_angle) std::memcpy(h + angle, s.t_angle, nt * 4);
  }
  KeypointsDev dev(const char* d, int nt) const {
    return {nt, reinterpret_cast<const uint32_t*>(d + desc), reinterpret_cast<const float*>(d + xy), reinterpret_cast<const int32_t*>(d + octave),
            has_uright ? reinterpret_cast<const float*>(d + uright) : nullptr, has_angle ? reinterpret_cast<const float*>(d + angle) : nullptr};
  }
};

// Everything of a Problem that describes the searched frame: its keypoints, its cols x rows buckets with the grid constants of `s`, its level tables.
void set_frame(Problem& P, const KeypointsDev& K, const lld_orb_search& s, int cols, int rows, const float* sigma2, const float* inv_sigma2) {
  P.nt = K.nt; P.t_desc = K.desc; P.t_xy = K.xy; P.t_octave = K.octave; P.t_uright = K.uright; P.t_angle = K.angle;
  P.min_x = s.grid_min_x; P.min_y = s.grid_min_y; P.winv = s.grid_width_inv; P.hinv = s.grid_height_inv;
  P.cols = cols; P.rows = rows; P.n_levels = s.n_levels;
  copy_levels(P.scale, s.level_scale, s.n_levels); copy_levels(P.sigma2, sigma2, s.n_levels); copy_levels(P.inv_sigma2, inv_sigma2, s.n_levels);
}

// ---------------------------------------------------------------- the results
void set_outputs(Problem& P, const SearchOut& o, bool want_owner, void* cache, bool desc_in_lds) {
  P.match = o.match; P.best_dist = o.best_dist; P.second_dist = o.second_dist; P.removed = o.removed; P.owner = o.owner; P.summary = o.summary;
  P.want_owner = want_owner; P.cache = static_cast<unsigned long long*>(cache); P.desc_in_lds = desc_in_lds;
}

// The block match | best_dist | second_dist | owner | summary | removed of one (nq, nt) search, laid out alike in pinned host memory and in HBM.
struct ResultRegion {
  size_t nq, nt, match, bd, sd, owner, sum, rem;
  void reserve(size_t& off, size_t nq_, size_t nt_) {
    auto add = [&](size_t b) { const size_t o = off; off += al(b); return o; };
    nq = nq_; nt = nt_;
    match = add(nq * 4); bd = add(nq * 4); sd = add(nq * 4); owner = add(nt * 4); sum = add(16); rem = add(nq);
  }
  SearchOut dev(char* d_out) const {
    return {reinterpret_cast<int32_t*>(d_out + match), reinterpret_cast<int32_t*>(d_out + bd), reinterpret_cast<int32_t*>(d_out + sd),
            reinterpret_cast<uint8_t*>(d_out + rem), reinterpret_cast<int32_t*>(d_out + owner), reinterpret_cast<int32_t*>(d_out + sum)};
  }
  void fetch(const char* h_out, lld_orb_search_result& o) const {
    if (nq) {
      std::memcpy(o.match, h_out + match, nq * 4); std::memcpy(o.best_dist, h_out + bd, nq * 4);
      std::memcpy(o.second_dist, h_out + sd, nq * 4); std::memcpy(o.removed, h_out + rem, nq);
    }
    if (o.owner && nt) std::memcpy(o.owner, h_out + owner, nt * 4);
    const int32_t* s = reinterpret_cast<const int32_t*>(h_out + sum);
    o.n_matches = s[0]; o.rounds = s[1];
  }
};

// Byte layout of one problem of a batch inside the packed input / output regions.
struct Layout { size_t q, q_desc, t_occ, cand; KeypointsUp kp; ResultRegion res; };

}  // namespace

extern "C" int lld_orb_search_batch(lld_ctx* ctx, int n, const lld_orb_search* problems, lld_orb_search_result* outs) {
  if (!ctx || n < 0 || (n > 0 && (!problems || !outs))) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) { const int st = validate(&problems[i], &outs[i]); if (st) return st; }
  if (n == 0) return LLD_OK;
  LLD_HIP_TRY(hipSetDevice(ctx->device));

  // ---- lay the batch out: [Problem x n | per-problem inputs ...] and [per-problem outputs ...]
  std::vector<Layout> lay((size_t)n);
  size_t in_off = al(sizeof(Problem) * (size_t)n), out_off = 0, lds_max = 0;
  auto add_in = [&](size_t b) { const size_t o = in_off; in_off += al(b); return o; };
  for (int i = 0; i < n; i++) {
    const lld_orb_search& s = problems[i]; Layout& L = lay[i];
    const size_t nt = s.nt, nq = s.nq;
    L.q = add_in(nq * sizeof(QRec)); L.q_desc = add_in(nq * 32);
    L.kp.reserve(in_off, nt, s.t_uright != nullptr, s.t_angle != nullptr);
    L.t_occ = add_in(s.t_occupied ? nt : 0);
    L.cand = add_in(s.candidates == LLD_ORB_CAND_CSR ? (size_t)s.n_cand * 4 : 0);
    L.res.reserve(out_off, nq, nt);
  }
  const size_t in_bytes = in_off, out_bytes = out_off;
  // device-only scratch behind the output region: the round-1 candidate cache of the sequential problems
  std::vector<size_t> cache_at((size_t)n);
  size_t cache_bytes = 0;
  for (int i = 0; i < n; i++) { cache_at[i] = cache_bytes; if (problems[i].sequential) cache_bytes += al((size_t)problems[i].nq * 8 * kTopK); }
  void* hbase; int st = lld_ctx_pinned(ctx, in_bytes + out_bytes, &hbase); if (st) return st;
  void* dbase; st = lld_ctx_scratch(ctx, in_bytes + out_bytes + cache_bytes + 256, &dbase); if (st) return st;
  char* h = (char*)hbase; char* d = (char*)dbase;
  char* d_out = d + in_bytes; char* h_out = h + in_bytes;
  char* d_cache = d_out + out_bytes;

  for (int i = 0; i < n; i++) {
    const lld_orb_search& s = problems[i]; const Layout& L = lay[i];
    const int nt = s.nt, nq = s.nq;
    const bool grid = s.candidates == LLD_ORB_CAND_GRID, by_rows = s.candidates == LLD_ORB_CAND_ROWS;
    QRec* qr = reinterpret_cast<QRec*>(h + L.q);
    for (int q = 0; q < nq; q++) {
      QRec& Q = qr[q]; std::memset(&Q, 0, sizeof(Q));
      if (s.q_uv) { Q.u = s.q_uv[2 * q]; Q.v = s.q_uv[2 * q + 1]; }
      if (s.q_radius) Q.radius = s.q_radius[q];
      if (s.q_uright) Q.ur = s.q_uright[q];
      if (s.q_stereo_radius) Q.stereo_radius = s.q_stereo_radius[q];
      if (s.q_angle) Q.angle = s.q_angle[q];
      if (s.q_epiline) { Q.ea = s.q_epiline[3 * q]; Q.eb = s.q_epiline[3 * q + 1]; Q.ec = s.q_epiline[3 * q + 2]; }
      Q.level_min = s.q_level_min ? s.q_level_min[q] : -1;
      Q.level_max = s.q_level_max ? s.q_level_max[q] : -1;
      Q.flags = ((!s.q_valid || s.q_valid[q]) ? 1 : 0) | ((!s.q_blocks || s.q_blocks[q]) ? 2 : 0) | ((s.q_stereo && s.q_stereo[q]) ? 4 : 0);
      if (s.candidates == LLD_ORB_CAND_CSR) { Q.cs = s.cand_range[2 * q]; Q.ce = s.cand_range[2 * q + 1]; }
    }
    if (nq) std::memcpy(h + L.q_desc, s.q_desc, (size_t)nq * 32);
    L.kp.stage(h, s);
    if (nt && s.t_occupied) std::memcpy(h + L.t_occ, s.t_occupied, (size_t)nt);
    if (s.candidates == LLD_ORB_CAND_CSR && s.n_cand) std::memcpy(h + L.cand, s.cand_idx, (size_t)s.n_cand * 4);

    Problem& P = reinterpret_cast<Problem*>(h)[i]; std::memset(&P, 0, sizeof(P));
    P.nq = nq;
    // the buckets of the counting sort: the caller's grid, or one per (octave, image row), or a single one
    const int n_lv = std::max(1, s.n_levels);
    const int cols = grid ? s.grid_cols : (by_rows ? n_lv : 1), rows = grid ? s.grid_rows : (by_rows ? std::min(kRowBuckets, 8190 / n_lv) : 1);
    set_frame(P, L.kp.dev(d, nt), s, cols, rows, s.level_sigma2, s.level_inv_sigma2);
    P.t_occupied = s.t_occupied ? reinterpret_cast<const uint8_t*>(d + L.t_occ) : nullptr;
    P.q_desc = reinterpret_cast<const uint32_t*>(d + L.q_desc); P.q = reinterpret_cast<const QRec*>(d + L.q);
    P.cand_idx = reinterpret_cast<const int32_t*>(d + L.cand);
    P.disp_min = s.disp_min; P.disp_max = s.disp_max; P.epi_x = s.epipole_x; P.epi_y = s.epipole_y; P.only_stereo = s.only_stereo; P.image_rows = s.image_rows;
    P.candidates = s.candidates; P.gates = s.gates; P.tie_last = s.tie_last; P.accept_max = s.accept_max; P.ratio_mode = s.ratio_mode;
    P.nnratio = s.nnratio; P.sequential = s.sequential; P.check_orientation = s.check_orientation;
    const LdsPlan lds = lds_plan(nt, cols * rows, grid || by_rows);
    set_outputs(P, L.res.dev(d_out), outs[i].owner != nullptr, d_cache + cache_at[i], lds.desc_in_lds);
    lds_max = std::max(lds_max, lds.bytes);
  }

  hipStream_t sm = ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, sm));
  st = launch_search(ctx, sm, d, n, lds_max); if (st) return st;
  LLD_HIP_TRY(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  for (int i = 0; i < n; i++) lay[i].res.fetch(h_out, outs[i]);
  return LLD_OK;
}

extern "C" int lld_orb_search_run(lld_ctx* ctx, const lld_orb_search* s, lld_orb_search_result* out) {
  return lld_orb_search_batch(ctx, 1, s, out);
}

namespace {

// Shared plumbing of the "project on the device, then search" entry points: one packed input region
// [Problem | QRec[nq] (written by the projection kernel) | q_desc | frame keypoints | caller inputs] and one output region.
struct ProjSearch {
  lld_ctx* ctx; const lld_orb_search* frame; int nt, nq; bool need_angle;
  const lld_frame* resident = nullptr;     // the keypoint side is already on the device (lld_frame_*): only t_occupied travels
  size_t in = 0, out = 0, o_q = 0, o_qd = 0, o_tocc = 0;
  KeypointsUp kp{}; ResultRegion res{}; LdsPlan lds{};
  char *h = nullptr, *d = nullptr, *h_out = nullptr, *d_out = nullptr;
  size_t add_in(size_t bytes) { const size_t o = in; in += al(bytes); return o; }
  size_t add_out(size_t bytes) { const size_t o = out; out += al(bytes); return o; }

  int check(const lld_orb_search_result* r) const {
    if (nq < 0) return LLD_ERR_INVALID;
    const int st = check_keypoints(frame, !resident, need_angle); if (st) return st;
    if (!r->match || !r->best_dist || !r->second_dist || !r->removed) return LLD_ERR_INVALID;
    if (resident && need_angle && nt > 0 && !resident->has_angle) return LLD_ERR_INVALID;
    return LLD_OK;
  }
  void layout() {
    in = al(sizeof(Problem));
    o_q = add_in((size_t)nq * sizeof(QRec)); o_qd = add_in((size_t)nq * 32);
    if (!resident) kp.reserve(in, (size_t)nt, frame->t_uright != nullptr, need_angle);
    o_tocc = frame->t_occupied ? add_in((size_t)nt) : 0;
    res.reserve(out, (size_t)nq, (size_t)nt);
  }
  int alloc() {
    void* hb; int st = lld_ctx_pinned(ctx, in + out, &hb); if (st) return st;
    void* db; st = lld_ctx_scratch(ctx, in + out + al((size_t)nq * 8 * kTopK) + 256, &db); if (st) return st;   // + the round-1 candidate cache
    h = (char*)hb; d = (char*)db; h_out = h + in; d_out = d + in;
    return LLD_OK;
  }
  // frame keypoints + query descriptors into the staging buffer, Problem with everything but the matching rules
  Problem& pack(const uint32_t* q_desc, bool want_owner) {
    if (nq) std::memcpy(h + o_qd, q_desc, (size_t)nq * 32);
    if (!resident) kp.stage(h, *frame);
    if (nt && frame->t_occupied) std::memcpy(h + o_tocc, frame->t_occupied, (size_t)nt);
    Problem& P = *reinterpret_cast<Problem*>(h); std::memset(&P, 0, sizeof(P));
    P.nq = nq;
    set_frame(P, resident ? resident_keypoints(resident, need_angle) : kp.dev(d, nt), *frame, frame->grid_cols, frame->grid_rows, nullptr, nullptr);
    P.t_occupied = frame->t_occupied ? reinterpret_cast<const uint8_t*>(d + o_tocc) : nullptr;
    P.q_desc = reinterpret_cast<const uint32_t*>(d + o_qd); P.q = reinterpret_cast<const QRec*>(d + o_q);
    P.candidates = LLD_ORB_CAND_GRID;
    lds = lds_plan(nt, P.cols * P.rows, true);
    set_outputs(P, res.dev(d_out), want_owner, d_out + out, lds.desc_in_lds);
    return P;
  }
  int upload() { LLD_HIP_TRY(hipMemcpyAsync(d, h, in, hipMemcpyHostToDevice, ctx->stream)); return LLD_OK; }
  int search_and_fetch(lld_orb_search_result* r) {
    const int st = launch_search(ctx, ctx->stream, d, 1, lds.bytes); if (st) return st;
    LLD_HIP_TRY(hipMemcpyAsync(h_out, d_out, out, hipMemcpyDeviceToHost, ctx->stream));
    LLD_HIP_TRY(hipStreamSynchronize(ctx->stream));
    res.fetch(h_out, *r);
    return LLD_OK;
  }
};

// A caller's lld_map_points in the upload region of a ProjSearch: pos | normal | max_distance | min_distance | has_obs | skip.  The normals
// and has_obs travel only for a routine that reads them, skip whenever the caller gave it.
struct MapPointsUp {
  size_t pos, nrm, maxd, mind, obs, skip; bool has_nrm, has_obs, has_skip;
  void reserve(ProjSearch& S, const lld_map_points* mp, bool with_normal, bool with_obs) {
    const size_t n = S.nq;
    has_nrm = with_normal; has_obs = with_obs && mp->has_obs; has_skip = mp->skip != nullptr;
    pos = S.add_in(n * 12); nrm = has_nrm ? S.add_in(n * 12) : 0; maxd = S.add_in(n * 4); mind = S.add_in(n * 4);
    obs = has_obs ? S.add_in(n) : 0; skip = has_skip ? S.add_in(n) : 0;
  }
  MapPointsDev stage(const ProjSearch& S, const lld_map_points* mp) const {
    const size_t n = S.nq;
    if (n) {
      std::memcpy(S.h + pos, mp->world_pos, n * 12);
      if (has_nrm) std::memcpy(S.h + nrm, mp->normal, n * 12);
      std::memcpy(S.h + maxd, mp->max_distance, n * 4); std::memcpy(S.h + mind, mp->min_distance, n * 4);
      if (has_obs) std::memcpy(S.h + obs, mp->has_obs, n);
      if (has_skip) std::memcpy(S.h + skip, mp->skip, n);
    }
    return {S.nq, reinterpret_cast<const float*>(S.d + pos), has_nrm ? reinterpret_cast<const float*>(S.d + nrm) : nullptr,
            reinterpret_cast<const float*>(S.d + maxd), reinterpret_cast<const float*>(S.d + mind),
            has_obs ? reinterpret_cast<const uint8_t*>(S.d + obs) : nullptr, has_skip ? reinterpret_cast<const uint8_t*>(S.d + skip) : nullptr};
  }
};

}  // namespace

static int local_points_impl(lld_ctx* ctx, const lld_orb_search* frame, const lld_frame* resident, const lld_frame_view* view, const lld_map_points* mp,
                             float viewing_cos_limit, float th, float nnratio, lld_frustum_result* fr, lld_orb_search_result* out) {
  if (!ctx || !frame || !view || !mp || !out) return LLD_ERR_INVALID;
  ProjSearch S{ctx, frame, frame->nt, mp->n, false, resident};
  int st = S.check(out); if (st) return st;
  const int nq = S.nq;
  if (nq > 0 && (!mp->world_pos || !mp->normal || !mp->max_distance || !mp->min_distance || !mp->desc)) return LLD_ERR_INVALID;
  if (view->n_levels != frame->n_levels) return LLD_ERR_INVALID;
  out->n_matches = 0; out->rounds = 0;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  S.layout();
  MapPointsUp U; U.reserve(S, mp, true, true);
  const size_t r_inv = S.add_out((size_t)nq), r_uvr = S.add_out((size_t)nq * 12), r_lvl = S.add_out((size_t)nq * 4), r_vc = S.add_out((size_t)nq * 4);
  st = S.alloc(); if (st) return st;
  const MapPointsDev M = U.stage(S, mp);
  Problem& P = S.pack(mp->desc, out->owner != nullptr);
  P.gates = LLD_ORB_GATE_LEVEL | LLD_ORB_GATE_STEREO; P.accept_max = 100;       // TH_HIGH, src/ORBmatcher.cc:37,117
  P.ratio_mode = 2; P.nnratio = nnratio; P.sequential = 1;
  st = S.upload(); if (st) return st;
  st = lld_track::orbs_project_local_points(ctx->stream, *frame, view, nullptr, M, viewing_cos_limit, th, S.d + S.o_q,
                                            FrustumOut{reinterpret_cast<uint8_t*>(S.d_out + r_inv), reinterpret_cast<float*>(S.d_out + r_uvr),
                                                       reinterpret_cast<int32_t*>(S.d_out + r_lvl), reinterpret_cast<float*>(S.d_out + r_vc), nullptr});
  if (st) return st;
  st = S.search_and_fetch(out); if (st) return st;
  if (nq && fr) {
    if (fr->in_view) std::memcpy(fr->in_view, S.h_out + r_inv, (size_t)nq);
    if (fr->proj_uvr) std::memcpy(fr->proj_uvr, S.h_out + r_uvr, (size_t)nq * 12);
    if (fr->level) std::memcpy(fr->level, S.h_out + r_lvl, (size_t)nq * 4);
    if (fr->view_cos) std::memcpy(fr->view_cos, S.h_out + r_vc, (size_t)nq * 4);
  }
  return LLD_OK;
}

extern "C" int lld_orb_search_local_points(lld_ctx* ctx, const lld_orb_search* frame, const lld_frame_view* view, const lld_map_points* mp,
                                           float viewing_cos_limit, float th, float nnratio, lld_frustum_result* fr, lld_orb_search_result* out) {
  return local_points_impl(ctx, frame, nullptr, view, mp, viewing_cos_limit, th, nnratio, fr, out);
}

static int last_frame_impl(lld_ctx* ctx, const lld_orb_search* frame, const lld_frame* resident, const lld_frame_view* view, const lld_last_frame_points* last,
                           int direction, float th, int check_orientation, float* proj_uvr, lld_orb_search_result* out) {
  if (!ctx || !frame || !view || !last || !out) return LLD_ERR_INVALID;
  ProjSearch S{ctx, frame, frame->nt, last->n, check_orientation != 0, resident};
  int st = S.check(out); if (st) return st;
  const int nq = S.nq;
  if (nq > 0 && (!last->world_pos || !last->valid || !last->octave || !last->desc || (check_orientation && !last->angle))) return LLD_ERR_INVALID;
  if (view->n_levels != frame->n_levels) return LLD_ERR_INVALID;                // (as the other projecting searches and lld_frame_track_motion_model)
  for (int i = 0; i < nq; i++) if (last->octave[i] < 0 || last->octave[i] >= frame->n_levels) return LLD_ERR_INVALID;
  out->n_matches = 0; out->rounds = 0;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  S.layout();
  const size_t o_pos = S.add_in((size_t)nq * 12), o_val = S.add_in((size_t)nq), o_oct = S.add_in((size_t)nq * 4);
  const size_t o_ang = last->angle ? S.add_in((size_t)nq * 4) : 0, o_obs = last->has_obs ? S.add_in((size_t)nq) : 0;
  const size_t r_uvr = S.add_out((size_t)nq * 12);
  st = S.alloc(); if (st) return st;
  if (nq) {
    std::memcpy(S.h + o_pos, last->world_pos, (size_t)nq * 12); std::memcpy(S.h + o_val, last->valid, (size_t)nq);
    std::memcpy(S.h + o_oct, last->octave, (size_t)nq * 4);
    if (last->angle) std::memcpy(S.h + o_ang, last->angle, (size_t)nq * 4);
    if (last->has_obs) std::memcpy(S.h + o_obs, last->has_obs, (size_t)nq);
  }
  const LastFrameDev L{nq, reinterpret_cast<const float*>(S.d + o_pos), reinterpret_cast<const uint8_t*>(S.d + o_val), reinterpret_cast<const int32_t*>(S.d + o_oct),
                       last->angle ? reinterpret_cast<const float*>(S.d + o_ang) : nullptr, last->has_obs ? reinterpret_cast<const uint8_t*>(S.d + o_obs) : nullptr};
  Problem& P = S.pack(last->desc, out->owner != nullptr);
  P.gates = LLD_ORB_GATE_LEVEL | LLD_ORB_GATE_STEREO; P.accept_max = 100;       // TH_HIGH, src/ORBmatcher.cc:1418
  P.ratio_mode = 0; P.sequential = 1; P.check_orientation = check_orientation != 0;
  st = S.upload(); if (st) return st;
  st = lld_track::orbs_project_last_frame(ctx->stream, *frame, view, nullptr, L, direction, th, S.d + S.o_q, reinterpret_cast<float*>(S.d_out + r_uvr), lld_track::RunIf{});
  if (st) return st;
  st = S.search_and_fetch(out); if (st) return st;
  if (nq && proj_uvr) std::memcpy(proj_uvr, S.h_out + r_uvr, (size_t)nq * 12);
  return LLD_OK;
}

extern "C" int lld_orb_search_last_frame(lld_ctx* ctx, const lld_orb_search* frame, const lld_frame_view* view, const lld_last_frame_points* last,
                                         int direction, float th, int check_orientation, float* proj_uvr, lld_orb_search_result* out) {
  return last_frame_impl(ctx, frame, nullptr, view, last, direction, th, check_orientation, proj_uvr, out);
}

// ---- the resident frame (lld_frame_*)
extern "C" int lld_frame_create(lld_ctx* ctx, const lld_orb_search* kp, lld_frame** out) {
  if (!ctx || !kp || !out) return LLD_ERR_INVALID;
  *out = nullptr;
  int st = check_keypoints(kp, true, false); if (st) return st;
  const int nt = kp->nt;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  lld_frame* f = new lld_frame();
  f->ctx = ctx; f->nt = nt; f->has_uright = kp->t_uright != nullptr; f->has_angle = kp->t_angle != nullptr; f->has_inv_sigma2 = kp->level_inv_sigma2 != nullptr;
  f->consts = *kp;
  f->consts.t_desc = nullptr; f->consts.t_xy = nullptr; f->consts.t_octave = nullptr; f->consts.t_uright = nullptr; f->consts.t_angle = nullptr; f->consts.t_occupied = nullptr;
  f->consts.nq = 0; f->consts.q_desc = nullptr;
  copy_levels(f->scale, kp->level_scale, kp->n_levels); copy_levels(f->sigma2, kp->level_sigma2, kp->n_levels); copy_levels(f->inv_sigma2, kp->level_inv_sigma2, kp->n_levels);
  f->consts.level_scale = f->scale; f->consts.level_sigma2 = f->sigma2; f->consts.level_inv_sigma2 = f->inv_sigma2;
  size_t bytes = 0;
  KeypointsUp U; U.reserve(bytes, (size_t)nt, f->has_uright, f->has_angle);
  f->o_td = U.desc; f->o_txy = U.xy; f->o_toct = U.octave; f->o_tur = U.uright; f->o_tang = U.angle;
  if (hipMalloc(reinterpret_cast<void**>(&f->d), bytes + 256) != hipSuccess) { delete f; return LLD_ERR_ALLOC; }
  void* hb = nullptr;
  st = lld_ctx_pinned(ctx, bytes + 256, &hb);
  if (st) { (void)hipFree(f->d); delete f; return st; }
  char* h = static_cast<char*>(hb);
  U.stage(h, *kp);
  // (the context's pinned staging is reused by the next call on this context: the copy must have left it before this one returns)
  if (hipMemcpyAsync(f->d, h, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { (void)hipFree(f->d); delete f; return LLD_ERR_HIP; }
  *out = f;
  return LLD_OK;
}

extern "C" void lld_frame_destroy(lld_frame* f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  (void)hipStreamSynchronize(f->ctx->stream);
  lld_track::state_free(f);
  if (f->d) (void)hipFree(f->d);
  if (f->h_stage) (void)hipHostFree(f->h_stage);
  if (f->h_lines) {                                                           // (the stream was waited for above: no copy reads it)
    if (f->ctx->line_staging.size() < lld_ctx::kLineStagingKept) f->ctx->line_staging.emplace_back(f->h_lines, f->h_lines_bytes);
    else (void)hipHostFree(f->h_lines);
  }
  if (f->d_bow) (void)hipFree(f->d_bow);
  delete f;
}

extern "C" int lld_frame_search_last_frame(lld_frame* f, const uint8_t* t_occupied, const lld_frame_view* view, const lld_last_frame_points* last,
                                           int direction, float th, int check_orientation, float* proj_uvr, lld_orb_search_result* out) {
  if (!f) return LLD_ERR_INVALID;
  lld_orb_search fs = f->consts; fs.nt = f->nt; fs.t_occupied = t_occupied;
  return last_frame_impl(f->ctx, &fs, f, view, last, direction, th, check_orientation, proj_uvr, out);
}

extern "C" int lld_frame_search_local_points(lld_frame* f, const uint8_t* t_occupied, const lld_frame_view* view, const lld_map_points* mp,
                                             float viewing_cos_limit, float th, float nnratio, lld_frustum_result* fr, lld_orb_search_result* out) {
  if (!f) return LLD_ERR_INVALID;
  lld_orb_search fs = f->consts; fs.nt = f->nt; fs.t_occupied = t_occupied;
  return local_points_impl(f->ctx, &fs, f, view, mp, viewing_cos_limit, th, nnratio, fr, out);
}

extern "C" int lld_orb_fuse_search(lld_ctx* ctx, const lld_orb_search* keyframe, const lld_frame_view* view, const lld_map_points* mp, float th,
                                   float* proj_uvr, lld_orb_search_result* out) {
  if (!ctx || !keyframe || !view || !mp || !out) return LLD_ERR_INVALID;
  ProjSearch S{ctx, keyframe, keyframe->nt, mp->n, false};
  int st = S.check(out); if (st) return st;
  const int nq = S.nq;
  if (nq > 0 && (!mp->world_pos || !mp->normal || !mp->max_distance || !mp->min_distance || !mp->desc)) return LLD_ERR_INVALID;
  if (view->n_levels != keyframe->n_levels || !keyframe->level_inv_sigma2) return LLD_ERR_INVALID;
  out->n_matches = 0; out->rounds = 0;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  S.layout();
  MapPointsUp U; U.reserve(S, mp, true, false);
  const size_t r_uvr = S.add_out((size_t)nq * 12);
  st = S.alloc(); if (st) return st;
  const MapPointsDev M = U.stage(S, mp);
  Problem& P = S.pack(mp->desc, out->owner != nullptr);
  copy_levels(P.inv_sigma2, keyframe->level_inv_sigma2, keyframe->n_levels);
  P.gates = LLD_ORB_GATE_LEVEL | LLD_ORB_GATE_CHI2; P.accept_max = 50;          // TH_LOW, src/ORBmatcher.cc:38,934
  st = S.upload(); if (st) return st;
  if (nq) {
    FuseArgs F; std::memset(&F, 0, sizeof(F));
    F.V = *view; F.n = nq;
    F.pos = M.pos; F.nrm = M.normal; F.maxd = M.maxd; F.mind = M.mind; F.skip = M.skip;
    copy_levels(F.scale, keyframe->level_scale, keyframe->n_levels);
    F.th = th;
    F.q = reinterpret_cast<QRec*>(S.d + S.o_q); F.uvr = reinterpret_cast<float*>(S.d_out + r_uvr);
    hipLaunchKernelGGL(project_fuse_kernel, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, F);
    LLD_HIP_TRY(hipGetLastError());
  }
  st = S.search_and_fetch(out); if (st) return st;
  if (nq && proj_uvr) std::memcpy(proj_uvr, S.h_out + r_uvr, (size_t)nq * 12);
  return LLD_OK;
}

extern "C" int lld_orb_search_projected(lld_ctx* ctx, const lld_orb_search* frame, const lld_frame_view* view, const lld_map_points* mp,
                                        const float* angle, const lld_orb_projection* proj, float* proj_uv, int32_t* level, lld_orb_search_result* out) {
  if (!ctx || !frame || !view || !mp || !proj || !out) return LLD_ERR_INVALID;
  const int routine = proj->routine;
  if (routine < LLD_ORB_PROJ_KF_SIM3 || routine > LLD_ORB_PROJ_SIM3_DIR) return LLD_ERR_INVALID;
  const bool reloc = routine == LLD_ORB_PROJ_RELOC, orient = reloc && proj->check_orientation != 0;
  const bool need_normal = routine == LLD_ORB_PROJ_KF_SIM3 || routine == LLD_ORB_PROJ_FUSE_SIM3;
  ProjSearch S{ctx, frame, frame->nt, mp->n, orient};
  int st = S.check(out); if (st) return st;
  const int nq = S.nq;
  if (nq > 0 && (!mp->world_pos || !mp->max_distance || !mp->min_distance || !mp->desc || (need_normal && !mp->normal) || (orient && !angle))) return LLD_ERR_INVALID;
  if (view->n_levels != frame->n_levels) return LLD_ERR_INVALID;
  out->n_matches = 0; out->rounds = 0;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  S.layout();
  MapPointsUp U; U.reserve(S, mp, need_normal, false);
  const size_t o_ang = angle ? S.add_in((size_t)nq * 4) : 0;
  const size_t r_uv = S.add_out((size_t)nq * 8), r_lvl = S.add_out((size_t)nq * 4);
  st = S.alloc(); if (st) return st;
  const MapPointsDev M = U.stage(S, mp);
  if (nq && angle) std::memcpy(S.h + o_ang, angle, (size_t)nq * 4);
  Problem& P = S.pack(mp->desc, out->owner != nullptr);
  P.gates = LLD_ORB_GATE_LEVEL;
  switch (routine) {
    case LLD_ORB_PROJ_KF_SIM3: P.accept_max = 50; P.sequential = 1; break;                                   // TH_LOW (:394); vpMatched[bestIdx]=pMP inside the loop
    case LLD_ORB_PROJ_RELOC: P.accept_max = proj->accept_max; P.sequential = 1; P.check_orientation = orient; break;   // ORBdist (:1555)
    case LLD_ORB_PROJ_FUSE_SIM3: P.accept_max = 50; break;                                                   // TH_LOW (:1078)
    default: P.accept_max = 100; break;                                                                      // TH_HIGH (:1220, :1300)
  }
  st = S.upload(); if (st) return st;
  if (nq) {
    ProjGenArgs F; std::memset(&F, 0, sizeof(F));
    F.V = *view; F.n = nq; F.routine = routine;
    for (int k = 0; k < 9; k++) F.sR[k] = proj->sR[k];
    for (int k = 0; k < 3; k++) F.t2[k] = proj->t[k];
    F.pos = M.pos; F.nrm = M.normal; F.maxd = M.maxd; F.mind = M.mind; F.skip = M.skip;
    F.angle = angle ? reinterpret_cast<const float*>(S.d + o_ang) : nullptr;
    copy_levels(F.scale, frame->level_scale, frame->n_levels);
    F.th = proj->th;
    F.q = reinterpret_cast<QRec*>(S.d + S.o_q); F.uv = reinterpret_cast<float*>(S.d_out + r_uv); F.level = reinterpret_cast<int32_t*>(S.d_out + r_lvl);
    hipLaunchKernelGGL(project_general_kernel, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, F);
    LLD_HIP_TRY(hipGetLastError());
  }
  st = S.search_and_fetch(out); if (st) return st;
  if (nq && proj_uv) std::memcpy(proj_uv, S.h_out + r_uv, (size_t)nq * 8);
  if (nq && level) std::memcpy(level, S.h_out + r_lvl, (size_t)nq * 4);
  return LLD_OK;
}

extern "C" int lld_orb_search_by_sim3(lld_ctx* ctx, const lld_orb_search* kf1, const lld_frame_view* view1, const lld_map_points* points1,
                                      const lld_orb_search* kf2, const lld_frame_view* view2, const lld_map_points* points2,
                                      const float* sR12, const float* t12, const float* sR21, const float* t21, float th, int32_t* match12, int32_t* n_found) {
  if (!ctx || !kf1 || !kf2 || !view1 || !view2 || !points1 || !points2 || !sR12 || !t12 || !sR21 || !t21 || !match12 || !n_found) return LLD_ERR_INVALID;
  const int n1 = points1->n, n2 = points2->n;
  if (n1 != kf1->nt || n2 != kf2->nt) return LLD_ERR_INVALID;                   // vpMapPoints1 / 2 are per keypoint of their keyframe
  std::vector<int32_t> m1((size_t)std::max(n1, 1)), m2((size_t)std::max(n2, 1)), bd((size_t)std::max(std::max(n1, n2), 1)), sd(bd.size());
  std::vector<uint8_t> rem(bd.size());
  lld_orb_projection pr; std::memset(&pr, 0, sizeof pr);
  pr.routine = LLD_ORB_PROJ_SIM3_DIR; pr.th = th;
  // KF1's MapPoints into KF2 (:1147-1224): camera 1 from world, then sR21 / t21; searched among KF2's keypoints
  for (int k = 0; k < 9; k++) pr.sR[k] = sR21[k];
  for (int k = 0; k < 3; k++) pr.t[k] = t21[k];
  // pose R1w, t1w; fx, fy, cx, cy are pKF1's in BOTH directions (:1105-1108); IsInImage and PredictScale are pKF2's (:1176, :1188)
  lld_frame_view v = *view1;
  v.min_x = view2->min_x; v.max_x = view2->max_x; v.min_y = view2->min_y; v.max_y = view2->max_y;
  v.log_scale_factor = view2->log_scale_factor; v.n_levels = view2->n_levels;
  lld_orb_search_result r1{m1.data(), bd.data(), sd.data(), rem.data(), nullptr, 0, 0};
  int st = lld_orb_search_projected(ctx, kf2, &v, points1, nullptr, &pr, nullptr, nullptr, &r1); if (st) return st;
  // KF2's MapPoints into KF1 (:1227-1304)
  for (int k = 0; k < 9; k++) pr.sR[k] = sR12[k];
  for (int k = 0; k < 3; k++) pr.t[k] = t12[k];
  v = *view2;                                                                   // pose R2w, t2w; pKF1's intrinsics, bounds and scale pyramid (:1256, :1268)
  v.fx = view1->fx; v.fy = view1->fy; v.cx = view1->cx; v.cy = view1->cy; v.min_x = view1->min_x; v.max_x = view1->max_x; v.min_y = view1->min_y; v.max_y = view1->max_y;
  v.log_scale_factor = view1->log_scale_factor; v.n_levels = view1->n_levels;
  lld_orb_search_result r2{m2.data(), bd.data(), sd.data(), rem.data(), nullptr, 0, 0};
  st = lld_orb_search_projected(ctx, kf1, &v, points2, nullptr, &pr, nullptr, nullptr, &r2); if (st) return st;
  // agreement (:1306-1322)
  int found = 0;
  for (int i1 = 0; i1 < n1; i1++) {
    const int idx2 = m1[i1];
    match12[i1] = -1;
    if (idx2 >= 0 && idx2 < n2 && m2[idx2] == i1) { match12[i1] = idx2; found++; }
  }
  *n_found = found;
  return LLD_OK;
}

// ================================================================ launchers for the device-resident Tracking chain (lld_track_internal.h)
namespace lld_track {

KeypointsDev resident_keypoints(const lld_frame* f, bool want_angle) {
  return {f->nt, reinterpret_cast<const uint32_t*>(f->d + f->o_td), reinterpret_cast<const float*>(f->d + f->o_txy), reinterpret_cast<const int32_t*>(f->d + f->o_toct),
          f->has_uright ? reinterpret_cast<const float*>(f->d + f->o_tur) : nullptr,
          (want_angle && f->has_angle) ? reinterpret_cast<const float*>(f->d + f->o_tang) : nullptr};
}

size_t orbs_problem_bytes() { return sizeof(Problem); }
size_t orbs_qrec_bytes(int nq) { return al((size_t)nq * sizeof(QRec)); }
size_t orbs_cache_bytes(int nq) { return al((size_t)nq * 8 * kTopK); }
void orbs_fill_problem(const lld_frame* f, int mode, int nq, const uint8_t* d_occupied, const void* d_qrec, const uint32_t* d_qdesc, const SearchOut& out,
                       void* d_cache, float nnratio, int check_orientation, RunIf run_if, const ApplyDev& ap, void* problem_h) {
  Problem& P = *static_cast<Problem*>(problem_h); std::memset(&P, 0, sizeof(P));
  const lld_orb_search& c = f->consts;
  P.nq = nq;
  set_frame(P, resident_keypoints(f, check_orientation != 0), c, c.grid_cols, c.grid_rows, nullptr, nullptr);
  P.t_occupied = d_occupied;
  P.q_desc = d_qdesc; P.q = static_cast<const QRec*>(d_qrec);
  P.candidates = LLD_ORB_CAND_GRID;
  P.gates = LLD_ORB_GATE_LEVEL | LLD_ORB_GATE_STEREO; P.accept_max = 100;       // TH_HIGH (src/ORBmatcher.cc:117, :1418)
  if (mode == 0) { P.ratio_mode = 0; P.check_orientation = check_orientation != 0; }
  else { P.ratio_mode = 2; P.nnratio = nnratio; }
  P.sequential = 1;
  set_outputs(P, out, true, d_cache, lds_plan(f->nt, c.grid_cols * c.grid_rows, true).desc_in_lds);
  P.run_if = run_if.flag; P.run_if_below = run_if.below; P.run_if_want = run_if.want;
  P.t_occ_obs = ap.kp_obs;                                                      // (the frame's own flags: only a MapPoint with observations blocks its keypoint)
  P.ap_has = ap.kp_has; P.ap_world = ap.kp_world; P.ap_id = ap.kp_id; P.ap_obs = ap.kp_obs; P.ap_q_pos = ap.q_pos; P.ap_q_id = ap.q_id; P.ap_q_obs = ap.q_obs;
  P.ap_counts = ap.counts; P.ap_min_matches = ap.min_matches; P.ap_is_retry = ap.is_retry;
}

// (The projections keep launches of their own: as a prologue of the search kernel, 2500 frustum tests on ONE compute unit take 38 us where ten
// workgroups of frustum_kernel take 11.)
int orbs_project_last_frame(hipStream_t st, const lld_orb_search& c, const lld_frame_view* view_h, const lld_frame_view* view_d, const LastFrameDev& last, int direction, float th,
                            void* d_qrec, float* d_uvr, RunIf run_if) {
  if (last.n <= 0) return LLD_OK;
  LastFrameArgs F; std::memset(&F, 0, sizeof(F));
  if (view_h) F.V = *view_h;
  F.view_d = view_d; F.n = last.n; F.direction = direction;
  F.pos = last.pos; F.valid = last.valid; F.octave = last.octave; F.angle = last.angle; F.has_obs = last.has_obs;
  copy_levels(F.scale, c.level_scale, c.n_levels);
  F.th = th; F.q = static_cast<QRec*>(d_qrec); F.uvr = d_uvr;
  F.run_if = run_if.flag; F.run_if_below = run_if.below; F.run_if_want = run_if.want;
  hipLaunchKernelGGL(project_last_frame_kernel, dim3((last.n + 255) / 256), dim3(256), 0, st, F);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

int orbs_project_local_points(hipStream_t st, const lld_orb_search& c, const lld_frame_view* view_h, const lld_frame_view* view_d, const MapPointsDev& mp, float cos_limit, float th,
                              void* d_qrec, const FrustumOut& out) {
  if (mp.n <= 0) return LLD_OK;
  FrustumArgs F; std::memset(&F, 0, sizeof(F));
  if (view_h) F.V = *view_h;
  F.view_d = view_d; F.n = mp.n;
  F.pos = mp.pos; F.nrm = mp.normal; F.maxd = mp.maxd; F.mind = mp.mind; F.has_obs = mp.has_obs; F.skip = mp.skip;
  copy_levels(F.scale, c.level_scale, c.n_levels);
  F.cos_limit = cos_limit; F.th = th; F.q = static_cast<QRec*>(d_qrec);
  F.in_view = out.in_view; F.uvr = out.uvr; F.level = out.level; F.view_cos = out.view_cos; F.n_in_view = out.n_in_view;
  hipLaunchKernelGGL(frustum_kernel, dim3((mp.n + 255) / 256), dim3(256), 0, st, F);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

void orbs_fill_problem_reloc(const lld_frame* f, int nq, const uint8_t* d_occupied, const void* d_qrec, const uint32_t* d_qdesc, const SearchOut& out, void* d_cache,
                             int accept_max, RunIf run_if, const ApplyDev& ap, void* problem_h) {
  orbs_fill_problem(f, 0, nq, d_occupied, d_qrec, d_qdesc, out, d_cache, 0.f, 1, run_if, ap, problem_h);
  Problem& P = *static_cast<Problem*>(problem_h);
  P.gates = LLD_ORB_GATE_LEVEL; P.accept_max = accept_max;                      // ORBdist (:1555); no stereo gate in this routine
  P.t_occ_obs = nullptr;                                                        // if(CurrentFrame.mvpMapPoints[i2]) continue;  (:1528)
}

int orbs_project_reloc_slots(hipStream_t st, const lld_frame* f, int n_slots, int n_max, const RelocProjSlot* slots_d, float th) {
  if (n_slots <= 0 || n_max <= 0) return LLD_OK;
  ProjRelocSlotsArgs A; std::memset(&A, 0, sizeof(A));
  A.slots = slots_d; A.th = th;
  copy_levels(A.scale, f->consts.level_scale, f->consts.n_levels);
  hipLaunchKernelGGL(project_reloc_slots_kernel, dim3((n_max + 255) / 256, n_slots), dim3(256), 0, st, A);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

int orbs_launch_n(lld_ctx* ctx, hipStream_t st, const lld_frame* f, const void* problems_d, int n) {
  if (n <= 0) return LLD_OK;
  return launch_search(ctx, st, problems_d, n, lds_plan(f->nt, f->consts.grid_cols * f->consts.grid_rows, true).bytes);
}

}  // namespace lld_track
