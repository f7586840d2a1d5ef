// lld_orb_extract.hip — ORBextractor::operator() (src/ORBextractor.cc:1043-1105) on the device: pyramid, FAST per cell, the octree
// distribution, IC_Angle, the blur and rBRIEF.  The OpenCV parts are restated as include/lld_amd.h defines them; every float
// operation that feeds a result is an explicit round-to-nearest intrinsic, so nothing is contracted into an FMA.
//
// Launch sequence per lld_orb_extract (all on the context's stream, all images in each launch):
//   copy level 0 -> orbx_resize per level 1..L-1 -> orbx_score (FAST score map) + orbx_blur (one launch each, every level)
//   -> orbx_cells (one wavefront per cell: thresholds, NMS, ordered output) -> orbx_octree (one workgroup per (image, level))
//   -> orbx_emit (orientation, descriptor, scaled keypoint) -> one copy of every image's results to the host.
#include "lld_stereo_internal.h"
#include "lld_glibc_sincosf.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kEdge = 19;          // EDGE_THRESHOLD
constexpr int kMinBorder = kEdge - 3;
constexpr int kHalfPatch = 15;
constexpr int kMaxSide = 16383;
constexpr int kOctThreads = 512;

// per (image, level) geometry and buffers, built on the host for each call
struct LevelGeo {
  int cols, rows, step;
  int n_cols, n_rows, w_cell, h_cell;       // FAST cells (:777-784)
  int max_bx, max_by;                       // maxBorderX / maxBorderY
  int n_ini; float hx;                      // DistributeOctTree's initial nodes
  int N;                                    // mnFeaturesPerLevel
  int cell_cap;                             // candidate slots per cell (w_cell * h_cell)
  int key_cap, node_cap, res_cap;
  uint8_t* img; uint8_t* blur; uint8_t* score;
  int32_t* cell_cnt; int32_t* cand_xy; uint8_t* cand_score;
  // octree workspace
  int32_t* kxy; int32_t* kscore; int32_t* knode; int8_t* kq;
  int32_t* nd[2];                           // [node_cap][6]: x0, y0, x1, y1, cnt, flags(1 = bNoMore)
  int32_t* cnt4;                            // [node_cap][4]
  int32_t* childpos;                        // [node_cap][4]
  int32_t* newpos;                          // [node_cap]
  int32_t* order;                           // [node_cap] processing order
  int32_t* vsize[2];                        // [node_cap] children with > 1 keys, push order
  unsigned long long* best;                 // [node_cap]
  int32_t* res;                             // [res_cap][3]: x, y (level pixels), score
  int32_t* stats;                           // [8] lld_orb_level_stats
};

struct GeoTable {
  int n_images, n_levels;
  int min_th, ini_th;
  LevelGeo g[1];                            // [n_images * n_levels] (allocated larger)
};

// OpenCV's cvRound: round half to even
__host__ __device__ inline int cv_round(float x) { return (int)rintf(x); }

// ---------------------------------------------------------------------------------------------------- pyramid

__device__ inline void lin_coef(int d, int ssize, int dsize, int* s0, int* s1, int* c0, int* c1) {
  const double scale = __ddiv_rn(1.0, __ddiv_rn((double)dsize, (double)ssize));
  float f = (float)__dadd_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), -0.5);
  int s = (int)floorf(f);
  f = __fsub_rn(f, (float)s);
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= ssize - 1) { s = ssize - 1; f = 0.f; }
  *s0 = s; *s1 = s + 1 < ssize ? s + 1 : ssize - 1;
  *c1 = cv_round(__fmul_rn(f, 2048.f)); *c0 = 2048 - *c1;
}

__global__ void orbx_resize(const GeoTable* T, int level) {
  const int im = blockIdx.z;
  const LevelGeo& S = T->g[im * T->n_levels + level - 1];
  const LevelGeo& D = T->g[im * T->n_levels + level];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= D.cols || y >= D.rows) return;
  int sx0, sx1, a0, a1, sy0, sy1, b0, b1;
  lin_coef(x, S.cols, D.cols, &sx0, &sx1, &a0, &a1);
  lin_coef(y, S.rows, D.rows, &sy0, &sy1, &b0, &b1);
  const uint8_t* r0 = S.img + (size_t)sy0 * S.step;
  const uint8_t* r1 = S.img + (size_t)sy1 * S.step;
  const int h0 = a0 * r0[sx0] + a1 * r0[sx1], h1 = a0 * r1[sx0] + a1 * r1[sx1];
  D.img[(size_t)y * D.step + x] = (uint8_t)((b0 * h0 + b1 * h1 + (1 << 21)) >> 22);
}

// ---------------------------------------------------------------------------------------------------- FAST score map
__constant__ int kCircle[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3},
                                   {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};

__global__ void orbx_score(const GeoTable* T) {
  const int im = blockIdx.z / T->n_levels, lv = blockIdx.z % T->n_levels;
  const LevelGeo& G = T->g[im * T->n_levels + lv];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= G.cols || y >= G.rows) return;
  int sc = 0;
  if (x >= 3 && y >= 3 && x < G.cols - 3 && y < G.rows - 3) {
    const uint8_t* c = G.img + (size_t)y * G.step + x;
    const int p = c[0];
    int d[16];
#pragma unroll
    for (int k = 0; k < 16; k++) d[k] = (int)c[kCircle[k][1] * G.step + kCircle[k][0]] - p;
    int best_b = -1000, best_d = -1000;
#pragma unroll
    for (int s = 0; s < 16; s++) {
      int mb = 1000, md = 1000;
#pragma unroll
      for (int k = 0; k < 9; k++) { const int v = d[(s + k) & 15]; mb = min(mb, v); md = min(md, -v); }
      best_b = max(best_b, mb); best_d = max(best_d, md);
    }
    sc = max(best_b, best_d) - 1;
    sc = sc < 0 ? 0 : sc;                   // scores below 1 never matter: thresholds are >= 1
  }
  G.score[(size_t)y * G.step + x] = (uint8_t)sc;
}

// ---------------------------------------------------------------------------------------------------- blur
__constant__ int kGauss[7] = {18, 34, 49, 54, 49, 34, 18};

__device__ inline int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ void orbx_blur(const GeoTable* T) {
  const int im = blockIdx.z / T->n_levels, lv = blockIdx.z % T->n_levels;
  const LevelGeo& G = T->g[im * T->n_levels + lv];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= G.cols || y >= G.rows) return;
  int xs[7];
#pragma unroll
  for (int k = 0; k < 7; k++) xs[k] = reflect101(x + k - 3, G.cols);
  int v = 0;
#pragma unroll
  for (int r = 0; r < 7; r++) {
    const uint8_t* row = G.img + (size_t)reflect101(y + r - 3, G.rows) * G.step;
    int h = 0;
#pragma unroll
    for (int k = 0; k < 7; k++) h += kGauss[k] * row[xs[k]];
    v += kGauss[r] * h;
  }
  G.blur[(size_t)y * G.step + x] = (uint8_t)((v + 32768) >> 16);
}

// ---------------------------------------------------------------------------------------------------- FAST per cell
// One wavefront per cell.  Lane = column of the cell's interior (<= wCell <= 59 columns), rows in order, so a ballot gives the
// row-major rank of each kept corner.
__global__ __launch_bounds__(64) void orbx_cells(const GeoTable* T) {
  const int im = blockIdx.z / T->n_levels, lv = blockIdx.z % T->n_levels;
  const LevelGeo& G = T->g[im * T->n_levels + lv];
  const int cell = blockIdx.x;
  if (cell >= G.n_cols * G.n_rows) return;
  const int i = cell / G.n_cols, j = cell % G.n_cols, lane = threadIdx.x;
  const float iniY = (float)(kMinBorder + i * G.h_cell), iniX = (float)(kMinBorder + j * G.w_cell);
  float maxY = iniY + (float)G.h_cell + 6.f, maxX = iniX + (float)G.w_cell + 6.f;
  int n_out = 0;
  if (!(iniY >= (float)(G.max_by - 3)) && !(iniX >= (float)(G.max_bx - 6))) {
    if (maxY > (float)G.max_by) maxY = (float)G.max_by;
    if (maxX > (float)G.max_bx) maxX = (float)G.max_bx;
    const int y0 = (int)iniY, x0 = (int)iniX, h = (int)maxY - y0, w = (int)maxX - x0;
    const int xr = lane + 3;                                   // column inside the sub-image
    int32_t* oxy = G.cand_xy + (size_t)cell * G.cell_cap;
    uint8_t* osc = G.cand_score + (size_t)cell * G.cell_cap;
    for (int pass = 0; pass < 2 && n_out == 0; pass++) {
      const int th = pass == 0 ? T->ini_th : T->min_th;
      for (int yr = 3; yr <= h - 4; yr++) {
        bool keep = false; int s = 0;
        if (xr <= w - 4) {
          const uint8_t* sp = G.score + (size_t)(y0 + yr) * G.step + (x0 + xr);
          s = sp[0];
          if (s >= th) {
            keep = true;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
              for (int dx = -1; dx <= 1; dx++) {
                if (dx == 0 && dy == 0) continue;
                const int nx = xr + dx, ny = yr + dy;
                int ns = 0;
                if (nx >= 3 && nx <= w - 4 && ny >= 3 && ny <= h - 4) { ns = sp[dy * G.step + dx]; if (ns < th) ns = 0; }
                if (!(s > ns)) keep = false;
              }
          }
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
          const int r = n_out + __popcll(m & ((1ull << lane) - 1ull));
          if (r < G.cell_cap) {                                // always true: the interior has <= cell_cap pixels
            oxy[r] = (x0 + xr - kMinBorder) | ((y0 + yr - kMinBorder) << 16);
            osc[r] = (uint8_t)s;
          }
        }
        n_out += __popcll(m);
      }
      if (n_out == 0 && lane == 0) atomicAdd(&G.stats[pass == 0 ? 1 : 2], 1);
    }
  }
  if (lane == 0) G.cell_cnt[cell] = n_out < G.cell_cap ? n_out : G.cell_cap;
}

// ---------------------------------------------------------------------------------------------------- DistributeOctTree
// One workgroup per (image, level).  The list lNodes is held as an array in list order (double-buffered: nd[cur] -> nd[nxt]);
// each key carries the index of its node.  One split step:
//   1. keys of the nodes in `order` (the nodes to split, in processing order) count themselves into their node's 4 quadrants;
//   2. thread 0 walks `order`, accumulating the list size, and stops after the node that makes it >= N when `limited` (sorted
//      phase); it writes the new list: the children of the processed nodes, last processed first and n4..n1 within a node
//      (push_front), then the old nodes not split, in their order; and the children with > 1 keys in push order (vSizeAndPointerToNode);
//   3. keys move to their child's (or their node's) new index.
struct OctShared {
  int size, prev, n_order, n_vs, cur, vs_cur, done, iteration, sorted_rounds, finish_unchanged, n_keys, overflow;
};

__device__ inline void oct_split_step(const LevelGeo& G, OctShared& S, bool limited) {
  const int tid = threadIdx.x, nt = blockDim.x;
  int32_t* nd = G.nd[S.cur];
  int32_t* nx = G.nd[S.cur ^ 1];
  // mark the nodes to split (newpos = -2 - rank), clear their quadrant counters
  for (int k = tid; k < S.size; k += nt) G.newpos[k] = -1;
  __syncthreads();
  for (int r = tid; r < S.n_order; r += nt) {
    const int n = G.order[r];
    G.newpos[n] = -2 - r;
    G.cnt4[4 * n] = G.cnt4[4 * n + 1] = G.cnt4[4 * n + 2] = G.cnt4[4 * n + 3] = 0;
  }
  __syncthreads();
  for (int k = tid; k < S.n_keys; k += nt) {
    const int n = G.knode[k];
    if (G.newpos[n] <= -2) {
      const int* b = nd + 6 * n;
      const int hx = (b[2] - b[0] + 1) >> 1, hy = (b[3] - b[1] + 1) >> 1;   // ceil((float)d / 2) for d >= 0
      const int x = G.kxy[k] & 0xffff, y = G.kxy[k] >> 16;
      const int q = (x < b[0] + hx) ? (y < b[1] + hy ? 0 : 2) : (y < b[1] + hy ? 1 : 3);
      G.kq[k] = (int8_t)q;
      atomicAdd(&G.cnt4[4 * n + q], 1);
    }
  }
  __syncthreads();
  if (tid == 0) {
    int size = S.size, J = 0;
    for (; J < S.n_order; J++) {
      const int n = G.order[J];
      int ne = 0;
      for (int q = 0; q < 4; q++) ne += G.cnt4[4 * n + q] > 0;
      size += ne - 1;
      if (limited && size >= G.N) { J++; break; }
    }
    for (int r = J; r < S.n_order; r++) G.newpos[G.order[r]] = -1;   // processed no further: stays where it is
    int pos = 0;
    for (int r = J - 1; r >= 0; r--) {
      const int n = G.order[r];
      const int* b = nd + 6 * n;
      const int hx = (b[2] - b[0] + 1) >> 1, hy = (b[3] - b[1] + 1) >> 1, xm = b[0] + hx, ym = b[1] + hy;
      for (int q = 3; q >= 0; q--) {
        const int c = G.cnt4[4 * n + q];
        if (c == 0) { G.childpos[4 * n + q] = -1; continue; }
        int* o = nx + 6 * pos;
        o[0] = (q & 1) ? xm : b[0]; o[1] = (q & 2) ? ym : b[1]; o[2] = (q & 1) ? b[2] : xm; o[3] = (q & 2) ? b[3] : ym;
        o[4] = c; o[5] = c == 1 ? 1 : 0;
        G.childpos[4 * n + q] = pos++;
      }
    }
    for (int n = 0; n < S.size; n++) {
      if (G.newpos[n] <= -2) continue;
      const int* b = nd + 6 * n; int* o = nx + 6 * pos;
      for (int f = 0; f < 6; f++) o[f] = b[f];
      G.newpos[n] = pos++;
    }
    int32_t* vs = G.vsize[S.vs_cur ^ 1];
    int nvs = 0;
    for (int r = 0; r < J; r++) {
      const int n = G.order[r];
      for (int q = 0; q < 4; q++) if (G.cnt4[4 * n + q] > 1) vs[nvs++] = G.childpos[4 * n + q];
    }
    S.prev = S.size; S.size = pos; S.n_vs = nvs; S.vs_cur ^= 1; S.cur ^= 1;
  }
  __syncthreads();
  for (int k = tid; k < S.n_keys; k += nt) {
    const int n = G.knode[k];
    const int p = G.newpos[n];
    G.knode[k] = p <= -2 ? G.childpos[4 * n + G.kq[k]] : p;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kOctThreads) void orbx_octree(const GeoTable* T) {
  const int im = blockIdx.y, lv = blockIdx.x;
  const LevelGeo& G = T->g[im * T->n_levels + lv];
  __shared__ OctShared S;
  __shared__ int cell_off_total;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int n_cells = G.n_cols * G.n_rows;
  // compaction of the per-cell candidate slots into candidate order (cells row-major); cell offsets by a serial scan into newpos
  if (tid == 0) {
    int acc = 0;
    for (int c = 0; c < n_cells; c++) { G.newpos[c] = acc; acc += G.cell_cnt[c]; }
    cell_off_total = acc;
  }
  __syncthreads();
  const int n_keys = cell_off_total;
  for (int c = tid; c < n_cells; c += nt) {
    const int o = G.newpos[c], m = G.cell_cnt[c];
    for (int r = 0; r < m; r++) {
      G.kxy[o + r] = G.cand_xy[(size_t)c * G.cell_cap + r];
      G.kscore[o + r] = G.cand_score[(size_t)c * G.cell_cap + r];
    }
  }
  // initial nodes (:548-581)
  for (int i = tid; i < G.n_ini; i += nt) {
    int* b = G.nd[0] + 6 * i;
    b[0] = (int)__fmul_rn(G.hx, (float)i); b[1] = 0; b[2] = (int)__fmul_rn(G.hx, (float)(i + 1)); b[3] = G.max_by - kMinBorder;
    b[4] = 0; b[5] = 0;
  }
  if (tid == 0) {
    S.n_keys = n_keys; S.cur = 0; S.vs_cur = 0; S.n_vs = 0; S.iteration = 0; S.sorted_rounds = 0; S.finish_unchanged = 0; S.done = 0;
  }
  __syncthreads();
  for (int k = tid; k < n_keys; k += nt) {
    int n = (int)__fdiv_rn((float)(G.kxy[k] & 0xffff), G.hx);
    n = n < G.n_ini ? n : G.n_ini - 1;       // x < maxX - minX keeps n < nIni; the clamp only guards the buffer
    G.knode[k] = n;
    atomicAdd(&G.nd[0][6 * n + 4], 1);
  }
  __syncthreads();
  if (tid == 0) {                            // erase empty initial nodes, bNoMore at one key
    int pos = 0;
    for (int n = 0; n < G.n_ini; n++) {
      const int* b = G.nd[0] + 6 * n;
      if (b[4] == 0) { G.newpos[n] = -1; continue; }
      int* o = G.nd[1] + 6 * pos;
      for (int f = 0; f < 6; f++) o[f] = b[f];
      o[5] = b[4] == 1 ? 1 : 0;
      G.newpos[n] = pos++;
    }
    S.size = pos; S.cur = 1;
  }
  __syncthreads();
  for (int k = tid; k < n_keys; k += nt) G.knode[k] = G.newpos[G.knode[k]];
  __syncthreads();

  while (!S.done) {
    // main pass (:606-670): every node without bNoMore, in list order
    if (tid == 0) {
      S.iteration++;
      int r = 0;
      const int32_t* nd = G.nd[S.cur];
      for (int n = 0; n < S.size; n++) if (!nd[6 * n + 5]) G.order[r++] = n;
      S.n_order = r;
    }
    __syncthreads();
    oct_split_step(G, S, false);
    if (tid == 0) {
      if (S.size >= G.N || S.size == S.prev) { S.done = 1; S.finish_unchanged = S.size < G.N; }
      else if (S.size + 3 * S.n_vs > G.N) S.done = 2;
    }
    __syncthreads();
    while (S.done == 2) {
      // sorted phase (:673-738): the previous step's children with > 1 keys, largest first; equal sizes: later-created first
      const int m = S.n_vs;
      const int32_t* vs = G.vsize[S.vs_cur];
      const int32_t* nd = G.nd[S.cur];
      for (int a = tid; a < m; a += nt) {
        const int ca = nd[6 * vs[a] + 4];
        int rank = 0;
        for (int b = 0; b < m; b++) {
          const int cb = nd[6 * vs[b] + 4];
          rank += (cb > ca) || (cb == ca && b > a);
        }
        G.order[rank] = vs[a];
      }
      if (tid == 0) { S.n_order = m; S.sorted_rounds++; }
      __syncthreads();
      oct_split_step(G, S, true);
      if (tid == 0 && (S.size >= G.N || S.size == S.prev)) { S.done = 1; S.finish_unchanged = S.size < G.N; }
      __syncthreads();
    }
  }
  // retain the first key of greatest response per node (:741-760)
  for (int n = tid; n < S.size; n += nt) G.best[n] = 0ull;
  __syncthreads();
  for (int k = tid; k < n_keys; k += nt)
    atomicMax(&G.best[G.knode[k]], ((unsigned long long)(uint32_t)G.kscore[k] << 32) | (unsigned long long)(0xffffffffu - (uint32_t)k));
  __syncthreads();
  const int n_out = S.size < G.res_cap ? S.size : G.res_cap;
  for (int n = tid; n < n_out; n += nt) {
    const int k = (int)(0xffffffffu - (uint32_t)(G.best[n] & 0xffffffffull));
    G.res[3 * n] = (G.kxy[k] & 0xffff) + kMinBorder;
    G.res[3 * n + 1] = (G.kxy[k] >> 16) + kMinBorder;
    G.res[3 * n + 2] = G.kscore[k];
  }
  if (tid == 0) {
    G.stats[0] = n_keys; G.stats[3] = S.iteration; G.stats[4] = S.sorted_rounds; G.stats[5] = S.finish_unchanged;
    G.stats[6] = n_out; G.stats[7] = G.N;
  }
}

// ---------------------------------------------------------------------------------------------------- orientation, descriptor
struct EmitArgs {
  int umax[16];
  float scale[LLD_ORB_MAX_LEVELS];
  int8_t pattern[512][2];
};

// OpenCV's fastAtan2, every operation rounded separately
__device__ inline float fast_atan2(float y, float x) {
  const float k = (float)(180.0 / M_PI);
  const float p1 = __fmul_rn(0.9997878412794807f, k), p3 = __fmul_rn(-0.3258083974640975f, k);
  const float p5 = __fmul_rn(0.1555786518463281f, k), p7 = __fmul_rn(-0.04432655554792128f, k);
  const float ax = fabsf(x), ay = fabsf(y), eps = (float)2.220446049250313e-16;
  float a, c, c2;
  if (ax >= ay) { c = __fdiv_rn(ay, __fadd_rn(ax, eps)); }
  else { c = __fdiv_rn(ax, __fadd_rn(ay, eps)); }
  c2 = __fmul_rn(c, c);
  a = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
  if (!(ax >= ay)) a = __fsub_rn(90.f, a);
  if (x < 0) a = __fsub_rn(180.f, a);
  if (y < 0) a = __fsub_rn(360.f, a);
  return a;
}

__global__ void orbx_emit(const GeoTable* T, EmitArgs A, char* out, size_t out_stride, int cap) {
  const int im = blockIdx.y, lv = blockIdx.z;
  const LevelGeo& G = T->g[im * T->n_levels + lv];
  int off = 0;
  for (int l = 0; l < lv; l++) off += T->g[im * T->n_levels + l].stats[6];
  const int n = G.stats[6];
  char* o = out + (size_t)im * out_stride;
  float* xy = (float*)o; int32_t* oct = (int32_t*)(o + (size_t)cap * 8); float* ang = (float*)(o + (size_t)cap * 12);
  float* resp = (float*)(o + (size_t)cap * 16); float* sz = (float*)(o + (size_t)cap * 20); uint32_t* desc = (uint32_t*)(o + (size_t)cap * 24);
  if (lv == T->n_levels - 1 && blockIdx.x == 0 && threadIdx.x == 0) *(int32_t*)(o + (size_t)cap * 56) = off + n;
  const float factor_pi = (float)(M_PI / 180.0);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int x = G.res[3 * i], y = G.res[3 * i + 1];
    // IC_Angle on the unblurred level
    const uint8_t* c = G.img + (size_t)y * G.step + x;
    int m01 = 0, m10 = 0;
    for (int u = -kHalfPatch; u <= kHalfPatch; u++) m10 += u * c[u];
    for (int v = 1; v <= kHalfPatch; v++) {
      int vs = 0;
      const int d = A.umax[v];
      for (int u = -d; u <= d; u++) {
        const int vp = c[u + v * G.step], vm = c[u - v * G.step];
        vs += vp - vm; m10 += u * (vp + vm);
      }
      m01 += v * vs;
    }
    const float angle = fast_atan2((float)m01, (float)m10);
    // computeOrbDescriptor on the blurred level
    const float ar = __fmul_rn(angle, factor_pi);
    const float a = lld_glibc_sincosf(ar, 1), b = lld_glibc_sincosf(ar, 0);
    const uint8_t* cb = G.blur + (size_t)y * G.step + x;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int bit = 0; bit < 256; bit++) {
      int t[2];
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const float px = (float)A.pattern[2 * bit + e][0], py = (float)A.pattern[2 * bit + e][1];
        const int ry = cv_round(__fadd_rn(__fmul_rn(px, b), __fmul_rn(py, a)));
        const int rx = cv_round(__fsub_rn(__fmul_rn(px, a), __fmul_rn(py, b)));
        t[e] = cb[ry * G.step + rx];
      }
      w[bit >> 5] |= (uint32_t)(t[0] < t[1]) << (bit & 31);
    }
    const int j = off + i;
    const float s = A.scale[lv];
    xy[2 * j] = lv ? __fmul_rn((float)x, s) : (float)x;
    xy[2 * j + 1] = lv ? __fmul_rn((float)y, s) : (float)y;
    oct[j] = lv; ang[j] = angle; resp[j] = (float)G.res[3 * i + 2];
    sz[j] = (float)(int)(31.f * s);
    for (int q = 0; q < 8; q++) desc[8 * j + q] = w[q];
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- host side
struct lld_orb_extractor {
  lld_ctx* ctx = nullptr;
  lld_orb_extractor_params p{};
  lld_orb_extractor_levels lv{};
  int8_t pattern[512][2];
  int cap_keys = 0;                         // per-image output capacity (max_keypoints)
  void* dmem = nullptr;                     // one slab for every buffer
  GeoTable* d_geo = nullptr; GeoTable* h_geo = nullptr; size_t geo_bytes = 0;
  std::vector<LevelGeo> slots;              // [max_images * n_levels] buffers sized for max_cols x max_rows
  char* d_out = nullptr; char* h_out = nullptr; size_t out_stride = 0;
  int last_n_images = 0;
};

namespace {

struct LevelShape { int cols, rows, n_cols, n_rows, w_cell, h_cell, max_bx, max_by, n_ini; float hx; };

// ComputeKeyPointsOctTree's cell grid and DistributeOctTree's initial split for one level; false where the reference divides by zero
bool level_shape(int cols, int rows, LevelShape* s) {
  s->cols = cols; s->rows = rows;
  s->max_bx = cols - kEdge + 3; s->max_by = rows - kEdge + 3;
  const float width = (float)(s->max_bx - kMinBorder), height = (float)(s->max_by - kMinBorder);
  if (!(width > 0.f) || !(height > 0.f)) return false;
  s->n_cols = (int)(width / 30.f); s->n_rows = (int)(height / 30.f);
  if (s->n_cols < 1 || s->n_rows < 1) return false;
  s->w_cell = (int)std::ceil(width / (float)s->n_cols); s->h_cell = (int)std::ceil(height / (float)s->n_rows);
  s->n_ini = (int)std::round((float)(s->max_bx - kMinBorder) / (float)(s->max_by - kMinBorder));
  if (s->n_ini < 1) return false;
  s->hx = (float)(s->max_bx - kMinBorder) / (float)s->n_ini;
  return true;
}

int level_res_cap(int N, int n_ini) { return std::max(N + 3, 4 * n_ini); }

}  // namespace

extern "C" int lld_orb_extractor_create(lld_ctx* ctx, const lld_orb_extractor_params* prm, lld_orb_extractor** out) {
  if (!ctx || !prm || !out || !prm->pattern) return LLD_ERR_INVALID;
  *out = nullptr;
  const lld_orb_extractor_params& P = *prm;
  if (P.n_levels < 1 || P.n_levels > LLD_ORB_MAX_LEVELS || P.nfeatures < 0 || !(P.scale_factor > 1.f) || !std::isfinite(P.scale_factor) ||
      P.ini_th_fast < 1 || P.ini_th_fast > 255 || P.min_th_fast < 1 || P.min_th_fast > 255 || P.max_images < 1 || P.max_images > 8 ||
      P.max_cols < 1 || P.max_rows < 1 || P.max_cols > kMaxSide || P.max_rows > kMaxSide)
    return LLD_ERR_INVALID;
  for (int i = 0; i < 1024; i++) if (P.pattern[i] < -13 || P.pattern[i] > 13) return LLD_ERR_INVALID;
  lld_orb_extractor* ex = new lld_orb_extractor();
  ex->ctx = ctx; ex->p = P; ex->p.pattern = nullptr;
  for (int i = 0; i < 512; i++) { ex->pattern[i][0] = (int8_t)P.pattern[2 * i]; ex->pattern[i][1] = (int8_t)P.pattern[2 * i + 1]; }
  // level tables (:411-470)
  lld_orb_extractor_levels& L = ex->lv;
  const int nl = P.n_levels;
  L.n_levels = nl;
  L.scale_factor[0] = 1.f; L.level_sigma2[0] = 1.f;
  for (int i = 1; i < nl; i++) { L.scale_factor[i] = L.scale_factor[i - 1] * P.scale_factor; L.level_sigma2[i] = L.scale_factor[i] * L.scale_factor[i]; }
  for (int i = 0; i < nl; i++) { L.inv_scale_factor[i] = 1.0f / L.scale_factor[i]; L.inv_level_sigma2[i] = 1.0f / L.level_sigma2[i]; }
  const float factor = 1.0f / P.scale_factor;
  float nd = (float)P.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nl));
  int sum = 0;
  for (int l = 0; l < nl - 1; l++) { L.features_per_level[l] = cv_round(nd); sum += L.features_per_level[l]; nd *= factor; }
  L.features_per_level[nl - 1] = std::max(P.nfeatures - sum, 0);
  const int vmax = (int)std::floor(kHalfPatch * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(kHalfPatch * std::sqrt(2.f) / 2);
  const double hp2 = kHalfPatch * kHalfPatch;
  for (int v = 0; v <= vmax; v++) L.umax[v] = cv_round((float)std::sqrt(hp2 - v * v));
  for (int v = kHalfPatch, v0 = 0; v >= vmin; --v) { while (L.umax[v0] == L.umax[v0 + 1]) ++v0; L.umax[v] = v0; ++v0; }
  // buffers for the largest image
  const int nslot = P.max_images * nl;
  ex->slots.assign(nslot, LevelGeo{});
  size_t bytes = 0;
  std::vector<size_t> lvl_bytes(nl);
  int cap = 0;
  std::vector<int> maxc(nl), maxr(nl), keycap(nl), nodecap(nl), rescap(nl), cellsmax(nl);
  for (int l = 0; l < nl; l++) {
    maxc[l] = l ? cv_round((float)P.max_cols * L.inv_scale_factor[l]) : P.max_cols;
    maxr[l] = l ? cv_round((float)P.max_rows * L.inv_scale_factor[l]) : P.max_rows;
    // candidate slots: nCols cells of wCell = ceil(width / nCols) slots span < width + nCols <= maxc + maxc / 30 columns (more than
    // maxc when width / nCols has a fraction, e.g. 4096 -> 135 cells of 31), likewise for rows
    keycap[l] = std::max((maxc[l] + maxc[l] / 30) * (maxr[l] + maxr[l] / 30), 1);
    const int ini_max = std::max(maxc[l] / 30 + 2, 1);
    nodecap[l] = keycap[l] + ini_max + 8;
    rescap[l] = level_res_cap(L.features_per_level[l], ini_max);
    cellsmax[l] = std::max((maxc[l] / 30 + 1) * (maxr[l] / 30 + 1), 1);
    cap += rescap[l];
    const size_t px = lld_slab::pad((size_t)maxc[l] * maxr[l] + 64);
    lvl_bytes[l] = 3 * px + lld_slab::pad(cellsmax[l] * 4) + lld_slab::pad((size_t)keycap[l] * 4) + lld_slab::pad(keycap[l]) +
                   3 * lld_slab::pad((size_t)keycap[l] * 4) + lld_slab::pad(keycap[l]) + 2 * lld_slab::pad((size_t)nodecap[l] * 24) +
                   2 * lld_slab::pad((size_t)nodecap[l] * 16) + 4 * lld_slab::pad((size_t)nodecap[l] * 4) + lld_slab::pad((size_t)nodecap[l] * 8) +
                   lld_slab::pad((size_t)rescap[l] * 12) + lld_slab::pad(32);
    bytes += lvl_bytes[l] * P.max_images;
  }
  ex->cap_keys = cap; L.max_keypoints = cap;
  ex->out_stride = lld_slab::pad((size_t)cap * 56 + 4);
  ex->geo_bytes = sizeof(GeoTable) + sizeof(LevelGeo) * nslot;
  bytes += ex->out_stride * P.max_images + lld_slab::pad(ex->geo_bytes);
  int st = LLD_OK;
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&ex->dmem, bytes) != hipSuccess) { delete ex; return LLD_ERR_ALLOC; }
  if (hipHostMalloc((void**)&ex->h_out, ex->out_stride * P.max_images, hipHostMallocDefault) != hipSuccess ||
      hipHostMalloc((void**)&ex->h_geo, ex->geo_bytes, hipHostMallocDefault) != hipSuccess) st = LLD_ERR_ALLOC;
  if (st) { lld_orb_extractor_destroy(ex); return st; }
  lld_slab S; S.base = (char*)ex->dmem; S.size = bytes;
  ex->d_geo = (GeoTable*)S.take<char>(ex->geo_bytes);
  ex->d_out = S.take<char>(ex->out_stride * P.max_images);
  for (int im = 0; im < P.max_images; im++)
    for (int l = 0; l < nl; l++) {
      LevelGeo& g = ex->slots[im * nl + l];
      const size_t px = (size_t)maxc[l] * maxr[l] + 64;
      g.img = S.take<uint8_t>(px); g.blur = S.take<uint8_t>(px); g.score = S.take<uint8_t>(px);
      g.cell_cnt = S.take<int32_t>(cellsmax[l]);
      g.cand_xy = S.take<int32_t>(keycap[l]); g.cand_score = S.take<uint8_t>(keycap[l]);
      g.kxy = S.take<int32_t>(keycap[l]); g.kscore = S.take<int32_t>(keycap[l]); g.knode = S.take<int32_t>(keycap[l]); g.kq = S.take<int8_t>(keycap[l]);
      g.nd[0] = S.take<int32_t>((size_t)nodecap[l] * 6); g.nd[1] = S.take<int32_t>((size_t)nodecap[l] * 6);
      g.cnt4 = S.take<int32_t>((size_t)nodecap[l] * 4); g.childpos = S.take<int32_t>((size_t)nodecap[l] * 4);
      g.newpos = S.take<int32_t>(nodecap[l]); g.order = S.take<int32_t>(nodecap[l]);
      g.vsize[0] = S.take<int32_t>(nodecap[l]); g.vsize[1] = S.take<int32_t>(nodecap[l]);
      g.best = S.take<unsigned long long>(nodecap[l]);
      g.res = S.take<int32_t>((size_t)rescap[l] * 3); g.stats = S.take<int32_t>(8);
      g.key_cap = keycap[l]; g.node_cap = nodecap[l]; g.res_cap = rescap[l]; g.cell_cap = 0;
      g.N = L.features_per_level[l];
    }
  if (S.used > S.size) { lld_orb_extractor_destroy(ex); return LLD_ERR_ALLOC; }
  *out = ex;
  return LLD_OK;
}

extern "C" void lld_orb_extractor_destroy(lld_orb_extractor* ex) {
  if (!ex) return;
  if (ex->dmem) (void)hipFree(ex->dmem);
  if (ex->h_out) (void)hipHostFree(ex->h_out);
  if (ex->h_geo) (void)hipHostFree(ex->h_geo);
  delete ex;
}

extern "C" int lld_orb_extractor_levels_get(const lld_orb_extractor* ex, lld_orb_extractor_levels* out) {
  if (!ex || !out) return LLD_ERR_INVALID;
  *out = ex->lv;
  return LLD_OK;
}

extern "C" int lld_orb_extract(lld_orb_extractor* ex, int n_images, const lld_orb_image* images, lld_orb_features* outs) {
  if (!ex || !images || !outs || n_images < 1 || n_images > ex->p.max_images) return LLD_ERR_INVALID;
  const int nl = ex->p.n_levels;
  GeoTable* H = ex->h_geo;
  // validate everything before anything is queued, into local storage: H still describes the last successful call's pyramid
  // (lld_orb_extractor_pyramids) until every image has passed
  std::vector<LevelGeo> geo((size_t)n_images * nl);
  for (int im = 0; im < n_images; im++) {
    const lld_orb_image& I = images[im];
    const lld_orb_features& O = outs[im];
    if (!I.data || I.cols < 1 || I.rows < 1 || I.cols > ex->p.max_cols || I.rows > ex->p.max_rows || I.step < I.cols) return LLD_ERR_INVALID;
    if (!O.xy || !O.octave || !O.angle || !O.response || !O.size || !O.desc) return LLD_ERR_INVALID;
    int need = 0;
    for (int l = 0; l < nl; l++) {
      LevelShape s;
      const int c = l ? cv_round((float)I.cols * ex->lv.inv_scale_factor[l]) : I.cols;
      const int r = l ? cv_round((float)I.rows * ex->lv.inv_scale_factor[l]) : I.rows;
      if (!level_shape(c, r, &s)) return LLD_ERR_INVALID;
      LevelGeo& g = geo[im * nl + l];
      g = ex->slots[im * nl + l];
      g.cols = c; g.rows = r; g.step = c;
      g.n_cols = s.n_cols; g.n_rows = s.n_rows; g.w_cell = s.w_cell; g.h_cell = s.h_cell;
      g.max_bx = s.max_bx; g.max_by = s.max_by; g.n_ini = s.n_ini; g.hx = s.hx;
      g.cell_cap = s.w_cell * s.h_cell;
      if ((size_t)g.n_cols * g.n_rows * g.cell_cap > (size_t)g.key_cap || g.n_ini > g.node_cap - g.key_cap ||
          level_res_cap(g.N, s.n_ini) > g.res_cap)
        return LLD_ERR_INVALID;                  // cannot happen for an image within max_cols x max_rows; kept as the bound check
      need += level_res_cap(g.N, s.n_ini);
    }
    if (O.capacity < need) return LLD_ERR_INVALID;
  }
  std::copy(geo.begin(), geo.end(), H->g);
  H->n_images = n_images; H->n_levels = nl; H->min_th = ex->p.min_th_fast; H->ini_th = ex->p.ini_th_fast;
  hipStream_t st = ex->ctx->stream;
  LLD_HIP_TRY(hipSetDevice(ex->ctx->device));
  LLD_HIP_TRY(hipMemcpyAsync(ex->d_geo, H, ex->geo_bytes, hipMemcpyHostToDevice, st));
  int maxc = 0, maxr = 0, maxcells = 0;
  for (int im = 0; im < n_images; im++) {
    const LevelGeo& g = H->g[im * nl];
    LLD_HIP_TRY(hipMemcpy2DAsync(g.img, g.step, images[im].data, images[im].step, g.cols, g.rows,
                                 images[im].on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    for (int l = 0; l < nl; l++) {
      const LevelGeo& gl = H->g[im * nl + l];
      LLD_HIP_TRY(hipMemsetAsync(gl.stats, 0, 32, st));
      maxcells = std::max(maxcells, gl.n_cols * gl.n_rows);
    }
    maxc = std::max(maxc, g.cols); maxr = std::max(maxr, g.rows);
  }
  const dim3 blk(32, 8);
  for (int l = 1; l < nl; l++) {
    int c = 0, r = 0;
    for (int im = 0; im < n_images; im++) { c = std::max(c, H->g[im * nl + l].cols); r = std::max(r, H->g[im * nl + l].rows); }
    hipLaunchKernelGGL(orbx_resize, dim3((c + 31) / 32, (r + 7) / 8, n_images), blk, 0, st, ex->d_geo, l);
  }
  const dim3 grid_px((maxc + 31) / 32, (maxr + 7) / 8, n_images * nl);
  hipLaunchKernelGGL(orbx_score, grid_px, blk, 0, st, ex->d_geo);
  hipLaunchKernelGGL(orbx_blur, grid_px, blk, 0, st, ex->d_geo);
  hipLaunchKernelGGL(orbx_cells, dim3(maxcells, 1, n_images * nl), dim3(64), 0, st, ex->d_geo);
  hipLaunchKernelGGL(orbx_octree, dim3(nl, n_images), dim3(kOctThreads), 0, st, ex->d_geo);
  EmitArgs A;
  std::memcpy(A.umax, ex->lv.umax, sizeof(A.umax));
  std::memcpy(A.scale, ex->lv.scale_factor, sizeof(A.scale));
  std::memcpy(A.pattern, ex->pattern, sizeof(A.pattern));
  hipLaunchKernelGGL(orbx_emit, dim3(4, n_images, nl), dim3(256), 0, st, ex->d_geo, A, ex->d_out, ex->out_stride, ex->cap_keys);
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(ex->h_out, ex->d_out, ex->out_stride * n_images, hipMemcpyDeviceToHost, st));
  std::vector<int32_t> stats((size_t)n_images * nl * 8);
  for (int im = 0; im < n_images; im++)
    for (int l = 0; l < nl; l++)
      LLD_HIP_TRY(hipMemcpyAsync(&stats[((size_t)im * nl + l) * 8], H->g[im * nl + l].stats, 32, hipMemcpyDeviceToHost, st));
  LLD_HIP_TRY(hipStreamSynchronize(st));
  const int cap = ex->cap_keys;
  for (int im = 0; im < n_images; im++) {
    const char* o = ex->h_out + ex->out_stride * im;
    lld_orb_features& O = outs[im];
    const int n = *(const int32_t*)(o + (size_t)cap * 56);
    if (n < 0 || n > O.capacity || n > cap) return LLD_ERR_HIP;
    O.n = n;
    std::memcpy(O.xy, o, (size_t)n * 8);
    std::memcpy(O.octave, o + (size_t)cap * 8, (size_t)n * 4);
    std::memcpy(O.angle, o + (size_t)cap * 12, (size_t)n * 4);
    std::memcpy(O.response, o + (size_t)cap * 16, (size_t)n * 4);
    std::memcpy(O.size, o + (size_t)cap * 20, (size_t)n * 4);
    std::memcpy(O.desc, o + (size_t)cap * 24, (size_t)n * 32);
    if (O.stats) std::memcpy(O.stats, &stats[(size_t)im * nl * 8], (size_t)nl * 32);
  }
  ex->last_n_images = n_images;
  return LLD_OK;
}

extern "C" int lld_orb_extractor_pyramids(const lld_orb_extractor* ex, int image_index, const uint8_t** levels, int32_t* cols, int32_t* rows,
                                          int32_t* step) {
  if (!ex || !levels || image_index < 0 || image_index >= ex->last_n_images) return LLD_ERR_INVALID;
  const int nl = ex->p.n_levels;
  for (int l = 0; l < nl; l++) {
    const LevelGeo& g = ex->h_geo->g[image_index * nl + l];
    levels[l] = g.img;
    if (cols) cols[l] = g.cols;
    if (rows) rows[l] = g.rows;
    if (step) step[l] = g.step;
  }
  return LLD_OK;
}

// ---- what lld_frame_build.hip reads in place (lld_stereo_internal.h)
int lld_stereo::extracted_image(const lld_orb_extractor* ex, int image, ExtractedImage* out) {
  if (!ex || !out || image < 0 || image >= ex->last_n_images) return LLD_ERR_INVALID;
  const size_t cap = (size_t)ex->cap_keys;
  const char* d = ex->d_out + ex->out_stride * image; const char* h = ex->h_out + ex->out_stride * image;
  std::memset(out, 0, sizeof(*out));
  out->n = *(const int32_t*)(h + cap * 56);
  out->d_xy = (const float*)d; out->d_octave = (const int32_t*)(d + cap * 8); out->d_angle = (const float*)(d + cap * 12);
  out->d_desc = (const uint32_t*)(d + cap * 24);
  out->h_octave = (const int32_t*)(h + cap * 8);
  const int nl = ex->p.n_levels;
  for (int l = 0; l < nl; l++) {
    const LevelGeo& g = ex->h_geo->g[image * nl + l];
    out->level[l] = g.img; out->cols[l] = g.cols; out->rows[l] = g.rows; out->step[l] = g.step;
  }
  return LLD_OK;
}
lld_ctx* lld_stereo::extractor_context(const lld_orb_extractor* ex) { return ex->ctx; }
const lld_orb_extractor_levels* lld_stereo::extractor_levels(const lld_orb_extractor* ex) { return &ex->lv; }

extern "C" int lld_orb_extractor_descriptors(const lld_orb_extractor* ex, int image_index, const uint32_t** desc, int32_t* n) {
  if (!ex || !desc || !n || image_index < 0 || image_index >= ex->last_n_images) return LLD_ERR_INVALID;
  const size_t cap = (size_t)ex->cap_keys;
  *desc = (const uint32_t*)(ex->d_out + ex->out_stride * image_index + cap * 24);
  *n = *(const int32_t*)(ex->h_out + ex->out_stride * image_index + cap * 56);     // the count lld_orb_extract brought back
  return LLD_OK;
}
