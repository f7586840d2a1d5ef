// lld_match.hip — descriptor matching kernels (gfx950).
//
//   hamming256_best2   ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1647-1663) + the best/second-best loops of
//                      the Search* family (e.g. :76-114): lane <-> query (two queries per lane), the four waves of a
//                      workgroup split a train tile that is staged through LDS and read back as wave-uniform
//                      (broadcast) ds_read_b128; xor + v_bcnt accumulate per word; running (best, second) kept as
//                      packed (distance, order) keys so that the lexicographic minimum reproduces the reference's
//                      strict '<' ("first candidate wins ties"); cross-wave merge through LDS.
//   l2f32_best2        LineMatcher::MatchLineDescriptors argmin loops (src/TwoFrameLineMatcher.cc:112, Tracking.cc:1092,
//                      1532) with the build-defined float-L2 distance (parity unpinned: LBDMOD is not vendored).
// The line matchers (TwoFrameLineMatcher::MatchLines, Tracking::AddLinesFrom, Tracking::MatchLinesLastKF) are lld_line_match.hip's.
#include "lld_common.h"

namespace {

constexpr int kWave = 64;
constexpr int kMatchThreads = 256;             // 4 waves
constexpr int kQPerLane = 4;                   // queries per lane: one pair of broadcast LDS reads feeds kQPerLane distance computations
constexpr int kQPerBlock = kQPerLane * 64;     // all 4 waves see the same 256 queries and split the train rows
constexpr int kTileRows = 256;                 // train rows staged per LDS tile (8 KiB)
constexpr unsigned kIdxBits = 22;              // packed key = dist << 22 | order  (order < 4 Mi)
constexpr unsigned kKeyEmpty = (256u << kIdxBits) | ((1u << kIdxBits) - 1u);

__device__ __forceinline__ void key_update(unsigned key, unsigned& best, unsigned& second) {
  // lexicographic top-2: second = min(second, max(best, key)); best = min(best, key)
  // with best <= second the new second is the median of the three (one v_med3_u32 instead of a max and a min)
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(second) : "v"(best), "v"(second), "v"(key));
  best = min(best, key);
}

// v_bcnt_u32_b32 D = popcount(S0) + S1: the eight words of a descriptor pair are counted in one accumulating chain.  Written as asm
// because the compiler prefers eight independent counts and three v_add3_u32 (shorter chains, 3 more instructions per pair); the brute-
// force kernel has four independent queries per lane to fill the chain's latency and is bound by VALU issue.
__device__ __forceinline__ unsigned bcnt_acc(unsigned x, unsigned acc) {
  unsigned d;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(acc));
  return d;
}
__device__ __forceinline__ unsigned hamming8(const uint4& qa, const uint4& qb, const uint4& ta, const uint4& tb) {
  unsigned d = __popc(qa.x ^ ta.x);
  d = bcnt_acc(qa.y ^ ta.y, d); d = bcnt_acc(qa.z ^ ta.z, d); d = bcnt_acc(qa.w ^ ta.w, d);
  d = bcnt_acc(qb.x ^ tb.x, d); d = bcnt_acc(qb.y ^ tb.y, d); d = bcnt_acc(qb.z ^ tb.z, d); d = bcnt_acc(qb.w ^ tb.w, d);
  return d;
}

// grid (ceil(nq / kQPerBlock), batch); block 256.
__global__ __launch_bounds__(kMatchThreads) void hamming256_best2_kernel(
    const uint4* __restrict__ q, int nq, const uint4* __restrict__ t, int nt, const uint8_t* __restrict__ mask,
    int* __restrict__ best_idx, int* __restrict__ best_dist, int* __restrict__ second_idx, int* __restrict__ second_dist) {
  __shared__ uint4 tile[kTileRows * 2];                       // 8 KiB train tile
  __shared__ unsigned merge[4][kQPerBlock][2];                // per-wave (best, second) keys
  const int pair = blockIdx.y;
  q += (size_t)pair * nq * 2; t += (size_t)pair * nt * 2;
  const size_t out_off = (size_t)pair * nq;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  uint4 qa[kQPerLane], qb[kQPerLane];
  unsigned best[kQPerLane], sec[kQPerLane];
  const uint8_t* mrow[kQPerLane];
#pragma unroll
  for (int k = 0; k < kQPerLane; k++) {
    const int qk = blockIdx.x * kQPerBlock + k * kWave + lane;
    const bool v = qk < nq;
    qa[k] = v ? q[qk * 2] : make_uint4(0, 0, 0, 0); qb[k] = v ? q[qk * 2 + 1] : make_uint4(0, 0, 0, 0);
    best[k] = kKeyEmpty; sec[k] = kKeyEmpty;
    mrow[k] = mask ? mask + ((size_t)pair * nq + (v ? qk : 0)) * nt : nullptr;
  }
  for (int base = 0; base < nt; base += kTileRows) {
    const int rows = min(kTileRows, nt - base);
    __syncthreads();                                           // previous tile fully consumed
    for (int i = threadIdx.x; i < rows * 2; i += kMatchThreads) tile[i] = t[(size_t)base * 2 + i];   // 16 B / lane, coalesced
    __syncthreads();
    // wave w takes rows w, w+4, ... of the tile; LDS reads are wave-uniform (broadcast, conflict-free)
    for (int r = wave; r < rows; r += 4) {
      const uint4 ta = tile[r * 2], tb = tile[r * 2 + 1];
      const unsigned j = (unsigned)(base + r);
#pragma unroll
      for (int k = 0; k < kQPerLane; k++) {
        unsigned key = (hamming8(qa[k], qb[k], ta, tb) << kIdxBits) | j;
        if (mask && !mrow[k][j]) key = kKeyEmpty;
        key_update(key, best[k], sec[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kQPerLane; k++) { merge[wave][k * kWave + lane][0] = best[k]; merge[wave][k * kWave + lane][1] = sec[k]; }
  __syncthreads();
  for (int qo = threadIdx.x; qo < kQPerBlock; qo += kMatchThreads) {
    const int qi = blockIdx.x * kQPerBlock + qo;
    if (qi < nq) {
      unsigned b = kKeyEmpty, s = kKeyEmpty;
      for (int w = 0; w < 4; w++) { key_update(merge[w][qo][0], b, s); key_update(merge[w][qo][1], b, s); }
      const unsigned idx_mask = (1u << kIdxBits) - 1u;
      best_idx[out_off + qi] = (b == kKeyEmpty) ? -1 : (int)(b & idx_mask);
      best_dist[out_off + qi] = (int)(b >> kIdxBits);
      second_idx[out_off + qi] = (s == kKeyEmpty) ? -1 : (int)(s & idx_mask);
      second_dist[out_off + qi] = (int)(s >> kIdxBits);
    }
  }
}

// Candidate-list form: one lane per query walks its own list (Frame::GetFeaturesInArea / BoW node order); the list
// position is the tie-break key, the output is the train index.
__global__ __launch_bounds__(256) void hamming256_csr_kernel(
    const uint4* __restrict__ q, int nq, const uint4* __restrict__ t, const int* __restrict__ cand_start, const int* __restrict__ cand_idx,
    int* __restrict__ best_idx, int* __restrict__ best_dist, int* __restrict__ second_idx, int* __restrict__ second_dist) {
  const int qi = blockIdx.x * blockDim.x + threadIdx.x;
  if (qi >= nq) return;
  const uint4 a = q[qi * 2], b = q[qi * 2 + 1];
  int bd = 256, bi = -1, sd = 256, si = -1;
  const int s = cand_start[qi], e = cand_start[qi + 1];
  for (int k = s; k < e; k++) {
    const int j = cand_idx[k];
    const int d = (int)hamming8(a, b, t[j * 2], t[j * 2 + 1]);
    if (d < bd) { sd = bd; si = bi; bd = d; bi = j; }
    else if (d < sd) { sd = d; si = j; }
  }
  best_idx[qi] = bi; best_dist[qi] = bd; second_idx[qi] = si; second_dist[qi] = sd;
}

// ------------------------------------------------------------------ float L2 (LBD)
// d = sqrt( sum_i (double)(a_i - b_i)^2 ), float difference, double accumulation in ascending i (the product of two
// floats is exact in double, so the fused multiply-add below rounds exactly like mul-then-add on the CPU).
// One wavefront per workgroup: the exact kernel holds a 72-float query and two rows' sums in 192 VGPRs (two wavefronts per SIMD), and the
// 300 queries of a frame pair are 4.7 wavefronts - in workgroups of 256 lanes the second one kept three idle wavefronts resident beside its
// single working one (5 working wavefronts in 8 slots).  Each wavefront now stages the train tile for itself (86 KB per pair and
// wavefront out of L2): 826 k -> 1.2 M frame pairs/s.
constexpr int kL2Threads = 64;
constexpr int kL2TileRows = 64;

// kExact: dim == DIM_MAX, known at compile time.  With a run-time dim every component of the unrolled sums sits behind its own `i < dim`
// branch: one ds_read_b32 per component, scalar registers spilled into lanes, 3158 instructions of which 225 are the FMAs.  The
// descriptor lengths in use (72: LBD, 32) therefore get the exact form, other lengths the guarded one.
template <int DIM_MAX, bool kExact>
__global__ __launch_bounds__(kL2Threads) void l2f32_best2_kernel(
    const float* __restrict__ q, int nq, const float* __restrict__ t, int nt, int dim_arg, const uint8_t* __restrict__ mask,
    int* __restrict__ best_idx, double* __restrict__ best_dist, int* __restrict__ second_idx, double* __restrict__ second_dist,
    double* __restrict__ dist_matrix /* optional [nq][nt] */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = reinterpret_cast<float*>(smem);                        // [kL2TileRows][dim]
  const int dim = kExact ? DIM_MAX : dim_arg;
  const int pair = blockIdx.y;
  q += (size_t)pair * nq * dim; t += (size_t)pair * nt * dim;
  const size_t out_off = (size_t)pair * nq;
  const int qi = blockIdx.x * kL2Threads + threadIdx.x;
  const bool valid = qi < nq;
  float qa[DIM_MAX];
#pragma unroll
  for (int i = 0; i < DIM_MAX; i++) qa[i] = (valid && (kExact || i < dim)) ? q[(size_t)qi * dim + i] : 0.f;
  double bd = 1.7976931348623157e308, sd = 1.7976931348623157e308;
  int bi = -1, si = -1;
  // (with workgroups of more than one wavefront: a wavefront without a single query only helps to stage the tiles)
  const bool wave_has_queries = blockIdx.x * kL2Threads + (threadIdx.x & ~63) < nq;
#define LLD_L2_TAKE(DIST, J)                                                                              \
  do {                                                                                                    \
    const double dist_ = (DIST); const int j_ = (J);                                                      \
    if (valid) {                                                                                          \
      if (dist_matrix) dist_matrix[((size_t)pair * nq + qi) * nt + j_] = dist_;                           \
      const bool cand_ = !mask || mask[((size_t)pair * nq + qi) * nt + j_];                               \
      if (cand_) {                                                                                        \
        if (dist_ < bd) { sd = bd; si = bi; bd = dist_; bi = j_; }                                        \
        else if (dist_ < sd) { sd = dist_; si = j_; }                                                     \
      }                                                                                                   \
    }                                                                                                     \
  } while (0)
  for (int base = 0; base < nt; base += kL2TileRows) {
    const int rows = min(kL2TileRows, nt - base);
    __syncthreads();
    for (int i = threadIdx.x; i < rows * dim; i += kL2Threads) tile[i] = t[(size_t)base * dim + i];
    __syncthreads();
    if (!wave_has_queries) continue;
    const float* tile_rows = tile;
    int r = 0;
    // two train rows at a time: two independent accumulation chains (each row's sum keeps its own index order, so the result is
    // bit-identical to the one-row loop and to the oracle)
    for (; r + 1 < rows; r += 2) {
      const float* tr0 = tile_rows + r * dim; const float* tr1 = tr0 + dim;
      double acc0 = 0.0, acc1 = 0.0;
#pragma unroll
      for (int i = 0; i < DIM_MAX; i++) {
        if (kExact || i < dim) {
          const float d0 = qa[i] - tr0[i], d1 = qa[i] - tr1[i];
          acc0 = fma((double)d0, (double)d0, acc0); acc1 = fma((double)d1, (double)d1, acc1);
        }
      }
      LLD_L2_TAKE(sqrt(acc0), base + r); LLD_L2_TAKE(sqrt(acc1), base + r + 1);
    }
    for (; r < rows; r++) {
      const float* tr = tile_rows + r * dim;
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < DIM_MAX; i++) {
        if (kExact || i < dim) { const float d = qa[i] - tr[i]; acc = fma((double)d, (double)d, acc); }
      }
      LLD_L2_TAKE(sqrt(acc), base + r);
    }
  }
#undef LLD_L2_TAKE
  if (valid) {
    best_idx[out_off + qi] = bi; best_dist[out_off + qi] = bd; second_idx[out_off + qi] = si; second_dist[out_off + qi] = sd;
  }
}

// Latency form of the same search for small problems (one frame pair): one wavefront per QUERY row, lanes stride over the train
// rows, so a 300 x 300 x 72 problem is 300 short wavefronts instead of two workgroups walking 21 600 dependent FMAs per lane.
// Same arithmetic per pair and the same lexicographic (distance, index) order, hence identical outputs.
__global__ __launch_bounds__(64) void l2f32_best2_row_kernel(const float* __restrict__ q, const float* __restrict__ t, int nt, int dim,
                                                            const uint8_t* __restrict__ mask, int* __restrict__ best_idx, double* __restrict__ best_dist,
                                                            int* __restrict__ second_idx, double* __restrict__ second_dist, double* __restrict__ dist_matrix) {
  extern __shared__ __attribute__((aligned(16))) float qrow_l2[];
  const int qi = blockIdx.x, lane = threadIdx.x;
  for (int i = lane; i < dim; i += 64) qrow_l2[i] = q[(size_t)qi * dim + i];
  __syncthreads();
  double bd = 1.7976931348623157e308, sd = 1.7976931348623157e308;
  int bi = 0x7fffffff, si = 0x7fffffff;
  for (int j = lane; j < nt; j += 64) {
    const float* tr = t + (size_t)j * dim;
    double acc = 0.0;
    for (int i = 0; i < dim; i++) { const float d = qrow_l2[i] - tr[i]; acc = fma((double)d, (double)d, acc); }
    const double dist = sqrt(acc);
    if (dist_matrix) dist_matrix[(size_t)qi * nt + j] = dist;
    if (mask && !mask[(size_t)qi * nt + j]) continue;
    if (dist < bd) { sd = bd; si = bi; bd = dist; bi = j; }            // ascending j per lane: strict '<' keeps the lower index
    else if (dist < sd) { sd = dist; si = j; }
  }
  auto less = [](double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); };
  for (int off = 32; off > 0; off >>= 1) {
    const double obd = __shfl_xor(bd, off), osd = __shfl_xor(sd, off);
    const int obi = __shfl_xor(bi, off), osi = __shfl_xor(si, off);
    // merge two sorted pairs (b, s) and (ob, os): the two smallest of the four in (distance, index) order
    if (less(obd, obi, bd, bi)) {
      if (less(bd, bi, osd, osi)) { sd = bd; si = bi; } else { sd = osd; si = osi; }
      bd = obd; bi = obi;
    } else if (less(obd, obi, sd, si)) { sd = obd; si = obi; }
  }
  if (lane == 0) {
    best_idx[qi] = bi == 0x7fffffff ? -1 : bi; best_dist[qi] = bd;
    second_idx[qi] = si == 0x7fffffff ? -1 : si; second_dist[qi] = sd;
  }
}

int launch_hamming(lld_ctx* ctx, int batch, const uint32_t* q, int nq, const uint32_t* t, int nt, const uint8_t* mask,
                   int* bi, int* bd, int* si, int* sd) {
  if (nt >= (1 << kIdxBits)) return LLD_ERR_UNSUPPORTED;
  dim3 grid((nq + kQPerBlock - 1) / kQPerBlock, batch);
  hipLaunchKernelGGL(hamming256_best2_kernel, grid, dim3(kMatchThreads), 0, ctx->stream, reinterpret_cast<const uint4*>(q), nq,
                     reinterpret_cast<const uint4*>(t), nt, mask, bi, bd, si, sd);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

int launch_l2(lld_ctx* ctx, int batch, const float* q, int nq, const float* t, int nt, int dim, const uint8_t* mask,
              int* bi, double* bd, int* si, double* sd, double* dist_matrix) {
  if (batch == 1 && nq <= 8192 && dim <= 128) {                       // one frame pair: the wavefront-per-row form
    hipLaunchKernelGGL(l2f32_best2_row_kernel, dim3(nq), dim3(64), (size_t)dim * sizeof(float), ctx->stream, q, t, nt, dim, mask, bi, bd, si, sd, dist_matrix);
    LLD_HIP_TRY(hipGetLastError());
    return LLD_OK;
  }
  dim3 grid((nq + kL2Threads - 1) / kL2Threads, batch);
  const size_t lds = (size_t)kL2TileRows * dim * sizeof(float);
#define LLD_L2_LAUNCH(N, EXACT)                                                                                                 \
  hipLaunchKernelGGL((l2f32_best2_kernel<N, EXACT>), grid, dim3(kL2Threads), lds, ctx->stream, q, nq, t, nt, dim, mask, bi, bd, si, sd, \
                     dist_matrix)
  if (dim == 32) LLD_L2_LAUNCH(32, true);
  else if (dim == 72) LLD_L2_LAUNCH(72, true);
  else if (dim <= 32) LLD_L2_LAUNCH(32, false);
  else if (dim <= 72) LLD_L2_LAUNCH(72, false);
  else if (dim <= 128) LLD_L2_LAUNCH(128, false);
  else return LLD_ERR_UNSUPPORTED;
#undef LLD_L2_LAUNCH
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

// the result of a host entry point: best / second index and distance of every query, then the call waits for them
template <class D>
int fetch_best2(lld_ctx* ctx, int nq, const int* dbi, const D* dbd, const int* dsi, const D* dsd, int32_t* best_idx, D* best_dist, int32_t* second_idx, D* second_dist) {
  LLD_HIP_TRY(hipMemcpyAsync(best_idx, dbi, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  LLD_HIP_TRY(hipMemcpyAsync(best_dist, dbd, (size_t)nq * sizeof(D), hipMemcpyDeviceToHost, ctx->stream));
  LLD_HIP_TRY(hipMemcpyAsync(second_idx, dsi, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  LLD_HIP_TRY(hipMemcpyAsync(second_dist, dsd, (size_t)nq * sizeof(D), hipMemcpyDeviceToHost, ctx->stream));
  LLD_HIP_TRY(hipStreamSynchronize(ctx->stream));
  return LLD_OK;
}

}  // namespace

extern "C" {

int lld_match_hamming256(lld_ctx* ctx, const uint32_t* q, int nq, const uint32_t* t, int nt, const uint8_t* mask,
                         int32_t* best_idx, int32_t* best_dist, int32_t* second_idx, int32_t* second_dist) {
  if (!ctx || !q || !t || nq < 0 || nt < 0 || !best_idx || !best_dist || !second_idx || !second_dist) return LLD_ERR_INVALID;
  if (nq == 0) return LLD_OK;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const size_t qb = lld_slab::pad((size_t)nq * 32), tb = lld_slab::pad((size_t)nt * 32 + 32), mb = mask ? lld_slab::pad((size_t)nq * nt) : 0;
  const size_t ob = lld_slab::pad((size_t)nq * 4);
  void* base; int st = lld_ctx_scratch(ctx, qb + tb + mb + 4 * ob, &base); if (st) return st;
  lld_slab s; s.base = (char*)base;
  uint32_t* dq = s.take<uint32_t>((size_t)nq * 8); uint32_t* dt = s.take<uint32_t>((size_t)nt * 8 + 8);
  uint8_t* dm = mask ? s.take<uint8_t>((size_t)nq * nt) : nullptr;
  int *dbi = s.take<int>(nq), *dbd = s.take<int>(nq), *dsi = s.take<int>(nq), *dsd = s.take<int>(nq);
  LLD_HIP_TRY(hipMemcpyAsync(dq, q, (size_t)nq * 32, hipMemcpyHostToDevice, ctx->stream));
  if (nt) LLD_HIP_TRY(hipMemcpyAsync(dt, t, (size_t)nt * 32, hipMemcpyHostToDevice, ctx->stream));
  if (mask) LLD_HIP_TRY(hipMemcpyAsync(dm, mask, (size_t)nq * nt, hipMemcpyHostToDevice, ctx->stream));
  st = launch_hamming(ctx, 1, dq, nq, dt, nt, dm, dbi, dbd, dsi, dsd); if (st) return st;
  return fetch_best2(ctx, nq, dbi, dbd, dsi, dsd, best_idx, best_dist, second_idx, second_dist);
}

int lld_match_hamming256_csr(lld_ctx* ctx, const uint32_t* q, int nq, const uint32_t* t, int nt, const int32_t* cand_start,
                             const int32_t* cand_idx, int32_t* best_idx, int32_t* best_dist, int32_t* second_idx, int32_t* second_dist) {
  if (!ctx || !q || !t || !cand_start || !cand_idx || nq < 0 || nt < 0) return LLD_ERR_INVALID;
  if (nq == 0) return LLD_OK;
  const int ncand = cand_start[nq];
  for (int i = 0; i < nq; i++) if (cand_start[i + 1] < cand_start[i]) return LLD_ERR_INVALID;
  for (int k = 0; k < ncand; k++) if (cand_idx[k] < 0 || cand_idx[k] >= nt) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const size_t need = lld_slab::pad((size_t)nq * 32) + lld_slab::pad((size_t)nt * 32 + 32) + lld_slab::pad((size_t)(nq + 1) * 4) +
                      lld_slab::pad((size_t)ncand * 4 + 4) + 4 * lld_slab::pad((size_t)nq * 4);
  void* base; int st = lld_ctx_scratch(ctx, need, &base); if (st) return st;
  lld_slab s; s.base = (char*)base;
  uint32_t* dq = s.take<uint32_t>((size_t)nq * 8); uint32_t* dt = s.take<uint32_t>((size_t)nt * 8 + 8);
  int* dcs = s.take<int>(nq + 1); int* dci = s.take<int>(ncand + 1);
  int *dbi = s.take<int>(nq), *dbd = s.take<int>(nq), *dsi = s.take<int>(nq), *dsd = s.take<int>(nq);
  LLD_HIP_TRY(hipMemcpyAsync(dq, q, (size_t)nq * 32, hipMemcpyHostToDevice, ctx->stream));
  if (nt) LLD_HIP_TRY(hipMemcpyAsync(dt, t, (size_t)nt * 32, hipMemcpyHostToDevice, ctx->stream));
  LLD_HIP_TRY(hipMemcpyAsync(dcs, cand_start, (size_t)(nq + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  if (ncand) LLD_HIP_TRY(hipMemcpyAsync(dci, cand_idx, (size_t)ncand * 4, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(hamming256_csr_kernel, dim3((nq + 255) / 256), dim3(256), 0, ctx->stream, reinterpret_cast<const uint4*>(dq), nq,
                     reinterpret_cast<const uint4*>(dt), dcs, dci, dbi, dbd, dsi, dsd);
  LLD_HIP_TRY(hipGetLastError());
  return fetch_best2(ctx, nq, dbi, dbd, dsi, dsd, best_idx, best_dist, second_idx, second_dist);
}

int lld_match_hamming256_batch_dev(lld_ctx* ctx, int batch, const uint32_t* q_dev, int nq, const uint32_t* t_dev, int nt,
                                   int32_t* best_idx_dev, int32_t* best_dist_dev, int32_t* second_idx_dev, int32_t* second_dist_dev) {
  if (!ctx || batch <= 0 || nq <= 0 || nt < 0 || !q_dev || !t_dev) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  return launch_hamming(ctx, batch, q_dev, nq, t_dev, nt, nullptr, best_idx_dev, best_dist_dev, second_idx_dev, second_dist_dev);
}

int lld_match_l2f32(lld_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, const uint8_t* mask,
                    int32_t* best_idx, double* best_dist, int32_t* second_idx, double* second_dist) {
  if (!ctx || !q || !t || nq < 0 || nt < 0 || dim <= 0) return LLD_ERR_INVALID;
  if (dim > 128) return LLD_ERR_UNSUPPORTED;
  if (nq == 0) return LLD_OK;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  const size_t need = lld_slab::pad((size_t)nq * dim * 4) + lld_slab::pad((size_t)nt * dim * 4 + 16) + (mask ? lld_slab::pad((size_t)nq * nt) : 0) +
                      2 * lld_slab::pad((size_t)nq * 4) + 2 * lld_slab::pad((size_t)nq * 8);
  void* base; int st = lld_ctx_scratch(ctx, need, &base); if (st) return st;
  lld_slab s; s.base = (char*)base;
  float* dq = s.take<float>((size_t)nq * dim); float* dt = s.take<float>((size_t)nt * dim + 4);
  uint8_t* dm = mask ? s.take<uint8_t>((size_t)nq * nt) : nullptr;
  int *dbi = s.take<int>(nq), *dsi = s.take<int>(nq); double *dbd = s.take<double>(nq), *dsd = s.take<double>(nq);
  LLD_HIP_TRY(hipMemcpyAsync(dq, q, (size_t)nq * dim * 4, hipMemcpyHostToDevice, ctx->stream));
  if (nt) LLD_HIP_TRY(hipMemcpyAsync(dt, t, (size_t)nt * dim * 4, hipMemcpyHostToDevice, ctx->stream));
  if (mask) LLD_HIP_TRY(hipMemcpyAsync(dm, mask, (size_t)nq * nt, hipMemcpyHostToDevice, ctx->stream));
  st = launch_l2(ctx, 1, dq, nq, dt, nt, dim, dm, dbi, dbd, dsi, dsd, nullptr); if (st) return st;
  return fetch_best2(ctx, nq, dbi, dbd, dsi, dsd, best_idx, best_dist, second_idx, second_dist);
}

int lld_match_l2f32_batch_dev(lld_ctx* ctx, int batch, const float* q_dev, int nq, const float* t_dev, int nt, int dim,
                              int32_t* best_idx_dev, double* best_dist_dev, int32_t* second_idx_dev, double* second_dist_dev) {
  if (!ctx || batch <= 0 || nq <= 0 || nt < 0 || dim <= 0) return LLD_ERR_INVALID;
  if (dim > 128) return LLD_ERR_UNSUPPORTED;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  return launch_l2(ctx, batch, q_dev, nq, t_dev, nt, dim, nullptr, best_idx_dev, best_dist_dev, second_idx_dev, second_dist_dev, nullptr);
}

}  // extern "C"
