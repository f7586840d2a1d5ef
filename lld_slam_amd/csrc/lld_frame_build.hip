// lld_frame_build.hip — the stereo Frame built on the device (lld_frame_build_stereo*, include/lld_amd.h): what Frame::Frame does between
// ORBextractor::operator() and the Tracking chain (src/Frame.cc:100-113, :159) without a trip through the host.
//   stage 1  row-band Hamming search (Frame.cc:536-613) -> stereo_rows_kernel: ONE WAVEFRONT PER LEFT KEYPOINT, a lane per right keypoint
//            (stride 64).  Every left keypoint is independent, so the grid is n_left wavefronts over the whole chip.  A lane applies the
//            reference's tests directly - octave +-1, (int)vL in [floor(yR-r), ceil(yR+r)], uR in [uL-maxD, uL-minD] - which is what
//            vRowIndices encodes; at <= 4096 x 4096 pairs of three float compares that costs less than building the row table would,
//            and there is no intermediate buffer, no atomic and no second launch.  The wave reduces on the key (distance << 12 | iR),
//            so the lowest iR wins ties as the reference's ascending loop with strict '<' does.  The same kernel moves the left
//            keypoints into the frame's own slab when they are read in place from somewhere else (the extractor's output).
//   stage 2  11x11 SAD refinement + parabola  \  the kernels of lld_stereo.hip through lld_stereo::refine_launch, writing u_right and depth
//   stage 3  median cut                       /  straight into the frame's arrays
// At most one host-to-device copy (none when everything comes from an extractor), no synchronisation: the call returns with the kernels
// queued on the context's stream, and the frame owns every byte the queued work and the later chain read, except the right keypoints and
// the pyramids of an extractor, which the stream orders before that extractor's next call.
#include "lld_stereo_internal.h"
#include "lld_track_internal.h"
#include "lld_wave.h"

namespace {

constexpr int kMaxLevels = LLD_ORB_MAX_LEVELS;
constexpr int kWave = 64, kBlock = 256;
constexpr int kThOrbDist = (100 + 50) / 2;            // (TH_HIGH + TH_LOW) / 2, Frame.cc:534
constexpr int kIdxBits = 12;                          // LLD_ORB_MAX_KEYPOINTS = 4096 right keypoints
static_assert(LLD_ORB_MAX_KEYPOINTS <= (1 << kIdxBits), "the reduction key packs iR into 12 bits");

struct RowsArgs {
  int n_left, n_right;
  // where the left keypoints are read, and the frame's own arrays; a pair that differs is copied (one keypoint per wavefront)
  const float* src_xy; const int32_t* src_octave; const float* src_angle; const uint32_t* src_desc;
  float* f_xy; int32_t* f_octave; float* f_angle; uint32_t* f_desc;
  const float* right_xy; const int32_t* right_octave; const uint32_t* right_desc;
  float scale[kMaxLevels];
  float min_d, max_d;
  int rows0;                                 // rows of level 0: a left keypoint whose row lies outside has no candidates
  int32_t* best_r;
};

__global__ __launch_bounds__(kBlock) void stereo_rows_kernel(RowsArgs A) {
  __shared__ float s_scale[kMaxLevels];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  if (tid < kMaxLevels) {
    float v = 1.f;
#pragma unroll
    for (int l = 0; l < kMaxLevels; l++) v = tid == l ? A.scale[l] : v;      // constant indices: the table stays in scalar registers
    s_scale[tid] = v;
  }
  __syncthreads();
  const int iL = blockIdx.x * (kBlock / kWave) + (tid >> 6);
  if (iL >= A.n_left) return;                                                 // whole wavefronts leave together
  const float uL = A.src_xy[2 * iL], vL = A.src_xy[2 * iL + 1];
  const int oL = A.src_octave[iL];
  uint32_t dl[8];
#pragma unroll
  for (int w = 0; w < 8; w++) dl[w] = A.src_desc[8 * iL + w];
  if (A.src_desc != A.f_desc && lane < 8) A.f_desc[8 * iL + lane] = A.src_desc[8 * iL + lane];
  if (lane == 0) {
    if (A.src_xy != A.f_xy) { A.f_xy[2 * iL] = uL; A.f_xy[2 * iL + 1] = vL; }
    if (A.src_octave != A.f_octave) A.f_octave[iL] = oL;
    if (A.src_angle != A.f_angle) A.f_angle[iL] = A.src_angle[iL];
  }
  const float minU = __fsub_rn(uL, A.max_d), maxU = __fsub_rn(uL, A.min_d);   // Frame.cc:574-575
  const long long row = (long long)vL;                                        // vRowIndices[vL], :569
  int best = 0x7fffffff;
  if (!(maxU < 0.f) && row >= 0 && row < A.rows0) {                           // :577-578; vRowIndices[vL] is indexed unchecked in the reference
    for (int iR = lane; iR < A.n_right; iR += kWave) {
      const int oR = A.right_octave[iR];
      if (oR < oL - 1 || oR > oL + 1) continue;                               // :589-590
      const float uR = A.right_xy[2 * iR], yR = A.right_xy[2 * iR + 1];
      const float r = __fmul_rn(2.0f, s_scale[min(max(oR, 0), kMaxLevels - 1)]);
      const long long maxr = (long long)ceilf(__fadd_rn(yR, r)), minr = (long long)floorf(__fsub_rn(yR, r));   // :546-556
      if (row < minr || row > maxr) continue;
      if (!(uR >= minU && uR <= maxU)) continue;                              // :594-596
      const int dist = lld_wave::hamming256(dl, A.right_desc + 8 * iR);
      best = min(best, (dist << kIdxBits) | iR);
    }
  }
  best = lld_wave::min(best);
  if (lane == 0) A.best_r[iL] = (best >> kIdxBits) < kThOrbDist ? (best & ((1 << kIdxBits) - 1)) : -1;       // bestDist < thOrbDist, :604
}

inline size_t al64(size_t b) { return (b + 63) & ~size_t(63); }

// One build, wherever its inputs live.  Device pointers unless named h_*.
struct BuildIn {
  int nl = 0, nr = 0, nlv = 0;
  bool kp_on_device = false;                 // left xy / angle / desc and the right side are device pointers, read in place
  const float* lxy = nullptr; const float* lang = nullptr; const uint32_t* ldesc = nullptr;
  const int32_t* loct_dev = nullptr;         // device octaves to read in place, or NULL: h_loct is uploaded
  const int32_t* h_loct = nullptr;           // host, always: the frame's host copy, and the upload when loct_dev is NULL
  const float* rxy = nullptr; const int32_t* roct = nullptr; const uint32_t* rdesc = nullptr;
  bool pyr_on_device = false;
  const uint8_t* limg[kMaxLevels] = {}; const uint8_t* rimg[kMaxLevels] = {};
  int cols[kMaxLevels] = {}, rows[kMaxLevels] = {}, lstep[kMaxLevels] = {}, rstep[kMaxLevels] = {};
  const float* pyr_scale = nullptr; const float* pyr_inv_scale = nullptr;                  // [nlv] host
  const float* level_scale = nullptr; const float* level_sigma2 = nullptr; const float* level_inv_sigma2 = nullptr;   // [nlv] host
  const lld_frame_stereo_params* prm = nullptr;
};

int build(lld_ctx* ctx, const BuildIn& B, lld_frame** out) {
  const int nl = B.nl, nr = B.nr, nlv = B.nlv;
  const lld_frame_stereo_params& P = *B.prm;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  lld_frame* f = new lld_frame();
  f->ctx = ctx; f->nt = nl; f->has_uright = f->has_angle = f->has_inv_sigma2 = true; f->stereo_built = true;
  std::memset(&f->consts, 0, sizeof(f->consts));
  f->consts.grid_min_x = P.grid_min_x; f->consts.grid_min_y = P.grid_min_y; f->consts.grid_width_inv = P.grid_width_inv; f->consts.grid_height_inv = P.grid_height_inv;
  f->consts.grid_cols = P.grid_cols; f->consts.grid_rows = P.grid_rows; f->consts.n_levels = nlv;
  for (int l = 0; l < kMaxLevels; l++) {
    f->scale[l] = l < nlv ? B.level_scale[l] : 1.f;
    f->sigma2[l] = (l < nlv && B.level_sigma2) ? B.level_sigma2[l] : 1.f;
    f->inv_sigma2[l] = l < nlv ? B.level_inv_sigma2[l] : 1.f;
  }
  f->consts.level_scale = f->scale; f->consts.level_sigma2 = f->sigma2; f->consts.level_inv_sigma2 = f->inv_sigma2;
  f->octave.assign(B.h_loct, B.h_loct + nl);

  // the slab: [u_right | depth | best_r | sad | summary]  [desc | xy | angle | octave]  [right xy | octave | desc]  [pyramid levels]
  // The first block is what lld_frame_stereo_download fetches; the last two exist only for inputs that start on the host.  Whatever is uploaded is
  // one contiguous range ending at the slab's end: from `desc` with host keypoints, from `octave` with device keypoints.
  size_t bytes = 0;
  auto add = [&](size_t b) { const size_t o = bytes; bytes += al64(b); return o; };
  f->o_res = f->o_tur = add((size_t)nl * 4); f->o_depth = add((size_t)nl * 4); f->o_bestr = add((size_t)nl * 4); f->o_sad = add((size_t)nl * 4); f->o_sum = add(16);
  f->res_bytes = bytes;
  f->o_td = add((size_t)nl * 32); f->o_txy = add((size_t)nl * 8); f->o_tang = add((size_t)nl * 4); f->o_toct = add((size_t)nl * 4);
  const bool up_oct = B.loct_dev == nullptr, up_kp = !B.kp_on_device, up_pyr = !B.pyr_on_device && nl > 0;
  size_t o_rxy = 0, o_roct = 0, o_rdesc = 0, o_limg[kMaxLevels] = {}, o_rimg[kMaxLevels] = {};
  if (up_kp) { o_rxy = add((size_t)nr * 8 + 8); o_roct = add((size_t)nr * 4 + 4); o_rdesc = add((size_t)nr * 32 + 32); }
  if (up_pyr) for (int l = 0; l < nlv; l++) { o_limg[l] = add((size_t)B.cols[l] * B.rows[l]); o_rimg[l] = add((size_t)B.cols[l] * B.rows[l]); }
  if (hipMalloc(reinterpret_cast<void**>(&f->d), bytes + 256) != hipSuccess) { delete f; return LLD_ERR_ALLOC; }
  if (nl == 0) { *out = f; return LLD_OK; }                                   // Frame.cc:108: mvKeys.empty() -> return

  const size_t up_from = up_kp ? f->o_td : f->o_toct;
  const size_t up_bytes = (up_kp || up_oct || up_pyr) ? bytes - up_from : 0;
  char* d = f->d;
  if (up_bytes) {
    if (hipHostMalloc(&f->h_stage, up_bytes, hipHostMallocDefault) != hipSuccess) { lld_frame_destroy(f); return LLD_ERR_ALLOC; }
    char* const stage = static_cast<char*>(f->h_stage);
    auto at = [&](size_t slab_offset) { return stage + (slab_offset - up_from); };
    if (up_kp) {
      std::memcpy(at(f->o_td), B.ldesc, (size_t)nl * 32); std::memcpy(at(f->o_txy), B.lxy, (size_t)nl * 8); std::memcpy(at(f->o_tang), B.lang, (size_t)nl * 4);
      if (nr) { std::memcpy(at(o_rxy), B.rxy, (size_t)nr * 8); std::memcpy(at(o_roct), B.roct, (size_t)nr * 4); std::memcpy(at(o_rdesc), B.rdesc, (size_t)nr * 32); }
    }
    if (up_kp || up_oct) std::memcpy(at(f->o_toct), B.h_loct, (size_t)nl * 4);
    if (up_pyr)
      for (int l = 0; l < nlv; l++)                                           // rows are packed tightly whatever the caller's step
        for (int r = 0; r < B.rows[l]; r++) {
          std::memcpy(at(o_limg[l]) + (size_t)r * B.cols[l], B.limg[l] + (size_t)r * B.lstep[l], (size_t)B.cols[l]);
          std::memcpy(at(o_rimg[l]) + (size_t)r * B.cols[l], B.rimg[l] + (size_t)r * B.rstep[l], (size_t)B.cols[l]);
        }
  }

  RowsArgs R; std::memset(&R, 0, sizeof(R));
  R.n_left = nl; R.n_right = nr;
  R.f_desc = reinterpret_cast<uint32_t*>(d + f->o_td); R.f_xy = reinterpret_cast<float*>(d + f->o_txy);
  R.f_angle = reinterpret_cast<float*>(d + f->o_tang); R.f_octave = reinterpret_cast<int32_t*>(d + f->o_toct);
  R.src_desc = up_kp ? R.f_desc : B.ldesc; R.src_xy = up_kp ? R.f_xy : B.lxy; R.src_angle = up_kp ? R.f_angle : B.lang;
  R.src_octave = (up_kp || up_oct) ? R.f_octave : B.loct_dev;
  R.right_xy = up_kp ? reinterpret_cast<const float*>(d + o_rxy) : B.rxy;
  R.right_octave = up_kp ? reinterpret_cast<const int32_t*>(d + o_roct) : B.roct;
  R.right_desc = up_kp ? reinterpret_cast<const uint32_t*>(d + o_rdesc) : B.rdesc;
  for (int l = 0; l < kMaxLevels; l++) R.scale[l] = l < nlv ? B.pyr_scale[l] : 1.f;
  R.min_d = 0.0f; R.max_d = P.mbf / P.mb;                                     // minZ = mb; minD = 0; maxD = mbf / minZ (Frame.cc:558-560)
  R.rows0 = B.rows[0];
  R.best_r = reinterpret_cast<int32_t*>(d + f->o_bestr);

  lld_stereo::RefineArgs A; std::memset(&A, 0, sizeof(A));
  for (int l = 0; l < nlv; l++) {
    A.cols[l] = B.cols[l]; A.rows[l] = B.rows[l]; A.scale[l] = B.pyr_scale[l]; A.inv_scale[l] = B.pyr_inv_scale[l];
    if (up_pyr) {
      A.left_img[l] = reinterpret_cast<const uint8_t*>(d + o_limg[l]); A.right_img[l] = reinterpret_cast<const uint8_t*>(d + o_rimg[l]);
      A.lstep[l] = B.cols[l]; A.rstep[l] = B.cols[l];
    } else { A.left_img[l] = B.limg[l]; A.right_img[l] = B.rimg[l]; A.lstep[l] = B.lstep[l]; A.rstep[l] = B.rstep[l]; }
  }
  A.n_left = nl; A.left_xy = R.f_xy; A.left_octave = R.f_octave; A.right_xy = R.right_xy; A.best_r = R.best_r;
  A.min_d = R.min_d; A.max_d = R.max_d; A.mbf = P.mbf;
  A.u_right = reinterpret_cast<float*>(d + f->o_tur); A.depth = reinterpret_cast<float*>(d + f->o_depth); A.sad = reinterpret_cast<int32_t*>(d + f->o_sad);

  hipStream_t sm = ctx->stream;
  int st = LLD_OK;
  if (up_bytes && hipMemcpyAsync(d + up_from, f->h_stage, up_bytes, hipMemcpyHostToDevice, sm) != hipSuccess) st = LLD_ERR_HIP;
  if (!st) {
    hipLaunchKernelGGL(stereo_rows_kernel, dim3((nl + kBlock / kWave - 1) / (kBlock / kWave)), dim3(kBlock), 0, sm, R);
    st = lld_stereo::refine_launch(sm, A, reinterpret_cast<int32_t*>(d + f->o_sum));
  }
  if (st) { lld_frame_destroy(f); return st; }
  *out = f;
  return LLD_OK;
}

// the refusals both entry points share (before anything is allocated or queued)
int check_params(const lld_frame_stereo_params* P) {
  if (!(P->mb > 0.f)) return LLD_ERR_INVALID;
  if (P->grid_cols <= 0 || P->grid_rows <= 0 || P->grid_cols * P->grid_rows > 8191) return LLD_ERR_INVALID;   // as lld_frame_create
  return LLD_OK;
}

}  // namespace

extern "C" int lld_frame_build_stereo_keypoints(lld_ctx* ctx, const lld_keypoints* left, const lld_keypoints* right, const lld_stereo_pyramids* pyr,
                                                const lld_frame_stereo_params* P, lld_frame** out) {
  if (out) *out = nullptr;
  if (!ctx || !left || !right || !pyr || !P || !out) return LLD_ERR_INVALID;
  const int nl = left->n, nr = right->n, nlv = P->n_levels;
  if (nlv <= 0 || nlv > kMaxLevels || pyr->n_levels != nlv) return LLD_ERR_INVALID;
  if (nl < 0 || nr < 0) return LLD_ERR_INVALID;
  int st = check_params(P); if (st) return st;
  if (!P->level_scale || !P->level_inv_sigma2) return LLD_ERR_INVALID;
  if (nl > LLD_ORB_MAX_KEYPOINTS || nr > LLD_ORB_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  if ((nl > 0 && (!left->xy || !left->octave || !left->desc || !P->left_angle)) || (nr > 0 && (!right->xy || !right->octave || !right->desc))) return LLD_ERR_INVALID;
  if (!pyr->left || !pyr->right || !pyr->cols || !pyr->rows || !pyr->left_step || !pyr->right_step || !pyr->scale_factors || !pyr->inv_scale_factors)
    return LLD_ERR_INVALID;
  for (int l = 0; l < nlv; l++)
    if (!pyr->left[l] || !pyr->right[l] || pyr->cols[l] <= 0 || pyr->rows[l] <= 0 || pyr->left_step[l] < pyr->cols[l] || pyr->right_step[l] < pyr->cols[l])
      return LLD_ERR_INVALID;
  const bool dev = P->keypoints_on_device != 0;
  for (int i = 0; i < nl; i++) if (left->octave[i] < 0 || left->octave[i] >= nlv) return LLD_ERR_INVALID;       // a host array on both routes
  if (!dev) for (int i = 0; i < nr; i++) if (right->octave[i] < 0 || right->octave[i] >= nlv) return LLD_ERR_INVALID;
  BuildIn B;
  B.nl = nl; B.nr = nr; B.nlv = nlv; B.kp_on_device = dev;
  B.lxy = left->xy; B.lang = P->left_angle; B.ldesc = left->desc; B.h_loct = left->octave;
  B.rxy = right->xy; B.roct = right->octave; B.rdesc = right->desc;
  B.pyr_on_device = pyr->on_device != 0;
  for (int l = 0; l < nlv; l++) {
    B.limg[l] = pyr->left[l]; B.rimg[l] = pyr->right[l]; B.cols[l] = pyr->cols[l]; B.rows[l] = pyr->rows[l];
    B.lstep[l] = pyr->left_step[l]; B.rstep[l] = pyr->right_step[l];
  }
  B.pyr_scale = pyr->scale_factors; B.pyr_inv_scale = pyr->inv_scale_factors;
  B.level_scale = P->level_scale; B.level_sigma2 = P->level_sigma2; B.level_inv_sigma2 = P->level_inv_sigma2;
  B.prm = P;
  return build(ctx, B, out);
}

extern "C" int lld_frame_build_stereo(lld_orb_extractor* ex, int left_image, int right_image, const lld_frame_stereo_params* P, lld_frame** out) {
  if (out) *out = nullptr;
  if (!ex || !P || !out || left_image == right_image) return LLD_ERR_INVALID;
  lld_stereo::ExtractedImage L, Rt;
  int st = lld_stereo::extracted_image(ex, left_image, &L); if (st) return st;
  st = lld_stereo::extracted_image(ex, right_image, &Rt); if (st) return st;
  st = check_params(P); if (st) return st;
  const lld_orb_extractor_levels* lv = lld_stereo::extractor_levels(ex);
  const int nlv = lv->n_levels;
  if (L.n < 0 || Rt.n < 0) return LLD_ERR_INVALID;
  if (L.n > LLD_ORB_MAX_KEYPOINTS || Rt.n > LLD_ORB_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  for (int i = 0; i < L.n; i++) if (L.h_octave[i] < 0 || L.h_octave[i] >= nlv) return LLD_ERR_INVALID;
  for (int l = 0; l < nlv; l++) if (L.cols[l] != Rt.cols[l] || L.rows[l] != Rt.rows[l]) return LLD_ERR_INVALID;   // a stereo pair has one size
  BuildIn B;
  B.nl = L.n; B.nr = Rt.n; B.nlv = nlv; B.kp_on_device = true;
  B.lxy = L.d_xy; B.lang = L.d_angle; B.ldesc = L.d_desc; B.loct_dev = L.d_octave; B.h_loct = L.h_octave;
  B.rxy = Rt.d_xy; B.roct = Rt.d_octave; B.rdesc = Rt.d_desc;
  B.pyr_on_device = true;
  for (int l = 0; l < nlv; l++) {
    B.limg[l] = L.level[l]; B.rimg[l] = Rt.level[l]; B.cols[l] = L.cols[l]; B.rows[l] = L.rows[l]; B.lstep[l] = L.step[l]; B.rstep[l] = Rt.step[l];
  }
  B.pyr_scale = lv->scale_factor; B.pyr_inv_scale = lv->inv_scale_factor;
  B.level_scale = lv->scale_factor; B.level_sigma2 = lv->level_sigma2; B.level_inv_sigma2 = lv->inv_level_sigma2;
  B.prm = P;
  return build(lld_stereo::extractor_context(ex), B, out);
}

extern "C" int lld_frame_stereo_download(lld_frame* f, lld_stereo_result* out) {
  if (!f || !out || !f->stereo_built) return LLD_ERR_INVALID;
  const int nl = f->nt;
  out->n_matches = 0;
  if (nl == 0) return LLD_OK;
  if (!out->u_right || !out->depth) return LLD_ERR_INVALID;
  lld_ctx* ctx = f->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  void* hb; int st = lld_ctx_pinned(ctx, f->res_bytes, &hb); if (st) return st;
  const char* const hc = static_cast<const char*>(hb);
  auto at = [&](size_t slab_offset) { return hc + (slab_offset - f->o_res); };
  LLD_HIP_TRY(hipMemcpyAsync(hb, f->d + f->o_res, f->res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LLD_HIP_TRY(hipStreamSynchronize(ctx->stream));
  std::memcpy(out->u_right, at(f->o_tur), (size_t)nl * 4); std::memcpy(out->depth, at(f->o_depth), (size_t)nl * 4);
  if (out->best_r) std::memcpy(out->best_r, at(f->o_bestr), (size_t)nl * 4);
  if (out->sad) std::memcpy(out->sad, at(f->o_sad), (size_t)nl * 4);
  out->n_matches = reinterpret_cast<const int32_t*>(at(f->o_sum))[0];
  return LLD_OK;
}
