// lld_frame_mono.hip — the RGB-D and the monocular Frame built on the device (lld_frame_build_mono*, include/lld_amd.h): what Frame::Frame does
// between ExtractORB and the Tracking chain for these two sensors (src/Frame.cc:163-215, :220-292) without a trip through the host:
// UndistortKeyPoints (:468-498, the restated cv::undistortPoints) and ComputeStereoFromRGBD (:707-728), or mvuRight = mvDepth = -1.
//   ONE launch, a lane per keypoint: every keypoint is independent, so there is no atomic, no LDS and no second kernel.  The lane reads its
//   keypoint where it lives (the extractor's buffers, caller device pointers or the frame's own uploaded slab), moves octave, angle and
//   descriptor into the frame's slab when the source differs, samples the depth image at the DISTORTED position, undistorts in double with
//   every operation rounded separately, and writes mvKeysUn, mvuRight and mvDepth.
// At most one host-to-device copy, no synchronisation: the call returns with the kernel queued on the context's stream, and the frame owns
// every byte the queued work and the later chain read, except a device depth image, which the caller keeps until the work has run.
#include <cmath>

#include "lld_stereo_internal.h"
#include "lld_track_internal.h"

namespace {

constexpr int kMaxLevels = LLD_ORB_MAX_LEVELS;
constexpr int kBlock = 64;                           // one wavefront per block: 1000 keypoints spread over 16 CUs, and the double divisions of a lane are a latency chain
constexpr int kUndistortIterations = 5;              // cvUndistortPoints: "compensate distortion iteratively", a fixed count
constexpr int kMaxDepthSide = 16383;

struct Camera { float fx, fy, cx, cy, k1, k2, p1, p2, k3; int undistort; };

// cv::undistortPoints(src, dst, K, dist, cv::Mat(), K) on one point, as include/lld_amd.h restates it.  The same text serves the kernel and
// lld_frame_image_bounds on the host; contraction is off, so no multiply-add pair is fused on either side and both round as numpy does.
__host__ __device__ inline void undistort_point(const Camera& C, float u, float v, float* u_un, float* v_un) {
#pragma clang fp contract(off)
  if (!C.undistort) { *u_un = u; *v_un = v; return; }                           // mDistCoef.at<float>(0)==0.0 -> mvKeysUn = mvKeys (Frame.cc:470-474)
  const double fx = C.fx, fy = C.fy, cx = C.cx, cy = C.cy, k1 = C.k1, k2 = C.k2, p1 = C.p1, p2 = C.p2, k3 = C.k3;
  const double ifx = 1.0 / fx, ify = 1.0 / fy;
  const double x0 = ((double)u - cx) * ifx, y0 = ((double)v - cy) * ify;
  double x = x0, y = y0;
  for (int it = 0; it < kUndistortIterations; it++) {
    const double r2 = x * x + y * y;
    const double icdist = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
    const double dx = ((2.0 * p1) * x) * y + p2 * (r2 + (2.0 * x) * x);
    const double dy = p1 * (r2 + (2.0 * y) * y) + ((2.0 * p2) * x) * y;
    x = (x0 - dx) * icdist;
    y = (y0 - dy) * icdist;
  }
  *u_un = (float)(fx * x + cx);
  *v_un = (float)(fy * y + cy);
}

struct MonoArgs {
  int n;
  // where the keypoints are read, and the frame's own arrays; a pair that differs is copied
  const float* src_xy; const int32_t* src_octave; const float* src_angle; const uint32_t* src_desc;
  float* f_xy; int32_t* f_octave; float* f_angle; uint32_t* f_desc;
  Camera cam;
  const char* depth;                         // NULL: the monocular frame
  int d_cols, d_rows, d_step, d_type;        // d_step in bytes
  float factor; int scale_f32;               // scale_f32: fabsf(factor - 1.0f) > 1e-5f, decided once on the host (Tracking.cc:252)
  float mbf;
  float* u_right; float* depth_out;
};

__global__ __launch_bounds__(kBlock) void frame_mono_kernel(MonoArgs A) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= A.n) return;
  const float u = A.src_xy[2 * i], v = A.src_xy[2 * i + 1];                   // read before f_xy[i] is written: the two may be one array
  if (A.src_desc != A.f_desc) {
#pragma unroll
    for (int w = 0; w < 8; w++) A.f_desc[8 * i + w] = A.src_desc[8 * i + w];
  }
  if (A.src_octave != A.f_octave) A.f_octave[i] = A.src_octave[i];
  if (A.src_angle != A.f_angle) A.f_angle[i] = A.src_angle[i];

  float u_un, v_un;
  undistort_point(A.cam, u, v, &u_un, &v_un);
  A.f_xy[2 * i] = u_un; A.f_xy[2 * i + 1] = v_un;

  float ur = -1.0f, dep = -1.0f;                                              // mvuRight / mvDepth = vector<float>(N,-1) (Frame.cc:709-710, :255-256)
  // imDepth.at<float>(v,u) is unchecked in the reference; here nothing outside the image is read (a NaN fails every comparison)
  if (A.depth && u > -1.0f && u < (float)A.d_cols && v > -1.0f && v < (float)A.d_rows) {
    const int col = (int)u, row = (int)v;                                     // truncation toward zero: (-1, 0) -> 0
    const char* const p = A.depth + (size_t)row * (size_t)A.d_step;
    float d;
    if (A.d_type == LLD_DEPTH_U16) d = __fmul_rn((float)reinterpret_cast<const uint16_t*>(p)[col], A.factor);
    else { d = reinterpret_cast<const float*>(p)[col]; if (A.scale_f32) d = __fmul_rn(d, A.factor); }
    if (d > 0.0f) { dep = d; ur = __fsub_rn(u_un, __fdiv_rn(A.mbf, d)); }     // Frame.cc:722-726
  }
  A.u_right[i] = ur; A.depth_out[i] = dep;
}

inline size_t al64(size_t b) { return (b + 63) & ~size_t(63); }
inline int depth_elem(int type) { return type == LLD_DEPTH_U16 ? 2 : 4; }

int check_camera(float fx, float fy, float cx, float cy, const float* dist, int n_dist, Camera* C) {
  if (!dist || !(fx > 0.f) || !(fy > 0.f) || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy)) return LLD_ERR_INVALID;
  if (n_dist != 4 && n_dist != 5) return LLD_ERR_INVALID;
  for (int k = 0; k < n_dist; k++) if (!std::isfinite(dist[k])) return LLD_ERR_INVALID;
  *C = Camera{fx, fy, cx, cy, dist[0], dist[1], dist[2], dist[3], n_dist == 5 ? dist[4] : 0.f, dist[0] != 0.0f};
  return LLD_OK;
}

// the refusals both entry points share (before anything is allocated or queued)
int check_params(const lld_frame_mono_params* P, const lld_depth_image* D, Camera* C) {
  int st = check_camera(P->fx, P->fy, P->cx, P->cy, P->dist, P->n_dist, C); if (st) return st;
  if (!std::isfinite(P->mbf)) return LLD_ERR_INVALID;
  if (P->grid_cols <= 0 || P->grid_rows <= 0 || P->grid_cols * P->grid_rows > 8191) return LLD_ERR_INVALID;   // as lld_frame_create
  if (D) {
    if (!D->data || (D->type != LLD_DEPTH_F32 && D->type != LLD_DEPTH_U16) || !std::isfinite(D->factor)) return LLD_ERR_INVALID;
    if (D->cols < 1 || D->cols > kMaxDepthSide || D->rows < 1 || D->rows > kMaxDepthSide) return LLD_ERR_INVALID;
    const int es = depth_elem(D->type);
    if (D->step < D->cols * es || D->step % es != 0) return LLD_ERR_INVALID;
  }
  return LLD_OK;
}

// One build, wherever its inputs live.  Device pointers unless named h_*.
struct BuildIn {
  int n = 0, nlv = 0;
  bool kp_on_device = false;                 // xy / angle / desc are device pointers, read in place
  const float* xy = nullptr; const float* angle = nullptr; const uint32_t* desc = nullptr;
  const int32_t* oct_dev = nullptr;          // device octaves to read in place, or NULL: h_oct is uploaded
  const int32_t* h_oct = nullptr;            // host, always: the frame's host copy, and the upload when oct_dev is NULL
  const float* level_scale = nullptr; const float* level_sigma2 = nullptr; const float* level_inv_sigma2 = nullptr;   // [nlv] host
  const lld_frame_mono_params* prm = nullptr;
  const lld_depth_image* depth = nullptr;
  Camera cam;
};

int build(lld_ctx* ctx, const BuildIn& B, lld_frame** out) {
  const int n = B.n, nlv = B.nlv;
  const lld_frame_mono_params& P = *B.prm;
  const lld_depth_image* D = B.depth;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  lld_frame* f = new lld_frame();
  f->ctx = ctx; f->nt = n; f->has_uright = f->has_angle = f->has_inv_sigma2 = true; f->mono_built = true;
  std::memset(&f->consts, 0, sizeof(f->consts));
  f->consts.grid_min_x = P.grid_min_x; f->consts.grid_min_y = P.grid_min_y; f->consts.grid_width_inv = P.grid_width_inv; f->consts.grid_height_inv = P.grid_height_inv;
  f->consts.grid_cols = P.grid_cols; f->consts.grid_rows = P.grid_rows; f->consts.n_levels = nlv;
  for (int l = 0; l < kMaxLevels; l++) {
    f->scale[l] = l < nlv ? B.level_scale[l] : 1.f;
    f->sigma2[l] = (l < nlv && B.level_sigma2) ? B.level_sigma2[l] : 1.f;
    f->inv_sigma2[l] = l < nlv ? B.level_inv_sigma2[l] : 1.f;
  }
  f->consts.level_scale = f->scale; f->consts.level_sigma2 = f->sigma2; f->consts.level_inv_sigma2 = f->inv_sigma2;
  f->octave.assign(B.h_oct, B.h_oct + n);

  // the slab: [u_right | depth | xy]  [desc | angle | octave]  [depth image]
  // The first block is what lld_frame_keypoints_download fetches; the depth image exists only when it starts on the host.  Whatever is uploaded
  // is one contiguous range ending at the slab's end: from `xy` with host keypoints (the kernel then undistorts xy in place), from `octave` with
  // device keypoints whose octaves are not on the device, from the image when only that is on the host.
  size_t bytes = 0;
  auto add = [&](size_t b) { const size_t o = bytes; bytes += al64(b); return o; };
  f->o_res = f->o_tur = add((size_t)n * 4); f->o_depth = add((size_t)n * 4); f->o_txy = add((size_t)n * 8);
  f->res_bytes = bytes;
  f->o_td = add((size_t)n * 32); f->o_tang = add((size_t)n * 4); f->o_toct = add((size_t)n * 4);
  const bool up_kp = !B.kp_on_device && n > 0, up_oct = !up_kp && B.oct_dev == nullptr && n > 0, up_img = D && !D->on_device && n > 0;
  const size_t row_bytes = D ? (size_t)D->cols * depth_elem(D->type) : 0;
  const size_t o_img = up_img ? add(row_bytes * D->rows) : 0;
  if (hipMalloc(reinterpret_cast<void**>(&f->d), bytes + 256) != hipSuccess) { delete f; return LLD_ERR_ALLOC; }
  if (n == 0) { *out = f; return LLD_OK; }                                    // Frame.cc:184-185: mvKeys.empty() -> return

  const size_t up_from = up_kp ? f->o_txy : up_oct ? f->o_toct : o_img;
  const size_t up_bytes = (up_kp || up_oct || up_img) ? bytes - up_from : 0;
  char* d = f->d;
  if (up_bytes) {
    if (hipHostMalloc(&f->h_stage, up_bytes, hipHostMallocDefault) != hipSuccess) { lld_frame_destroy(f); return LLD_ERR_ALLOC; }
    char* const stage = static_cast<char*>(f->h_stage);
    auto at = [&](size_t slab_offset) { return stage + (slab_offset - up_from); };
    if (up_kp) {
      std::memcpy(at(f->o_txy), B.xy, (size_t)n * 8); std::memcpy(at(f->o_td), B.desc, (size_t)n * 32); std::memcpy(at(f->o_tang), B.angle, (size_t)n * 4);
    }
    if (up_kp || up_oct) std::memcpy(at(f->o_toct), B.h_oct, (size_t)n * 4);
    if (up_img)                                                               // rows are packed tightly whatever the caller's step
      for (int r = 0; r < D->rows; r++) std::memcpy(at(o_img) + (size_t)r * row_bytes, static_cast<const char*>(D->data) + (size_t)r * D->step, row_bytes);
  }

  MonoArgs A; std::memset(&A, 0, sizeof(A));
  A.n = n;
  A.f_desc = reinterpret_cast<uint32_t*>(d + f->o_td); A.f_xy = reinterpret_cast<float*>(d + f->o_txy);
  A.f_angle = reinterpret_cast<float*>(d + f->o_tang); A.f_octave = reinterpret_cast<int32_t*>(d + f->o_toct);
  A.src_desc = up_kp ? A.f_desc : B.desc; A.src_xy = up_kp ? A.f_xy : B.xy; A.src_angle = up_kp ? A.f_angle : B.angle;
  A.src_octave = (up_kp || up_oct) ? A.f_octave : B.oct_dev;
  A.cam = B.cam;
  if (D) {
    A.depth = up_img ? d + o_img : static_cast<const char*>(D->data);
    A.d_cols = D->cols; A.d_rows = D->rows; A.d_step = up_img ? (int)row_bytes : D->step; A.d_type = D->type;
    A.factor = D->factor; A.scale_f32 = std::fabs(D->factor - 1.0f) > 1e-5f;
  }
  A.mbf = P.mbf;
  A.u_right = reinterpret_cast<float*>(d + f->o_tur); A.depth_out = reinterpret_cast<float*>(d + f->o_depth);

  hipStream_t sm = ctx->stream;
  int st = LLD_OK;
  if (up_bytes && hipMemcpyAsync(d + up_from, f->h_stage, up_bytes, hipMemcpyHostToDevice, sm) != hipSuccess) st = LLD_ERR_HIP;
  if (!st) {
    hipLaunchKernelGGL(frame_mono_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, sm, A);
    if (hipGetLastError() != hipSuccess) st = LLD_ERR_HIP;
  }
  if (st) { lld_frame_destroy(f); return st; }
  *out = f;
  return LLD_OK;
}

}  // namespace

extern "C" int lld_frame_build_mono_keypoints(lld_ctx* ctx, const lld_keypoints* kp, const lld_depth_image* D, const lld_frame_mono_params* P, lld_frame** out) {
  if (out) *out = nullptr;
  if (!ctx || !kp || !P || !out) return LLD_ERR_INVALID;
  const int n = kp->n, nlv = P->n_levels;
  if (nlv <= 0 || nlv > kMaxLevels || n < 0) return LLD_ERR_INVALID;
  BuildIn B;
  int st = check_params(P, D, &B.cam); if (st) return st;
  if (!P->level_scale || !P->level_inv_sigma2) return LLD_ERR_INVALID;
  if (n > LLD_ORB_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  if (n > 0 && (!kp->xy || !kp->octave || !kp->desc || !P->left_angle)) return LLD_ERR_INVALID;
  for (int i = 0; i < n; i++) if (kp->octave[i] < 0 || kp->octave[i] >= nlv) return LLD_ERR_INVALID;               // a host array on both routes
  B.n = n; B.nlv = nlv; B.kp_on_device = P->keypoints_on_device != 0;
  B.xy = kp->xy; B.angle = P->left_angle; B.desc = kp->desc; B.h_oct = kp->octave;
  B.level_scale = P->level_scale; B.level_sigma2 = P->level_sigma2; B.level_inv_sigma2 = P->level_inv_sigma2;
  B.prm = P; B.depth = D;
  return build(ctx, B, out);
}

extern "C" int lld_frame_build_mono(lld_orb_extractor* ex, int image, const lld_depth_image* D, const lld_frame_mono_params* P, lld_frame** out) {
  if (out) *out = nullptr;
  if (!ex || !P || !out) return LLD_ERR_INVALID;
  lld_stereo::ExtractedImage E;
  int st = lld_stereo::extracted_image(ex, image, &E); if (st) return st;
  BuildIn B;
  st = check_params(P, D, &B.cam); if (st) return st;
  const lld_orb_extractor_levels* lv = lld_stereo::extractor_levels(ex);
  const int nlv = lv->n_levels;
  if (E.n < 0) return LLD_ERR_INVALID;
  if (E.n > LLD_ORB_MAX_KEYPOINTS) return LLD_ERR_UNSUPPORTED;
  for (int i = 0; i < E.n; i++) if (E.h_octave[i] < 0 || E.h_octave[i] >= nlv) return LLD_ERR_INVALID;
  B.n = E.n; B.nlv = nlv; B.kp_on_device = true;
  B.xy = E.d_xy; B.angle = E.d_angle; B.desc = E.d_desc; B.oct_dev = E.d_octave; B.h_oct = E.h_octave;
  B.level_scale = lv->scale_factor; B.level_sigma2 = lv->level_sigma2; B.level_inv_sigma2 = lv->inv_level_sigma2;
  B.prm = P; B.depth = D;
  return build(lld_stereo::extractor_context(ex), B, out);
}

extern "C" int lld_frame_keypoints_download(lld_frame* f, float* xy_un, float* u_right, float* depth) {
  if (!f || !f->mono_built) return LLD_ERR_INVALID;
  const int n = f->nt;
  if (n == 0) return LLD_OK;
  lld_ctx* ctx = f->ctx;
  LLD_HIP_TRY(hipSetDevice(ctx->device));
  void* hb; int st = lld_ctx_pinned(ctx, f->res_bytes, &hb); if (st) return st;
  const char* const hc = static_cast<const char*>(hb);
  auto at = [&](size_t slab_offset) { return hc + (slab_offset - f->o_res); };
  LLD_HIP_TRY(hipMemcpyAsync(hb, f->d + f->o_res, f->res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LLD_HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (xy_un) std::memcpy(xy_un, at(f->o_txy), (size_t)n * 8);
  if (u_right) std::memcpy(u_right, at(f->o_tur), (size_t)n * 4);
  if (depth) std::memcpy(depth, at(f->o_depth), (size_t)n * 4);
  return LLD_OK;
}

extern "C" int lld_frame_image_bounds(int32_t cols, int32_t rows, float fx, float fy, float cx, float cy, const float* dist, int32_t n_dist, float bounds[4]) {
  Camera C;
  if (!bounds || cols <= 0 || rows <= 0) return LLD_ERR_INVALID;
  int st = check_camera(fx, fy, cx, cy, dist, n_dist, &C); if (st) return st;
  if (!C.undistort) { bounds[0] = 0.0f; bounds[1] = (float)cols; bounds[2] = 0.0f; bounds[3] = (float)rows; return LLD_OK; }   // Frame.cc:521-527
  const float cu[4] = {0.0f, (float)cols, 0.0f, (float)cols}, cv[4] = {0.0f, 0.0f, (float)rows, (float)rows};                  // :505-508
  float x[4], y[4];
  for (int k = 0; k < 4; k++) undistort_point(C, cu[k], cv[k], &x[k], &y[k]);
  bounds[0] = std::min(x[0], x[2]); bounds[1] = std::max(x[1], x[3]);                                                          // :515-518
  bounds[2] = std::min(y[0], y[1]); bounds[3] = std::max(y[2], y[3]);
  return LLD_OK;
}
