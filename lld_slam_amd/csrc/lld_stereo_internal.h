// lld_stereo_internal.h — what lld_stereo.hip (lld_compute_stereo_matches), lld_orb_extract.hip and lld_frame_build.hip share: the launcher of the
// SAD refinement + median cut of Frame::ComputeStereoMatches (src/Frame.cc:615-703) on DEVICE arrays, and a read-only view of what the last
// lld_orb_extract left in HBM.  Nothing here is exported (-fvisibility=hidden).
#ifndef LLD_STEREO_INTERNAL_H
#define LLD_STEREO_INTERNAL_H

#include "lld_common.h"

namespace lld_stereo {

// Every pointer is a device pointer.  best_r [n_left] is the Hamming stage's bestIdxR (-1: none); u_right, depth and sad [n_left] are written for
// every left keypoint.
struct RefineArgs {
  int n_left;
  const float* left_xy; const int32_t* left_octave; const float* right_xy; const int32_t* best_r;
  const uint8_t* left_img[LLD_ORB_MAX_LEVELS]; const uint8_t* right_img[LLD_ORB_MAX_LEVELS];
  int cols[LLD_ORB_MAX_LEVELS], rows[LLD_ORB_MAX_LEVELS], lstep[LLD_ORB_MAX_LEVELS], rstep[LLD_ORB_MAX_LEVELS];
  float scale[LLD_ORB_MAX_LEVELS], inv_scale[LLD_ORB_MAX_LEVELS];
  float min_d, max_d, mbf;
  float* u_right; float* depth; int32_t* sad;
};

// Queues stereo_refine_kernel and stereo_median_kernel on `st` (n_left > 0).  summary [2] (device): entries that survive the median cut, the median.
int refine_launch(hipStream_t st, const RefineArgs& A, int32_t* summary);

// Image `image` of the extractor's last successful lld_orb_extract: device arrays of its n keypoints (valid until the next extract on the handle),
// the host copy of the octaves that call brought back, and the pyramid levels.
struct ExtractedImage {
  int n;
  const float* d_xy; const int32_t* d_octave; const float* d_angle; const uint32_t* d_desc;
  const int32_t* h_octave;
  const uint8_t* level[LLD_ORB_MAX_LEVELS];
  int cols[LLD_ORB_MAX_LEVELS], rows[LLD_ORB_MAX_LEVELS], step[LLD_ORB_MAX_LEVELS];
};
// LLD_ERR_INVALID when the handle has no successful extract yet or `image` is outside its n_images.
int extracted_image(const lld_orb_extractor* ex, int image, ExtractedImage* out);
lld_ctx* extractor_context(const lld_orb_extractor* ex);
const lld_orb_extractor_levels* extractor_levels(const lld_orb_extractor* ex);

}  // namespace lld_stereo

#endif
