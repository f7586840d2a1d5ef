// local_map_harness.h — what local_map_harness.cpp read from its two files, handed to the object mode (local_map_objects.cpp).
#ifndef LLD_LOCAL_MAP_HARNESS_H
#define LLD_LOCAL_MAP_HARNESS_H

#include <cstdint>
#include <vector>

#include "lld_amd.hpp"

struct HarnessInput {
  int nt, nl, nr, dim, n_levels;
  const float* fc;                                  // min_x min_y max_x max_y grid_width_inv grid_height_inv
  const double* dc;                                 // fx fy cx cy bf gamma line_thr_base md_thr
  const std::vector<float>*scale, *inv_sigma2, *t_xy, *t_ur, *t_ang, *ln_left, *ln_right, *ln_desc;
  const std::vector<uint32_t>* t_desc;
  const std::vector<int32_t>*t_oct, *ln_lo, *ln_ro, *ln_lm;
  float log_scale_factor;
  // what stage 1 left in the frame (a TrackedFrame ran it): ids after the discard, the pose
  std::vector<int32_t> kp_id, ln_id; float Tcw[16];
  // the map file
  lld_map_limits L;
  const lld_amd::DeviceMap::KeyFrameRows* K;        // order_key is not used by the object mode: pointers order the keyframes there
  const std::vector<uint8_t>*pt_state, *ln_bad;
  const std::vector<int32_t>*obs_start, *obs;
  const std::vector<float>*p_pos, *p_nrm, *p_mind, *p_maxd, *l_desc;
  const std::vector<uint32_t>* p_desc;
  const std::vector<double>*l_x0, *l_dir, *l_x1, *l_x2;
};

// FrameOnDevice::TrackLocalMap(.., MapOnDevice&, ..) against host UpdateLocalMap (local_map_host.cpp on tables gathered from the objects) + the
// existing FrameOnDevice::TrackLocalMap, on two copies of one object graph; once after Upload, once after UpdatePoints / UpdateKeyFrames on
// a changed map.  Writes both graphs' dumps; returns 0 when they are equal, 3 when they differ.
int run_objects(lld_amd::Context& ctx, const HarnessInput& in, const char* out_path);

#endif
