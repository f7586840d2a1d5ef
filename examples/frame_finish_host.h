// frame_finish_host.h — see frame_finish_host.cpp
#ifndef FRAME_FINISH_HOST_H
#define FRAME_FINISH_HOST_H

#include "../include/lld_amd.h"

// The frame's state (kp_id: -1 = no MapPoint; kp_obs: Observations() > 0; kp_outlier: mvbOutlier; kp_world [nt][3]) is read and left as
// mCurrentFrame holds it when Track() returns.  p->n_matches_inliers is taken as given; p->depth and p->sensor_rgbd are not read (the state
// handed in is the frame's).  out: every array of lld_frame_finish_result must be bound.
extern "C" void frame_finish_host_tail(int nt, const float* mvDepth, const float* mvKeysUn_xy, const lld_frame_view* view, const lld_frame_finish_params* p,
                                       int32_t* kp_id, uint8_t* kp_obs, uint8_t* kp_outlier, float* kp_world, lld_frame_finish_result* out);

// What the host holds of the frame after TrackLocalMap, from the stage-2 record and its own MapPoints (see the .cpp).
extern "C" void frame_finish_host_state(int nt, const int32_t* rec_kp_point_id, const uint8_t* rec_kp_outlier, const float* world_of, const uint8_t* obs_of,
                                        int32_t* kp_id, uint8_t* kp_obs, uint8_t* kp_outlier, float* kp_world);

#endif
