// lld_covisibility_adapter.h — host adapter for the covisibility counting on live SLAM objects:
//   KeyFrame::UpdateConnections()       src/KeyFrame.cc:312-402
//   LocalMapping::KeyFrameCulling()     src/LocalMapping.cc:633-697
// Both gather the observation table in std::map order, number the keyframes by std::less<KeyFrame*> (the order in which the
// reference's maps iterate, which decides every tie), make one device call (lld_covisibility, include/lld_amd.h) for all their
// keyframes and apply the results as the reference does.  Same object model switch as lld_optimizer_adapter.h
// (LLD_ADAPTER_OBJECTS_HEADER).
#ifndef LLD_COVISIBILITY_ADAPTER_H
#define LLD_COVISIBILITY_ADAPTER_H

#include <vector>

#include "../include/lld_amd.hpp"

#ifndef LLD_ADAPTER_OBJECTS_HEADER
#define LLD_ADAPTER_OBJECTS_HEADER "lld_slam_objects.h"
#endif
#include LLD_ADAPTER_OBJECTS_HEADER

namespace lld_adapter {

using lld_slam::KeyFrame;
using lld_slam::MapPoint;

// pKF->UpdateConnections() for every keyframe of the list, in list order, with ONE device call.  The counts read only the
// observations, which no UpdateConnections changes, so this equals the per-object calls: AddConnection on each listed neighbour
// (their UpdateBestCovisibles re-sort stays on the host), mConnectedKeyFrameWeights, the two ordered vectors, and on the first
// connection the parent and AddChild.  A nullptr entry is skipped.  Returns the number of keyframes the rule wrote (a keyframe
// with an empty counter returns early, :346-347).  phase_ms, when given, receives the upload / kernel / download times.
int UpdateConnections(const lld_amd::Context& ctx, const std::vector<KeyFrame*>& vpKFs, float* phase_ms = nullptr);

// LocalMapping::KeyFrameCulling for pCurrentKF: one device call for all of GetVectorCovisibleKeyFrames(), walked in order.
// SetBadFlag erases observations, so after each keyframe it flags the adapter calls again for the keyframes that remain.
// Returns the flagged keyframes in order; n_calls, when given, receives the number of device calls.
std::vector<KeyFrame*> KeyFrameCulling(const lld_amd::Context& ctx, KeyFrame* pCurrentKF, bool bMonocular, int* n_calls = nullptr,
                                       float* phase_ms = nullptr);

}  // namespace lld_adapter
#endif
