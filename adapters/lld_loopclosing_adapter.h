// lld_loopclosing_adapter.h — host adapter for the three places where the loop-closing thread moves the map, on live SLAM objects:
//   CorrectLoopPoses         LoopClosing::CorrectLoop                      src/LoopClosing.cc:440-518   (lld_loop_correct)
//   ApplyEssentialGraph      the write-back of OptimizeEssentialGraph      src/Optimizer.cc:1601-1653   (lld_essential_graph_apply)
//   UpdateMapAfterGlobalBA   LoopClosing::RunGlobalBundleAdjustment        src/LoopClosing.cc:678-739   (lld_global_ba_apply)
// Each gathers the objects into flat tables (keyframes numbered in pointer order, observations in std::map order), makes ONE device
// call and scatters the result into the members the reference writes.  The caller holds Map::mMutexMapUpdate around each, as the
// reference does.  Same object model switch as lld_optimizer_adapter.h (LLD_ADAPTER_OBJECTS_HEADER).
#ifndef LLD_LOOPCLOSING_ADAPTER_H
#define LLD_LOOPCLOSING_ADAPTER_H

#include <map>
#include <vector>

#include "../include/lld_amd.hpp"

#ifndef LLD_ADAPTER_OBJECTS_HEADER
#define LLD_ADAPTER_OBJECTS_HEADER "lld_slam_objects.h"
#endif
#include LLD_ADAPTER_OBJECTS_HEADER

namespace lld_adapter {

using lld_slam::KeyFrame;
using lld_slam::Map;
using lld_slam::MapPoint;
using lld_slam::Sim3;

// LoopClosing.h: typedef map<KeyFrame*, g2o::Sim3, std::less<KeyFrame*>, ...> KeyFrameAndPose
typedef std::map<KeyFrame*, Sim3> KeyFrameAndPose;

// Replaces :440-518.  mvpCurrentConnectedKFs holds mpCurrentKF (pushed at :438).  Fills CorrectedSim3 / NonCorrectedSim3, and writes per
// corrected point SetWorldPos, mnCorrectedByKF, mnCorrectedReference, mNormalVector, mfMinDistance, mfMaxDistance, and per connected
// keyframe SetPose plus Ow (the doubles' SetPose does not derive it).  pKFi->UpdateConnections() (:517) stays the batched
// lld_adapter::UpdateConnections call after this one.  scw_f32 (optional): toCvMat(CorrectedSiw) per keyframe of CorrectedSim3, in its
// iteration order, 12 floats each - what SearchAndFuse takes.  Returns the number of points corrected.
int CorrectLoopPoses(const lld_amd::Context& ctx, KeyFrame* mpCurrentKF, const Sim3& mg2oScw, const std::vector<KeyFrame*>& mvpCurrentConnectedKFs,
                     KeyFrameAndPose& CorrectedSim3, KeyFrameAndPose& NonCorrectedSim3, std::vector<float>* scw_f32 = nullptr);

// Replaces Optimizer.cc:1601-1653.  vScw: the Sim3 every keyframe of the map entered the optimisation with; vCorrectedSiw: the
// optimised ones (both for every keyframe of pMap->GetAllKeyFrames()).  Writes SetPose plus Ow of every keyframe, and SetWorldPos, normal
// and depth of every point of pMap->GetAllMapPoints() that is not bad.  Returns the number of points corrected, or -1 with nothing
// called and nothing written when a keyframe of the map, or one that a live point observes or refers to, is missing from either table
// (the reference optimises every keyframe of the map; the centre of one that was no vertex would be unknown).
int ApplyEssentialGraph(const lld_amd::Context& ctx, Map* pMap, KeyFrame* pCurKF, const KeyFrameAndPose& vScw, const KeyFrameAndPose& vCorrectedSiw);

// Replaces :678-739.  Writes mTcwGBA and mnBAGlobalForKF of the keyframes the walk composes, mTcwBefGBA, SetPose and Ow of every
// visited keyframe, and SetWorldPos of the points.  Returns the number of points moved.
int UpdateMapAfterGlobalBA(const lld_amd::Context& ctx, Map* pMap, unsigned long nLoopKF);

}  // namespace lld_adapter
#endif
