// lld_frame_track_bow.hip — ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (src/ORBmatcher.cc:159-288) as a stage of the
// device-resident Tracking chain (lld_frame_track_reference_keyframe, lld_frame_track.hip).  The node merge and the rotation histogram are
// the device bodies of lld_bow_merge.h (shared with Tracking::Relocalization's batched search, lld_frame_reloc.hip):
//
//   bow_match_kernel     one wavefront per keyframe node (bow_match_node)
//   bow_finish_kernel    one workgroup after all nodes (bow_finish_block): mCurrentFrame.mvpMapPoints = vpMapPointMatches
//                        (src/Tracking.cc:788) written straight into the chain's tables.
#include "lld_common.h"
#include "lld_bow_merge.h"
#include "lld_track_internal.h"

namespace {

using namespace lld_track;
using namespace lld_bow_merge;

__global__ __launch_bounds__(kMatchWaves * 64) void bow_match_kernel(BowSearchDev B) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * kMatchWaves + (threadIdx.x >> 6);
  if (w >= B.n_kf_nodes) return;                 // whole wavefronts leave; nothing below synchronises the workgroup
  bow_match_node(B, w, lane);
}

__global__ __launch_bounds__(kFinishThreads) void bow_finish_kernel(BowSearchDev B, ApplyDev A) {
  __shared__ int hist[kHisto];
  __shared__ int ctl[4];
  bow_finish_block(B, A, hist, ctl);
}

}  // namespace

namespace lld_track {

int bow_search_launch(hipStream_t st, const BowSearchDev& in, const ApplyDev& ap) {
  if (in.nt < 0 || in.nt > LLD_ORB_MAX_KEYPOINTS) return LLD_ERR_INVALID;
  if (in.nt > 0) LLD_HIP_TRY(hipMemsetAsync(in.taken, 0xff, (size_t)in.nt * 4, st));
  if (in.nt > 0 && in.n_kf_nodes > 0)
    hipLaunchKernelGGL(bow_match_kernel, dim3((in.n_kf_nodes + kMatchWaves - 1) / kMatchWaves), dim3(kMatchWaves * 64), 0, st, in);
  hipLaunchKernelGGL(bow_finish_kernel, dim3(1), dim3(kFinishThreads), 0, st, in, ap);
  LLD_HIP_TRY(hipGetLastError());
  return LLD_OK;
}

}  // namespace lld_track
