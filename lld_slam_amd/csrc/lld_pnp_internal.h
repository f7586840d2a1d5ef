// lld_pnp_internal.h — the seam of lld_pnp.hip that Tracking::Relocalization's device-resident stage uses (lld_frame_reloc.hip): a batch of
// PnPsolvers over a correspondence slab that a KERNEL fills, iterate() under a device `live` mask, and the device addresses of the solvers'
// outputs.  Nothing here is exported.
#ifndef LLD_PNP_INTERNAL_H
#define LLD_PNP_INTERNAL_H

#include "lld_common.h"

namespace lld_pnp {

struct PnpRes {                              // the last iterate()'s outputs of one solver (device)
  float tcw[12];
  int32_t has_pose, n_inliers, no_more, iterations, best_inliers, pad[3];
};

// What the PnPsolver constructor (src/PnPsolver.cc:66-110) leaves per correspondence; solver s owns [off[s], off[s] + n[s]).
struct SlabDev { float4* pt; /* X, Y, Z, mvMaxError = sigma2 * th2 (float) */ float2* uv; int32_t* kp; };

// lld_pnp_batch_create without the upload of the correspondences: n solvers of n_corr[s] correspondences each over n_keypoints keypoints,
// SetRansacParameters computed on the host exactly as lld_pnp_batch_create computes it, the streams seeded.  The caller queues the kernel
// that fills `slab` on the context's stream before the first iterate.  off[s]: first correspondence of solver s (host, n entries).
int batch_create_dev(lld_ctx* ctx, int32_t n, const int32_t* n_corr, int32_t n_keypoints, float fx, float fy, float cx, float cy, const uint32_t* seed,
                     const lld_pnp_params* params, lld_pnp_batch** out, SlabDev* slab, int32_t* off);
// iterate(n_iterations) on every solver with live[s] != 0 (device memory, read when the kernels run).  The host lays out hypothesis slots
// for all solvers; a solver with live[s] = 0 keeps its state and last results, as an inactive one does.
int batch_iterate_live(lld_pnp_batch* b, int32_t n_iterations, const uint8_t* live_d);
const PnpRes* batch_results_dev(const lld_pnp_batch* b);                   // [n]
const uint8_t* batch_flags_dev(const lld_pnp_batch* b, int32_t solver);    // vbInliers of `solver`, [n_keypoints]

}  // namespace lld_pnp

#endif
