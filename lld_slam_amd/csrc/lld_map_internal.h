// lld_map_internal.h — what lld_frame_track.hip needs of the resident map (lld_map.hip) to run stage 2 from it: the limits that size the
// stage's buffers, and the two launches around the stage's kernels.  Nothing here is exported.
#ifndef LLD_MAP_INTERNAL_H
#define LLD_MAP_INTERNAL_H

#include "lld_common.h"

namespace lld_map_dev {

// Where stage 2 keeps the local map it searches (the buffers lld_frame_track_local_map stages from the host), the frame's two "holds" tables
// and a backup of them (device scratch of the stage).
struct GatherDst {
  int nt, nl;
  float* pos; float* nrm; float* maxd; float* mind; uint8_t* obs; uint8_t* skip; uint32_t* desc; int32_t* id;
  double* x0; double* dir; double* x1; double* x2; uint8_t* lskip; float* ldesc; int32_t* lid;   // all null: the frame has no lines
  uint8_t* kp_has; uint8_t* ln_has; uint8_t* bk_kp; uint8_t* bk_ln;
  int32_t* rec2;                                   // the stage-2 record header as int32 words, n_rec2 of them
  int n_rec2;
};

struct Limits { lld_ctx* ctx; int max_local_points, max_local_lines, line_dim; bool poisoned; unsigned long long serial; };   // serial: of the last UpdateLocalMap run on the map
Limits limits(const lld_map* m);
// Copies the rows the local lists name into stage 2's input layout; entries behind the device-side counts are skipped entries.  When the last
// lld_frame_track_update_local_map overflowed, every entry is skipped AND the frame's holds tables are emptied (saved in bk_*) so that the
// stage's kernels find nothing to do; restore_launch, queued behind them, puts the tables back and blanks the stage-2 record.
int gather_launch(hipStream_t st, const lld_map* m, const GatherDst& G);
int restore_launch(hipStream_t st, const lld_map* m, const GatherDst& G);

}  // namespace lld_map_dev

#endif
