// local_map_host.h — Tracking::UpdateLocalMap (src/Tracking.cc:1667-1835 of the reference) as the host runs it, in compiled C++ on flat tables:
// the two loops lld_frame_track_update_local_map replaces, for the timing of the host route (tools/time_local_map.py) and as a second
// restatement next to tests/local_map_ref.py.  Restated from the reference, not copied: objects are slots, members are arrays.
#ifndef LLD_LOCAL_MAP_HOST_H
#define LLD_LOCAL_MAP_HOST_H

#include <cstdint>
#include <vector>

namespace local_map_host {

// Every list is CSR over the slots of its table: start[n + 1], entries.  The tables are the caller's.
struct Tables {
  int n_keyframes, n_points, n_lines;
  const uint64_t* kf_key;                  // position in std::map<KeyFrame*,int> / std::set<KeyFrame*> iteration
  const uint8_t* kf_bad;                   // isBad, or the slot holds no keyframe
  const int32_t* kf_parent;                // -1: none
  const int32_t *cov_start, *cov, *child_start, *child, *point_start, *point, *line_start, *line;
  const uint8_t* pt_state;                 // 0 the map does not hold it, 1 live, 2 isBad
  const int32_t *obs_start, *obs;
  const uint8_t* ln_bad;                   // isBad, or the slot holds no line
};

enum { KEYFRAME_OVERFLOW = 1, POINT_OVERFLOW = 2, LINE_OVERFLOW = 4, MAX_VOTED = 1024 };

struct State { std::vector<int32_t> local_keyframes; };   // mvpLocalKeyFrames: it survives a frame whose vote is empty

struct Result {
  int status = 0, n_voted = 0, n_bad_cleared = 0, ref_keyframe = -1, vote_empty = 0;
  std::vector<int32_t> local_points, local_lines;
};

// frame_ids [nt]: mCurrentFrame.mvpMapPoints as point slots, -1 = NULL; a bad MapPoint's entry is set to -1 (:1743).
void update_local_map(const Tables& T, State& S, int32_t* frame_ids, int nt, int max_local_points, int max_local_lines, Result& R);

}  // namespace local_map_host

// The same through a C entry (tools/time_local_map.py loads it with ctypes).  list / n_list: mvpLocalKeyFrames, in and out (capacity 1280);
// scalars: status, n_voted, n_bad_cleared, ref_keyframe, vote_empty; local_points / local_lines: capacity max_local_points / max_local_lines
// (filled only when they fit), n_local[2] the true counts.
extern "C" void local_map_host_update(const local_map_host::Tables* T, int32_t* list, int32_t* n_list, int32_t* frame_ids, int nt, int max_local_points,
                                      int max_local_lines, int32_t* scalars, int32_t* local_points, int32_t* local_lines, int32_t* n_local);

#endif
