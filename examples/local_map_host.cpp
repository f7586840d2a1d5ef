// local_map_host.cpp — see local_map_host.h.
#include "local_map_host.h"

#include <algorithm>
#include <utility>

namespace local_map_host {

namespace {

// UpdateLocalKeyFrames (:1726-1835).  Returns false when the routine returned early or the vote overflowed: the list is then unchanged.
bool update_local_keyframes(const Tables& T, State& S, int32_t* ids, int nt, Result& R) {
  std::vector<int32_t> count(T.n_keyframes, 0);
  std::vector<std::pair<uint64_t, int32_t> > voted;                 // (key, slot): sorted below into the std::map's order
  for (int i = 0; i < nt; i++) {
    const int32_t p = ids[i];
    if (p < 0 || p >= T.n_points || T.pt_state[p] == 0) continue;   // NULL, or a temporal point the map does not hold
    if (T.pt_state[p] == 2) { ids[i] = -1; R.n_bad_cleared++; continue; }
    for (int32_t o = T.obs_start[p]; o < T.obs_start[p + 1]; o++) {
      const int32_t kf = T.obs[o];
      if (count[kf]++ == 0) voted.push_back(std::make_pair(T.kf_key[kf], kf));
    }
  }
  R.n_voted = (int)voted.size();
  if (voted.empty()) { R.vote_empty = 1; return false; }
  if (voted.size() > (size_t)MAX_VOTED) { R.status |= KEYFRAME_OVERFLOW; return false; }
  std::sort(voted.begin(), voted.end());
  std::vector<uint8_t> marked(T.n_keyframes, 0);
  std::vector<int32_t>& L = S.local_keyframes;
  L.clear();
  int best = 0;
  for (size_t v = 0; v < voted.size(); v++) {
    const int32_t kf = voted[v].second;
    if (T.kf_bad[kf]) continue;
    if (count[kf] > best) { best = count[kf]; R.ref_keyframe = kf; }
    L.push_back(kf); marked[kf] = 1;
  }
  const size_t n_first = L.size();                                  // the end iterator is taken before the pushes
  for (size_t i = 0; i < n_first; i++) {
    if (L.size() > 80) break;
    const int32_t kf = L[i];
    const int32_t c1 = std::min(T.cov_start[kf + 1], T.cov_start[kf] + 10);   // GetBestCovisibilityKeyFrames(10)
    for (int32_t c = T.cov_start[kf]; c < c1; c++) {
      const int32_t nb = T.cov[c];
      if (!T.kf_bad[nb] && !marked[nb]) { L.push_back(nb); marked[nb] = 1; break; }
    }
    // std::set<KeyFrame*>: ascending key; the first that is neither bad nor marked = the least key among those
    int32_t child = -1;
    for (int32_t c = T.child_start[kf]; c < T.child_start[kf + 1]; c++) {
      const int32_t ch = T.child[c];
      if (T.kf_bad[ch] || marked[ch]) continue;
      if (child < 0 || T.kf_key[ch] < T.kf_key[child]) child = ch;
    }
    if (child >= 0) { L.push_back(child); marked[child] = 1; }
    const int32_t par = T.kf_parent[kf];
    if (par >= 0 && !marked[par]) { L.push_back(par); marked[par] = 1; break; }   // this break leaves the outer loop (:1824)
  }
  return true;
}

// UpdateLocalPoints (:1677-1723)
void update_local_points(const Tables& T, const State& S, Result& R) {
  std::vector<uint8_t> taken_p(T.n_points, 0), taken_l(T.n_lines, 0);
  for (size_t i = 0; i < S.local_keyframes.size(); i++) {
    const int32_t kf = S.local_keyframes[i];
    for (int32_t k = T.point_start[kf]; k < T.point_start[kf + 1]; k++) {
      const int32_t p = T.point[k];
      if (p < 0 || taken_p[p] || T.pt_state[p] != 1) continue;
      R.local_points.push_back(p); taken_p[p] = 1;
    }
    for (int32_t k = T.line_start[kf]; k < T.line_start[kf + 1]; k++) {
      const int32_t l = T.line[k];
      if (l < 0 || taken_l[l] || T.ln_bad[l]) continue;
      R.local_lines.push_back(l); taken_l[l] = 1;
    }
  }
}

}  // namespace

void update_local_map(const Tables& T, State& S, int32_t* frame_ids, int nt, int max_local_points, int max_local_lines, Result& R) {
  R = Result();
  update_local_keyframes(T, S, frame_ids, nt, R);
  if (R.status & KEYFRAME_OVERFLOW) return;
  update_local_points(T, S, R);
  if ((int)R.local_points.size() > max_local_points) R.status |= POINT_OVERFLOW;
  if ((int)R.local_lines.size() > max_local_lines) R.status |= LINE_OVERFLOW;
}

}  // namespace local_map_host

extern "C" void local_map_host_update(const local_map_host::Tables* T, int32_t* list, int32_t* n_list, int32_t* frame_ids, int nt, int max_local_points,
                                      int max_local_lines, int32_t* scalars, int32_t* local_points, int32_t* local_lines, int32_t* n_local) {
  local_map_host::State S; local_map_host::Result R;
  S.local_keyframes.assign(list, list + *n_list);
  local_map_host::update_local_map(*T, S, frame_ids, nt, max_local_points, max_local_lines, R);
  *n_list = (int32_t)S.local_keyframes.size();
  std::copy(S.local_keyframes.begin(), S.local_keyframes.end(), list);
  scalars[0] = R.status; scalars[1] = R.n_voted; scalars[2] = R.n_bad_cleared; scalars[3] = R.ref_keyframe; scalars[4] = R.vote_empty;
  n_local[0] = (int32_t)R.local_points.size(); n_local[1] = (int32_t)R.local_lines.size();
  if (n_local[0] <= max_local_points) std::copy(R.local_points.begin(), R.local_points.end(), local_points);
  if (n_local[1] <= max_local_lines) std::copy(R.local_lines.begin(), R.local_lines.end(), local_lines);
}
