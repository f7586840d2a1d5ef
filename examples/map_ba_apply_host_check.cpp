// map_ba_apply_host_check.cpp — the host tail of LocalBundleAdjustment (map_ba_apply_host.cpp) over a scene file, stand-alone (no
// liblld_amd.so):  map_ba_apply_host_check <scene> <answer>.  tests/test_map_ba_apply_host.py holds the answer to tests/map_ba_apply_ref.py.
#include <cstdio>

#include "map_ba_apply_scene.h"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: map_ba_apply_host_check <scene> <answer>\n"); return 1; }
  try {
    using namespace map_ba_apply_scene;
    Scene S; read_scene(argv[1], S);
    map_ba_apply_host::Out O;
    map_ba_apply_host::apply(S.M, S.W, S.R, O);
    const map_ba_apply_host::Map& M = S.M;
    const std::vector<int32_t>& P = S.W.point_slot; const std::vector<int32_t>& L = S.W.line_slot;
    File w(argv[2], "wb");
    const int32_t counts[6] = {S.W.n_local, O.n_pt_obs_erased, O.n_ln_obs_erased, O.n_points_bad, O.n_lines_bad, O.n_index_skipped};
    w.put(counts, 6); w.put(S.R.tcw); w.put(O.ow);
    std::vector<float> pos, nrm, mind, maxd; std::vector<int32_t> nobs, ref, len, lnobs, llen; std::vector<uint8_t> lbad;
    for (size_t q = 0; q < P.size(); q++) {
      const int s = P[q];
      for (int k = 0; k < 3; k++) { pos.push_back(M.pt_pos[3 * (size_t)s + k]); nrm.push_back(M.pt_nrm[3 * (size_t)s + k]); }
      mind.push_back(M.pt_mind[s]); maxd.push_back(M.pt_maxd[s]); nobs.push_back(M.pt_nobs[s]); ref.push_back(M.has_refs ? M.pt_ref[s] : -1);
      len.push_back((int32_t)M.pt_obs_kf[s].size());
    }
    for (size_t l = 0; l < L.size(); l++) { lbad.push_back(M.ln_bad[L[l]]); lnobs.push_back(M.ln_nobs[L[l]]); llen.push_back((int32_t)M.ln_obs_kf[L[l]].size()); }
    w.put(pos); w.put(nrm); w.put(mind); w.put(maxd); w.put(nobs); w.put(ref); w.put(len); w.put(O.pt_flags); w.put(lbad); w.put(lnobs); w.put(llen);
    put_rows(w, M.pt_obs_kf); put_rows(w, M.pt_obs_idx); put_rows(w, M.kf_points); put_rows(w, M.kf_lines); put_rows(w, M.ln_obs_kf); put_rows(w, M.ln_obs_idx);
    std::printf("erased %d + %d, bad %d + %d, skipped %d; changed rows: %zu keyframes, %zu points, %zu lines\n", O.n_pt_obs_erased, O.n_ln_obs_erased, O.n_points_bad,
                O.n_lines_bad, O.n_index_skipped, O.changed_kf_rows.size(), O.changed_pt_rows.size(), O.changed_ln_rows.size());
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "map_ba_apply_host_check: %s\n", e.what());
    return 1;
  }
}
