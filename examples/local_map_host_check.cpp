// local_map_host_check.cpp — runs local_map_host.cpp on a scene file and prints what it computed, one line per frame; a stand-alone program
// (tests/test_local_map_ref.py builds it with g++, once more with -fsanitize=address,undefined, and compares the lines with tests/local_map_ref.py).
// Scene file, whitespace-separated integers: n_keyframes n_points n_lines max_local_points max_local_lines; per keyframe slot: key bad parent,
// then four lists (cov, child, point, line) each as count and entries; per point slot: state and its observation list; per line slot: bad;
// then the number of steps and per step: 0 nt ids... (a frame) or 1 n slots... (these points turn bad).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "local_map_host.h"

namespace {
std::FILE* in = nullptr;
long long next_int() { long long v; if (std::fscanf(in, "%lld", &v) != 1) { std::fprintf(stderr, "scene file ends early\n"); std::exit(2); } return v; }
unsigned long long next_u64() { unsigned long long v; if (std::fscanf(in, "%llu", &v) != 1) { std::fprintf(stderr, "scene file ends early\n"); std::exit(2); } return v; }
void read_list(std::vector<int32_t>& start, std::vector<int32_t>& flat) {
  const int n = (int)next_int();
  for (int i = 0; i < n; i++) flat.push_back((int32_t)next_int());
  start.push_back((int32_t)flat.size());
}
void print_list(const std::vector<int32_t>& v) { std::printf(" %zu", v.size()); for (size_t i = 0; i < v.size(); i++) std::printf(" %d", v[i]); }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2 || !(in = std::fopen(argv[1], "r"))) { std::fprintf(stderr, "usage: local_map_host_check scene.txt\n"); return 2; }
  const int nk = (int)next_int(), np = (int)next_int(), nl = (int)next_int(), max_lp = (int)next_int(), max_ll = (int)next_int();
  std::vector<uint64_t> key(nk); std::vector<uint8_t> kbad(nk), state(np), lbad(nl); std::vector<int32_t> parent(nk);
  std::vector<int32_t> cs(1, 0), cv, hs(1, 0), hv, ps(1, 0), pv, ls(1, 0), lv, os(1, 0), ov;
  for (int k = 0; k < nk; k++) {
    key[k] = next_u64(); kbad[k] = (uint8_t)next_int(); parent[k] = (int32_t)next_int();
    read_list(cs, cv); read_list(hs, hv); read_list(ps, pv); read_list(ls, lv);
  }
  for (int p = 0; p < np; p++) { state[p] = (uint8_t)next_int(); read_list(os, ov); }
  for (int l = 0; l < nl; l++) lbad[l] = (uint8_t)next_int();
  local_map_host::Tables T;
  T.n_keyframes = nk; T.n_points = np; T.n_lines = nl;
  T.kf_key = key.data(); T.kf_bad = kbad.data(); T.kf_parent = parent.data();
  T.cov_start = cs.data(); T.cov = cv.data(); T.child_start = hs.data(); T.child = hv.data(); T.point_start = ps.data(); T.point = pv.data();
  T.line_start = ls.data(); T.line = lv.data(); T.pt_state = state.data(); T.obs_start = os.data(); T.obs = ov.data(); T.ln_bad = lbad.data();
  local_map_host::State S;
  const int n_steps = (int)next_int();
  for (int s = 0; s < n_steps; s++) {
    const int kind = (int)next_int(), n = (int)next_int();
    std::vector<int32_t> v(n);
    for (int i = 0; i < n; i++) v[i] = (int32_t)next_int();
    if (kind == 1) { for (int i = 0; i < n; i++) state[v[i]] = 2; continue; }
    local_map_host::Result R;
    local_map_host::update_local_map(T, S, v.data(), n, max_lp, max_ll, R);
    std::printf("%d %d %d %d %d", R.status, R.n_voted, R.n_bad_cleared, R.ref_keyframe, R.vote_empty);
    print_list(v);
    if (!(R.status & local_map_host::KEYFRAME_OVERFLOW)) { print_list(S.local_keyframes); print_list(R.local_points); print_list(R.local_lines); }
    std::printf("\n");
  }
  std::fclose(in);
  return 0;
}
