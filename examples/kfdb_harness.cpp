// C++ caller of lld_amd::KeyFrameDatabase (include/lld_amd.hpp): runs a binary script of database operations, the calls
// LoopClosing, KeyFrame::SetBadFlag and Tracking::Relocalization make.
//   kfdb_harness <vocabulary.txt> <script.bin> <out.bin> [max_keyframes [max_words]]      (default 1024 and 2^20)
//   script.bin: a sequence of int32 op codes, each followed by its arguments; a BowVector is int32 n, {int32 word, f64 value} x n
//     1 add     u64 id, BowVector            2 erase   u64 id            3 clear
//     4 covis   u64 id, int32 m, u64 x m     5 reloc   u64 query id, BowVector
//     6 loop    u64 query id, BowVector, int32 nc, u64 x nc (connected), f32 minScore          0 end
//   out.bin: per query: int32 n, u64 ids x n, f32 accScore x n, int32 n_sharing, max_common_words, min_common_words, n_scored
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "lld_amd.hpp"

namespace {

template <class T>
bool get(FILE* f, T* x) { return std::fread(x, sizeof(T), 1, f) == 1; }

bool get_bow(FILE* f, lld_amd::BowVector* v) {
  int32_t n = 0;
  if (!get(f, &n) || n < 0) return false;
  v->clear();
  for (int i = 0; i < n; i++) {
    int32_t w; double x;
    if (!get(f, &w) || !get(f, &x)) return false;
    (*v)[(unsigned int)w] = x;
  }
  return true;
}

void put_result(FILE* out, const lld_amd::KeyFrameDatabase& db, const std::vector<uint64_t>& ids) {
  const int32_t n = (int32_t)ids.size();
  std::fwrite(&n, 4, 1, out);
  if (n) { std::fwrite(ids.data(), 8, ids.size(), out); std::fwrite(db.lastAccScores().data(), 4, ids.size(), out); }
  const lld_kfdb_result& r = db.lastStats();
  const int32_t s[4] = {r.n_sharing, r.max_common_words, r.min_common_words, r.n_scored};
  std::fwrite(s, 4, 4, out);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4 || argc > 6) { std::fprintf(stderr, "usage: %s vocabulary.txt script.bin out.bin [max_keyframes [max_words]]\n", argv[0]); return 2; }
  const int max_keyframes = argc > 4 ? std::atoi(argv[4]) : 1024;
  const long long max_words = argc > 5 ? std::atoll(argv[5]) : 1 << 20;
  FILE* in = std::fopen(argv[2], "rb");
  FILE* out = std::fopen(argv[3], "wb");
  if (!in || !out) return 2;
  int n_queries = 0;
  try {
    lld_amd::Context ctx(0);
    lld_amd::ORBVocabulary voc(ctx);
    if (!voc.loadFromTextFile(argv[1])) { std::fprintf(stderr, "loadFromTextFile failed\n"); return 3; }
    lld_amd::KeyFrameDatabase db(voc, max_keyframes, (int64_t)max_words);
    int32_t op = 0;
    while (get(in, &op) && op != 0) {
      uint64_t id = 0;
      lld_amd::BowVector v;
      if (op == 3) { db.clear(); continue; }
      if (!get(in, &id)) return 2;
      if (op == 1) {
        if (!get_bow(in, &v)) return 2;
        db.add(id, v);
      } else if (op == 2) {
        db.erase(id);
      } else if (op == 4) {
        int32_t m = 0;
        if (!get(in, &m) || m < 0) return 2;
        std::vector<uint64_t> nb((size_t)m);
        if (m && std::fread(nb.data(), 8, (size_t)m, in) != (size_t)m) return 2;
        db.setCovisibles(id, nb);
      } else if (op == 5) {
        if (!get_bow(in, &v)) return 2;
        put_result(out, db, db.DetectRelocalizationCandidates(id, v));
        n_queries++;
      } else if (op == 6) {
        int32_t nc = 0;
        if (!get_bow(in, &v) || !get(in, &nc) || nc < 0) return 2;
        std::set<uint64_t> conn;
        for (int i = 0; i < nc; i++) { uint64_t c; if (!get(in, &c)) return 2; conn.insert(c); }
        float ms = 0.0f;
        if (!get(in, &ms)) return 2;
        put_result(out, db, db.DetectLoopCandidates(id, v, conn, ms));
        n_queries++;
      } else {
        return 2;
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::fclose(in);
  std::fclose(out);
  std::printf("kfdb_harness: %d queries\n", n_queries);
  return 0;
}
