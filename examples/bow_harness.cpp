// C++ caller of lld_amd::ORBVocabulary (include/lld_amd.hpp): loadFromTextFile, transform of two descriptor sets and their score,
// the calls Frame::ComputeBoW / KeyFrame::ComputeBoW and KeyFrameDatabase make.
//   bow_harness <vocabulary.txt> <in.bin> <out.bin>
//   in.bin:  int32 levelsup, int32 n1, u32 [n1][8], int32 n2, u32 [n2][8]
//   out.bin: per set: int32 n_words, {int32 word, f64 value} x n_words, int32 n_nodes, {int32 node, int32 count, int32 features[count]}
//            x n_nodes; then f64 score(v1, v2)
#include <cstdio>
#include <vector>

#include "lld_amd.hpp"

static bool read_set(FILE* f, std::vector<uint32_t>* d) {
  int32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n < 0) return false;
  d->resize((size_t)n * 8);
  return n == 0 || std::fread(d->data(), 32, (size_t)n, f) == (size_t)n;
}

static void write_vectors(FILE* f, const lld_amd::BowVector& v, const lld_amd::FeatureVector& fv) {
  int32_t n = (int32_t)v.size();
  std::fwrite(&n, 4, 1, f);
  for (lld_amd::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) {
    int32_t w = (int32_t)it->first;
    std::fwrite(&w, 4, 1, f); std::fwrite(&it->second, 8, 1, f);
  }
  n = (int32_t)fv.size();
  std::fwrite(&n, 4, 1, f);
  for (lld_amd::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
    int32_t h[2] = {(int32_t)it->first, (int32_t)it->second.size()};
    std::fwrite(h, 4, 2, f);
    for (size_t i = 0; i < it->second.size(); i++) { int32_t x = (int32_t)it->second[i]; std::fwrite(&x, 4, 1, f); }
  }
}

int main(int argc, char** argv) {
  if (argc != 4) { std::fprintf(stderr, "usage: %s vocabulary.txt in.bin out.bin\n", argv[0]); return 2; }
  FILE* in = std::fopen(argv[2], "rb");
  if (!in) return 2;
  int32_t levelsup = 4;
  std::vector<uint32_t> d1, d2;
  const bool ok = std::fread(&levelsup, 4, 1, in) == 1 && read_set(in, &d1) && read_set(in, &d2);
  std::fclose(in);
  if (!ok) return 2;
  try {
    lld_amd::Context ctx(0);
    lld_amd::ORBVocabulary voc(ctx);
    if (!voc.loadFromTextFile(argv[1])) { std::fprintf(stderr, "loadFromTextFile failed\n"); return 3; }
    lld_amd::BowVector v1, v2;
    lld_amd::FeatureVector f1, f2;
    voc.transform(d1, v1, f1, levelsup);
    voc.transform(d2, v2, f2, levelsup);
    const double s = voc.score(v1, v2);
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    write_vectors(out, v1, f1);
    write_vectors(out, v2, f2);
    std::fwrite(&s, 8, 1, out);
    std::fclose(out);
    std::printf("bow_harness: %zu words / %zu nodes, %zu words / %zu nodes, score %.17g\n", v1.size(), f1.size(), v2.size(), f2.size(), s);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
