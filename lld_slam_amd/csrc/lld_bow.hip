// lld_bow.hip — DBoW2's TemplatedVocabulary<FORB> on the device: the text loader (host), the upload, transform into BowVector +
// FeatureVector, and L1Scoring::score.  The rules restated and the two deviations are written out in include/lld_amd.h.
//
// Layout on the device (one slab per vocabulary):
//   info[n_nodes]        int2 {packed position of the first child, child count}; the children of a node are contiguous
//   pdesc[n_nodes-1][8]  u32 child descriptors in packed order (32 B each, so a node's k children are k x 32 B)
//   pnode[n_nodes-1]     node id of each packed child
//   word_of / weight     per node (word_of = -1 for a node with children)
//   qpos[n_words]        word -> position in the query of lld_bow_score, -1 between calls
// Kernels:
//   bow_descend   16 lanes per descriptor, one child per lane; the minimum of (distance << 6 | child position) over the group is
//                 the reference's strict-< scan (the first child wins a tie)
//   bow_assemble  one 1024-thread workgroup per set: bitonic sort of (word, feature) and (nid, feature) keys in LDS, the word sums
//                 by repeated addition, the L1 norm summed by one lane in ascending word order, the CSR of the FeatureVector
//   bow_score     one wavefront per candidate: the terms of the common words in parallel (qpos lookup), summed in word order
//                 (lld_bow_l1_score_wave of lld_bow_score.h, which the keyframe database runs too)
#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <string>

#include "lld_bow_score.h"
#include "lld_common.h"
#include "lld_track_internal.h"
#include "lld_wave.h"

namespace {

constexpr int kGroup = 16;                       // lanes per descriptor in bow_descend
constexpr int kDescPerBlock = 256 / kGroup;
constexpr int kFeatBits = 13;                    // LLD_BOW_MAX_FEATURES = 1 << kFeatBits
constexpr int kAsmThreads = 1024;
constexpr int kAsmPerThread = LLD_BOW_MAX_FEATURES / kAsmThreads;
static_assert((1 << kFeatBits) == LLD_BOW_MAX_FEATURES, "feature index bits");
static_assert(LLD_BOW_MAX_CHILDREN <= 64, "child position must fit 6 bits");

struct BowSetDev {
  const uint32_t* desc;
  int32_t n;
  int32_t nid_level;                             // m_L - levelsup, clamped to int
  int32_t feat_off;                              // into the per-feature scratch
  int32_t pad;
  size_t out_off;                                // byte offset of the set's output block
};

// Output block of a set with n features: value[n] f64, then int32 {n_words, n_nodes}, word[n], node[n], node_start[n+1],
// feature[n], feature_word[n], feature_nid[n].
size_t out_block_bytes(int n) { return lld_slab::pad((size_t)8 * n + (size_t)4 * (6 * (size_t)n + 3)); }

}  // namespace

struct lld_bow_vocab {
  lld_ctx* ctx = nullptr;
  lld_bow_vocab_info info{};
  void* dmem = nullptr;
  int2* d_info = nullptr;
  uint4* d_pdesc = nullptr;
  int32_t* d_pnode = nullptr;
  int32_t* d_word_of = nullptr;
  double* d_weight = nullptr;
  int32_t* d_qpos = nullptr;
  int32_t* d_fword = nullptr; int32_t* d_fnid = nullptr; double* d_fw = nullptr;
  char* d_stage = nullptr; char* h_stage = nullptr; size_t stage_bytes = 0;    // set table + host descriptors
  char* d_out = nullptr; char* h_out = nullptr; size_t out_bytes = 0;
};

// ------------------------------------------------------------------------------------------------------------------ kernels

__global__ __launch_bounds__(256) void bow_descend(const int2* __restrict__ info, const uint4* __restrict__ pdesc,
                                                   const int32_t* __restrict__ pnode, const int32_t* __restrict__ word_of,
                                                   const double* __restrict__ weight, const BowSetDev* __restrict__ sets,
                                                   int32_t* __restrict__ fword, int32_t* __restrict__ fnid, double* __restrict__ fw) {
  const BowSetDev S = sets[blockIdx.y];
  const int lane = threadIdx.x & (kGroup - 1);
  const int f = blockIdx.x * kDescPerBlock + (threadIdx.x / kGroup);
  if (f >= S.n) return;                          // whole groups leave together: the shuffles below stay inside a group
  uint32_t d[8];
  const uint32_t* q = S.desc + (size_t)f * 8;    // caller pointers are only 4-B aligned
#pragma unroll
  for (int j = 0; j < 8; j++) d[j] = q[j];
  int cur = 0, level = 0;
  int nid = S.nid_level <= 0 ? 0 : -1;
  int2 nf = info[0];
  do {
    ++level;
    unsigned best = 0xFFFFFFFFu;
    for (int c0 = 0; c0 < nf.y; c0 += kGroup) {
      const int c = c0 + lane;
      if (c < nf.y) {
        const uint4* p = pdesc + (size_t)(nf.x + c) * 2;
        const unsigned dist = lld_wave::hamming256(d, p[0], p[1]);
        best = min(best, (dist << 6) | (unsigned)c);
      }
    }
    best = lld_wave::min<kGroup>(best);
    cur = pnode[nf.x + (int)(best & 63u)];
    if (level == S.nid_level) nid = cur;
    nf = info[cur];
  } while (nf.y > 0);
  if (nid < 0) nid = cur;                        // DEVIATION: a leaf above the nid level stands for itself
  if (lane == 0) {
    const double w = weight[cur];
    const size_t o = (size_t)S.feat_off + f;
    fword[o] = (w > 0) ? word_of[cur] : -1;
    fnid[o] = nid;
    fw[o] = w;
  }
}

__global__ __launch_bounds__(kAsmThreads) void bow_assemble(const BowSetDev* __restrict__ sets, const int32_t* __restrict__ fword,
                                                            const int32_t* __restrict__ fnid, const double* __restrict__ fw, char* out,
                                                            int repeated_add) {
  __shared__ unsigned long long keys[LLD_BOW_MAX_FEATURES];
  __shared__ int tmp[kAsmThreads / 64];
  __shared__ int s_nvalid;
  __shared__ double s_norm;
  const BowSetDev S = sets[blockIdx.x];
  const int n = S.n, t = threadIdx.x;
  const int32_t* sw = fword + S.feat_off;
  const int32_t* sn = fnid + S.feat_off;
  const double* sv = fw + S.feat_off;
  char* o = out + S.out_off;
  double* value = (double*)o;
  int32_t* I = (int32_t*)(o + (size_t)8 * n);
  int32_t* word = I + 2; int32_t* node = I + 2 + n; int32_t* node_start = I + 2 + 2 * n; int32_t* feature = I + 3 + 3 * n;
  int32_t* ofword = I + 3 + 4 * n; int32_t* ofnid = I + 3 + 5 * n;
  int npad = 1;
  while (npad < n) npad <<= 1;
  if (t == 0) s_nvalid = 0;
  __syncthreads();
  int cnt = 0;
  for (int i = t; i < npad; i += blockDim.x) {
    unsigned long long k = ~0ull;
    if (i < n) {
      const int wd = sw[i];
      ofword[i] = wd; ofnid[i] = sn[i];
      if (wd >= 0) { k = ((unsigned long long)wd << kFeatBits) | (unsigned)i; cnt++; }
    }
    keys[i] = k;
  }
  if (cnt) atomicAdd(&s_nvalid, cnt);
  __syncthreads();
  const int nv = s_nvalid;
  lld_wave::bitonic_sort<kAsmThreads>(keys, npad);

  // BowVector: one run per word; thread t owns sorted positions [t*8, t*8+8)
  double v[kAsmPerThread];
  int32_t wid[kAsmPerThread];
  unsigned flags = 0;
  cnt = 0;
#pragma unroll
  for (int e = 0; e < kAsmPerThread; e++) {
    const int i = t * kAsmPerThread + e;
    v[e] = 0.0; wid[e] = 0;
    if (i < nv) {
      const unsigned long long wk = keys[i] >> kFeatBits;
      if (i == 0 || (keys[i - 1] >> kFeatBits) != wk) {
        double val = sv[keys[i] & (LLD_BOW_MAX_FEATURES - 1)];
        if (repeated_add)                        // BowVector::addWeight: += w per further hit, in feature order
          for (int j = i + 1; j < nv && (keys[j] >> kFeatBits) == wk; j++) val += sv[keys[j] & (LLD_BOW_MAX_FEATURES - 1)];
        v[e] = val; wid[e] = (int32_t)wk;
        flags |= 1u << e; cnt++;
      }
    }
  }
  int nw;
  int r = lld_wave::block_excl_scan<kAsmThreads>(cnt, tmp, nw);   // every lane is past its reads of keys: they may be overwritten now
  double* vals = (double*)keys;
#pragma unroll
  for (int e = 0; e < kAsmPerThread; e++)
    if (flags & (1u << e)) { vals[r] = v[e]; word[r] = wid[e]; r++; }
  __syncthreads();
  if (t == 0) {                                  // BowVector::normalize(L1): sequential, ascending word id
    double norm = 0.0;
    for (int k = 0; k < nw; k++) norm += fabs(vals[k]);
    s_norm = norm;
  }
  __syncthreads();
  const double norm = s_norm;
  for (int k = t; k < nw; k += blockDim.x) value[k] = norm > 0.0 ? vals[k] / norm : vals[k];
  __syncthreads();

  // FeatureVector: (nid, feature) keys of the kept features
  for (int i = t; i < npad; i += blockDim.x) {
    unsigned long long k = ~0ull;
    if (i < n && sw[i] >= 0) k = ((unsigned long long)(uint32_t)sn[i] << kFeatBits) | (unsigned)i;
    keys[i] = k;
  }
  __syncthreads();
  lld_wave::bitonic_sort<kAsmThreads>(keys, npad);
  flags = 0; cnt = 0;
#pragma unroll
  for (int e = 0; e < kAsmPerThread; e++) {
    const int i = t * kAsmPerThread + e;
    if (i < nv) {
      feature[i] = (int32_t)(keys[i] & (LLD_BOW_MAX_FEATURES - 1));
      if (i == 0 || (keys[i - 1] >> kFeatBits) != (keys[i] >> kFeatBits)) { flags |= 1u << e; cnt++; }
    }
  }
  int nn;
  r = lld_wave::block_excl_scan<kAsmThreads>(cnt, tmp, nn);
#pragma unroll
  for (int e = 0; e < kAsmPerThread; e++)
    if (flags & (1u << e)) {
      const int i = t * kAsmPerThread + e;
      node[r] = (int32_t)(keys[i] >> kFeatBits); node_start[r] = i; r++;
    }
  if (t == 0) { I[0] = nw; I[1] = nn; node_start[nn] = nv; }
}

__global__ void bow_qpos_set(int32_t* qpos, const int32_t* __restrict__ qword, int nq, int mark) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nq; i += gridDim.x * blockDim.x) qpos[qword[i]] = mark ? i : -1;
}

__global__ __launch_bounds__(256) void bow_score(const int32_t* __restrict__ qpos, const double* __restrict__ qval, int n_cand,
                                                 const int32_t* __restrict__ cstart, const int32_t* __restrict__ cword,
                                                 const double* __restrict__ cval, double* __restrict__ out) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= n_cand) return;
  const double score = lld_bow_l1_score_wave(qpos, qval, cword, cval, cstart[c], cstart[c + 1], lane);
  if (lane == 0) out[c] = score;
}

// lld_frame_compute_bow's one-entry set table
__global__ void bow_set_store(BowSetDev S, BowSetDev* dst) {
  if (threadIdx.x == 0) *dst = S;
}

// ------------------------------------------------------------------------------------------------------------------ host

namespace {

// One set's output block (host copy) into the caller's arrays.
int unpack_result(const char* o, int n, lld_bow_result& R) {
  const int32_t* I = (const int32_t*)(o + (size_t)8 * n);
  const int nw = I[0], nn = I[1];
  if (nw < 0 || nw > n || nn < 0 || nn > n) return LLD_ERR_HIP;
  R.n_words = nw; R.n_nodes = nn;
  const int nv = I[2 + 2 * n + nn];              // node_start[n_nodes]
  if (nv < 0 || nv > n) return LLD_ERR_HIP;
  if (nw) { std::memcpy(R.value, o, (size_t)nw * 8); std::memcpy(R.word, I + 2, (size_t)nw * 4); }
  if (nn) std::memcpy(R.node, I + 2 + n, (size_t)nn * 4);
  std::memcpy(R.node_start, I + 2 + 2 * n, (size_t)(nn + 1) * 4);
  if (nv) std::memcpy(R.feature, I + 3 + 3 * n, (size_t)nv * 4);
  if (R.feature_word && n) std::memcpy(R.feature_word, I + 3 + 4 * n, (size_t)n * 4);
  if (R.feature_nid && n) std::memcpy(R.feature_nid, I + 3 + 5 * n, (size_t)n * 4);
  return LLD_OK;
}

// Whitespace-separated tokens of one line.
void split(const std::string& s, std::vector<std::string>* out) {
  out->clear();
  size_t i = 0;
  while (i < s.size()) {
    while (i < s.size() && std::isspace((unsigned char)s[i])) i++;
    size_t j = i;
    while (j < s.size() && !std::isspace((unsigned char)s[j])) j++;
    if (j > i) out->push_back(s.substr(i, j - i));
    i = j;
  }
}

bool to_int(const std::string& s, int* v) {
  char* e = nullptr;
  errno = 0;
  const long x = std::strtol(s.c_str(), &e, 10);
  if (errno || *e || x < INT_MIN || x > INT_MAX) return false;
  *v = (int)x;
  return true;
}

bool to_double(const std::string& s, double* v) {
  char* e = nullptr;
  *v = std::strtod(s.c_str(), &e);
  return e && *e == 0 && e != s.c_str();
}

bool read_line(FILE* f, std::string* s) {
  s->clear();
  int c;
  bool any = false;
  while ((c = std::fgetc(f)) != EOF) {
    any = true;
    if (c == '\n') return true;
    s->push_back((char)c);
  }
  return any;
}

}  // namespace

extern "C" int lld_bow_vocab_read_text(const char* path, lld_bow_vocab_desc* d) {
  if (!path || !d) return LLD_ERR_INVALID;
  const bool fill = d->parent != nullptr;
  if (fill && (!d->is_leaf || !d->desc || !d->weight || d->n_nodes < 1)) return LLD_ERR_INVALID;
  FILE* f = std::fopen(path, "rb");
  if (!f) return LLD_ERR_INVALID;
  std::string line;
  std::vector<std::string> tok;
  int hdr[4];
  int st = LLD_OK;
  if (!read_line(f, &line)) st = LLD_ERR_INVALID;
  if (!st) {
    split(line, &tok);
    if (tok.size() < 4) st = LLD_ERR_INVALID;
    for (int i = 0; !st && i < 4; i++)
      if (!to_int(tok[i], &hdr[i])) st = LLD_ERR_INVALID;
  }
  // TemplatedVocabulary.h:1358
  if (!st && (hdr[0] < 0 || hdr[0] > 20 || hdr[1] < 1 || hdr[1] > 10 || hdr[2] < 0 || hdr[2] > 5 || hdr[3] < 0 || hdr[3] > 3))
    st = LLD_ERR_INVALID;
  int n = 1, words = 0;
  if (fill) {
    d->parent[0] = -1; d->is_leaf[0] = 0; d->weight[0] = 0.0;
    std::memset(d->desc, 0, 32);
  }
  while (!st && read_line(f, &line)) {
    split(line, &tok);
    if (tok.empty()) continue;                   // DEVIATION: blank lines (the reference's trailing empty line) add no node
    int pid, leaf;
    double w;
    uint8_t bytes[32];
    if (tok.size() < 35 || !to_int(tok[0], &pid) || !to_int(tok[1], &leaf) || !to_double(tok[34], &w) || pid < 0 || pid >= n) {
      st = LLD_ERR_INVALID;
      break;
    }
    for (int j = 0; j < 32; j++) {
      int b;
      if (!to_int(tok[2 + j], &b)) { st = LLD_ERR_INVALID; break; }
      bytes[j] = (uint8_t)b;                     // FORB::fromString: (unsigned char) of the int
    }
    if (st) break;
    if (fill) {
      if (n >= d->n_nodes) { st = LLD_ERR_INVALID; break; }
      d->parent[n] = pid; d->is_leaf[n] = leaf > 0 ? 1 : 0; d->weight[n] = w;
      std::memcpy(d->desc + (size_t)n * 8, bytes, 32);
    }
    if (leaf > 0) words++;
    if (n == INT_MAX) { st = LLD_ERR_INVALID; break; }
    n++;
  }
  std::fclose(f);
  if (st) return st;
  if (fill && (n != d->n_nodes || words != d->n_words)) return LLD_ERR_INVALID;
  d->k = hdr[0]; d->L = hdr[1]; d->scoring = hdr[2]; d->weighting = hdr[3];
  d->n_nodes = n; d->n_words = words;
  return LLD_OK;
}

extern "C" int lld_bow_vocab_create(lld_ctx* ctx, const lld_bow_vocab_desc* d, int max_sets, int max_features, lld_bow_vocab** out) {
  if (!ctx || !d || !out) return LLD_ERR_INVALID;
  *out = nullptr;
  if (!d->parent || !d->is_leaf || !d->desc || !d->weight || d->n_nodes < 2 || max_sets < 1 || max_sets > 65535 || max_features < 1 ||
      max_features > LLD_BOW_MAX_FEATURES)
    return LLD_ERR_INVALID;
  if (d->weighting < 0 || d->weighting > 3 || d->scoring < 0 || d->scoring > 5) return LLD_ERR_INVALID;
  if (d->scoring != LLD_BOW_L1_NORM) return LLD_ERR_UNSUPPORTED;
  const int nn = d->n_nodes;
  // the tree: node 0 is the root, parents come first, leaf flag == "has no children", <= 64 children, depth <= 16
  if (d->parent[0] != -1 || d->is_leaf[0]) return LLD_ERR_INVALID;
  std::vector<int32_t> nch(nn, 0), depth(nn, 0), first(nn, 0), word_of(nn, -1);
  for (int i = 1; i < nn; i++) {
    const int p = d->parent[i];
    if (p < 0 || p >= i) return LLD_ERR_INVALID;
    if (++nch[p] > LLD_BOW_MAX_CHILDREN) return LLD_ERR_INVALID;
    depth[i] = depth[p] + 1;
    if (depth[i] > LLD_BOW_MAX_DEPTH) return LLD_ERR_INVALID;
  }
  int words = 0, min_leaf = INT_MAX, max_depth = 0;
  for (int i = 0; i < nn; i++) {
    if ((d->is_leaf[i] != 0) != (nch[i] == 0)) return LLD_ERR_INVALID;
    if (nch[i] == 0) { word_of[i] = words++; min_leaf = std::min(min_leaf, depth[i]); }
    max_depth = std::max(max_depth, depth[i]);
  }
  if (words != d->n_words) return LLD_ERR_INVALID;
  // pack: the children of a node contiguous, in ascending id
  for (int i = 0, pos = 0; i < nn; i++) { first[i] = pos; pos += nch[i]; }
  std::vector<int32_t> fill(first);
  std::vector<int2> info(nn);
  std::vector<uint32_t> pdesc((size_t)(nn - 1) * 8);
  std::vector<int32_t> pnode(nn - 1);
  for (int i = 1; i < nn; i++) {
    const int pos = fill[d->parent[i]]++;
    pnode[pos] = i;
    std::memcpy(&pdesc[(size_t)pos * 8], d->desc + (size_t)i * 8, 32);
  }
  for (int i = 0; i < nn; i++) info[i] = make_int2(first[i], nch[i]);

  lld_bow_vocab* v = new lld_bow_vocab();
  v->ctx = ctx;
  v->info = lld_bow_vocab_info{d->k, d->L, d->scoring, d->weighting, nn, words, min_leaf, max_depth, max_sets, max_features};
  v->stage_bytes = lld_slab::pad(sizeof(BowSetDev) * max_sets) + (size_t)max_sets * max_features * 32;
  v->out_bytes = (size_t)max_sets * out_block_bytes(max_features);
  const size_t F = (size_t)max_sets * max_features;
  const size_t bytes = lld_slab::pad(sizeof(int2) * nn) + lld_slab::pad((size_t)(nn - 1) * 32) + lld_slab::pad((size_t)(nn - 1) * 4) +
                       lld_slab::pad((size_t)nn * 4) + lld_slab::pad((size_t)nn * 8) + lld_slab::pad((size_t)words * 4) +
                       2 * lld_slab::pad(F * 4) + lld_slab::pad(F * 8) + lld_slab::pad(v->stage_bytes) + lld_slab::pad(v->out_bytes);
  if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(&v->dmem, bytes) != hipSuccess) { v->dmem = nullptr; lld_bow_vocab_destroy(v); return LLD_ERR_ALLOC; }
  if (hipHostMalloc((void**)&v->h_stage, v->stage_bytes, hipHostMallocDefault) != hipSuccess) { v->h_stage = nullptr; lld_bow_vocab_destroy(v); return LLD_ERR_ALLOC; }
  if (hipHostMalloc((void**)&v->h_out, v->out_bytes, hipHostMallocDefault) != hipSuccess) { v->h_out = nullptr; lld_bow_vocab_destroy(v); return LLD_ERR_ALLOC; }
  lld_slab S; S.base = (char*)v->dmem; S.size = bytes;
  v->d_info = S.take<int2>(nn);
  v->d_pdesc = S.take<uint4>((size_t)(nn - 1) * 2);
  v->d_pnode = S.take<int32_t>(nn - 1);
  v->d_word_of = S.take<int32_t>(nn);
  v->d_weight = S.take<double>(nn);
  v->d_qpos = S.take<int32_t>(words);
  v->d_fword = S.take<int32_t>(F); v->d_fnid = S.take<int32_t>(F); v->d_fw = S.take<double>(F);
  v->d_stage = S.take<char>(v->stage_bytes);
  v->d_out = S.take<char>(v->out_bytes);
  if (S.used > S.size) { lld_bow_vocab_destroy(v); return LLD_ERR_ALLOC; }
  hipStream_t st = ctx->stream;
  int rc = LLD_OK;
  if (hipMemcpyAsync(v->d_info, info.data(), sizeof(int2) * nn, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(v->d_pdesc, pdesc.data(), (size_t)(nn - 1) * 32, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(v->d_pnode, pnode.data(), (size_t)(nn - 1) * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(v->d_word_of, word_of.data(), (size_t)nn * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(v->d_weight, d->weight, (size_t)nn * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(v->d_qpos, 0xFF, (size_t)words * 4, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    rc = LLD_ERR_HIP;                            // synchronised: the pageable host vectors die with this call
  if (rc) { lld_bow_vocab_destroy(v); return rc; }
  *out = v;
  return LLD_OK;
}

extern "C" void lld_bow_vocab_destroy(lld_bow_vocab* v) {
  if (!v) return;
  if (v->dmem) (void)hipFree(v->dmem);
  if (v->h_stage) (void)hipHostFree(v->h_stage);
  if (v->h_out) (void)hipHostFree(v->h_out);
  delete v;
}

lld_ctx* lld_bow_vocab_context(const lld_bow_vocab* v) { return v->ctx; }

extern "C" int lld_bow_vocab_info_get(const lld_bow_vocab* v, lld_bow_vocab_info* out) {
  if (!v || !out) return LLD_ERR_INVALID;
  *out = v->info;
  return LLD_OK;
}

extern "C" int lld_bow_transform(lld_bow_vocab* v, int n_sets, const lld_bow_set* sets, lld_bow_result* results) {
  if (!v || !sets || !results || n_sets < 1 || n_sets > v->info.max_sets) return LLD_ERR_INVALID;
  int max_n = 0;
  for (int s = 0; s < n_sets; s++) {
    const lld_bow_set& B = sets[s];
    const lld_bow_result& R = results[s];
    if (B.n < 0 || B.n > v->info.max_features || !R.node_start) return LLD_ERR_INVALID;
    if (B.n > 0 && (!B.desc || !R.word || !R.value || !R.node || !R.feature)) return LLD_ERR_INVALID;
    max_n = std::max(max_n, B.n);
  }
  // set table and the host descriptors, packed into one upload
  BowSetDev* T = (BowSetDev*)v->h_stage;
  const size_t table = lld_slab::pad(sizeof(BowSetDev) * v->info.max_sets);
  size_t in_used = 0, out_used = 0;
  for (int s = 0; s < n_sets; s++) {
    const lld_bow_set& B = sets[s];
    const long long lvl = (long long)v->info.L - B.levelsup;
    T[s].n = B.n;
    T[s].nid_level = (int32_t)std::max<long long>(INT_MIN, std::min<long long>(INT_MAX, lvl));
    T[s].feat_off = s * v->info.max_features;
    T[s].pad = 0;
    T[s].out_off = out_used;
    out_used += out_block_bytes(B.n);
    if (B.on_device || B.n == 0) {
      T[s].desc = B.desc;
    } else {
      std::memcpy(v->h_stage + table + in_used, B.desc, (size_t)B.n * 32);
      T[s].desc = (const uint32_t*)(v->d_stage + table + in_used);
      in_used += (size_t)B.n * 32;
    }
  }
  hipStream_t st = v->ctx->stream;
  LLD_HIP_TRY(hipSetDevice(v->ctx->device));
  LLD_HIP_TRY(hipMemcpyAsync(v->d_stage, v->h_stage, table + in_used, hipMemcpyHostToDevice, st));
  const BowSetDev* dT = (const BowSetDev*)v->d_stage;
  if (max_n > 0)
    hipLaunchKernelGGL(bow_descend, dim3((max_n + kDescPerBlock - 1) / kDescPerBlock, n_sets), dim3(256), 0, st, v->d_info, v->d_pdesc,
                       v->d_pnode, v->d_word_of, v->d_weight, dT, v->d_fword, v->d_fnid, v->d_fw);
  const int repeated_add = v->info.weighting == LLD_BOW_TF_IDF || v->info.weighting == LLD_BOW_TF;
  hipLaunchKernelGGL(bow_assemble, dim3(n_sets), dim3(kAsmThreads), 0, st, dT, v->d_fword, v->d_fnid, v->d_fw, v->d_out, repeated_add);
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(v->h_out, v->d_out, out_used, hipMemcpyDeviceToHost, st));
  LLD_HIP_TRY(hipStreamSynchronize(st));
  for (int s = 0; s < n_sets; s++) {
    const int rc = unpack_result(v->h_out + T[s].out_off, sets[s].n, results[s]);
    if (rc) return rc;
  }
  return LLD_OK;
}

// Frame::ComputeBoW on a resident frame (include/lld_amd.h).  The set table has one entry, written by a kernel from its arguments: the
// vocabulary's pinned staging is not touched, so a call that returns without waiting leaves nothing a later lld_bow_transform could overwrite.
extern "C" int lld_frame_compute_bow(lld_frame* f, lld_bow_vocab* v, int levelsup, lld_bow_result* R) {
  if (!f || !v || f->ctx != v->ctx) return LLD_ERR_INVALID;
  const int n = f->nt;
  if (n < 0 || n > v->info.max_features) return LLD_ERR_INVALID;
  if (R && (!R->node_start || (n > 0 && (!R->word || !R->value || !R->node || !R->feature)))) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(v->ctx->device));
  const size_t bytes = out_block_bytes(n);
  if (!f->d_bow && hipMalloc(reinterpret_cast<void**>(&f->d_bow), bytes) != hipSuccess) { f->d_bow = nullptr; return LLD_ERR_ALLOC; }   // (nt is fixed for the frame's life)
  BowSetDev S{};
  S.desc = reinterpret_cast<const uint32_t*>(f->d + f->o_td); S.n = n;
  S.nid_level = (int32_t)std::max<long long>(INT_MIN, std::min<long long>(INT_MAX, (long long)v->info.L - levelsup));
  hipStream_t st = v->ctx->stream;
  BowSetDev* dT = reinterpret_cast<BowSetDev*>(v->d_stage);
  hipLaunchKernelGGL(bow_set_store, dim3(1), dim3(64), 0, st, S, dT);
  if (n > 0)
    hipLaunchKernelGGL(bow_descend, dim3((n + kDescPerBlock - 1) / kDescPerBlock, 1), dim3(256), 0, st, v->d_info, v->d_pdesc, v->d_pnode, v->d_word_of,
                       v->d_weight, dT, v->d_fword, v->d_fnid, v->d_fw);
  const int repeated_add = v->info.weighting == LLD_BOW_TF_IDF || v->info.weighting == LLD_BOW_TF;
  hipLaunchKernelGGL(bow_assemble, dim3(1), dim3(kAsmThreads), 0, st, dT, v->d_fword, v->d_fnid, v->d_fw, v->d_out, repeated_add);
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(f->d_bow, v->d_out, bytes, hipMemcpyDeviceToDevice, st));
  f->has_bow = true;
  if (!R) return LLD_OK;
  LLD_HIP_TRY(hipMemcpyAsync(v->h_out, v->d_out, bytes, hipMemcpyDeviceToHost, st));
  LLD_HIP_TRY(hipStreamSynchronize(st));
  return unpack_result(v->h_out, n, *R);
}

extern "C" int lld_bow_score(lld_bow_vocab* v, const lld_bow_vector* query, int n_cand, const int32_t* cand_start, const int32_t* cand_word,
                             const double* cand_value, double* out) {
  if (!v || !query || n_cand < 0 || (n_cand > 0 && (!cand_start || !out)) || query->n < 0 || (query->n > 0 && (!query->word || !query->value)))
    return LLD_ERR_INVALID;
  if (n_cand == 0) return LLD_OK;
  if (cand_start[0] < 0 || cand_start[n_cand] < cand_start[0]) return LLD_ERR_INVALID;
  if (cand_start[n_cand] > cand_start[0] && (!cand_word || !cand_value)) return LLD_ERR_INVALID;
  const int W = v->info.n_words;
  for (int i = 0; i < query->n; i++)
    if (query->word[i] < 0 || query->word[i] >= W || (i && query->word[i] <= query->word[i - 1])) return LLD_ERR_INVALID;
  for (int c = 0; c < n_cand; c++) {
    if (cand_start[c + 1] < cand_start[c]) return LLD_ERR_INVALID;
    for (int j = cand_start[c]; j < cand_start[c + 1]; j++)
      if (cand_word[j] < 0 || cand_word[j] >= W || (j > cand_start[c] && cand_word[j] <= cand_word[j - 1])) return LLD_ERR_INVALID;
  }
  // one upload: query words, query values, rebased starts, candidate words, candidate values; then out
  const int nq = query->n, c0 = cand_start[0], total = cand_start[n_cand] - c0;
  const size_t o_qv = lld_slab::pad((size_t)nq * 4), o_cs = o_qv + lld_slab::pad((size_t)nq * 8),
               o_cw = o_cs + lld_slab::pad((size_t)(n_cand + 1) * 4), o_cv = o_cw + lld_slab::pad((size_t)total * 4),
               o_out = o_cv + lld_slab::pad((size_t)total * 8), bytes = o_out + lld_slab::pad((size_t)n_cand * 8);
  void* hp = nullptr; void* dp = nullptr;
  int rc = lld_ctx_pinned(v->ctx, bytes, &hp);
  if (rc) return rc;
  LLD_HIP_TRY(hipSetDevice(v->ctx->device));
  rc = lld_ctx_scratch(v->ctx, bytes, &dp);
  if (rc) return rc;
  char* h = (char*)hp; char* dd = (char*)dp;
  if (nq) { std::memcpy(h, query->word, (size_t)nq * 4); std::memcpy(h + o_qv, query->value, (size_t)nq * 8); }
  int32_t* cs = (int32_t*)(h + o_cs);
  for (int c = 0; c <= n_cand; c++) cs[c] = cand_start[c] - c0;
  if (total) { std::memcpy(h + o_cw, cand_word + c0, (size_t)total * 4); std::memcpy(h + o_cv, cand_value + c0, (size_t)total * 8); }
  hipStream_t st = v->ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(dd, h, o_out, hipMemcpyHostToDevice, st));
  const int qb = std::max(1, std::min(1024, (nq + 255) / 256));
  if (nq) hipLaunchKernelGGL(bow_qpos_set, dim3(qb), dim3(256), 0, st, v->d_qpos, (const int32_t*)dd, nq, 1);
  hipLaunchKernelGGL(bow_score, dim3((n_cand + 3) / 4), dim3(256), 0, st, v->d_qpos, (const double*)(dd + o_qv), n_cand,
                     (const int32_t*)(dd + o_cs), (const int32_t*)(dd + o_cw), (const double*)(dd + o_cv), (double*)(dd + o_out));
  if (nq) hipLaunchKernelGGL(bow_qpos_set, dim3(qb), dim3(256), 0, st, v->d_qpos, (const int32_t*)dd, nq, 0);
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(h + o_out, dd + o_out, (size_t)n_cand * 8, hipMemcpyDeviceToHost, st));
  LLD_HIP_TRY(hipStreamSynchronize(st));
  std::memcpy(out, h + o_out, (size_t)n_cand * 8);
  return LLD_OK;
}
