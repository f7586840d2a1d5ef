// lld_kfdb.hip — ORB-SLAM2's KeyFrameDatabase on the device: the resident BowVectors of the keyframes (the inverted file), their
// covisibility lists and the per-keyframe query registers of KeyFrame, and the two queries DetectLoopCandidates /
// DetectRelocalizationCandidates.  The rules restated and the one deviation are written out in include/lld_amd.h.
//
// Layout on the device (one handle):
//   slot[max_keyframes]     KfSlot: the keyframe's BowVector as a range of the word pool, its add sequence number, its first <= 10
//                           covisibles (slots), its id.  A keyframe not in the database has n = 0.
//   regs[max_keyframes]     KfRegs: mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore
//   word / value pools      [2][max_words]: the BowVectors of the keyframes in the database.  Every (word, keyframe) pair of the
//                           reference's mvInvertedFile is one pool entry; a bucket's list order is rebuilt from the add sequence
//                           numbers.  Adds append; an add that does not fit behind the last vector compacts into the other pool.
//   qpos[n_words]           word -> position in the query, -1 between queries
//   per-query scratch       connected flags, listed slots, first query word per slot, kept entries, accScore / pBestKF per entry,
//                           a min-key per slot (-1 between queries), counters, and the output records
// Kernels of one query:
//   kfdb_prep    qpos and connected flags of the query, counters to zero
//   kfdb_walk    one wavefront per slot: the common words with the query (count, first query word), then the register update of
//                the walk (:86-104 / :207-222) and the listing of lKFsSharingWords
//   kfdb_score   one wavefront per listed slot: words > minCommonWords -> the L1 score (lld_bow_score.h), the score register, and
//                lScoreAndMatch.  A kernel boundary follows: every register is final before anything accumulates
//   kfdb_finish  one workgroup: accumulation over <= 10 covisibles, bestAccScore, retention, de-duplication by the smallest
//                (first word, add seq) key per pBestKF, a bitonic sort of the kept keys in LDS and the output in list order;
//                resets qpos, the connected flags and the min-keys
#include <algorithm>
#include <climits>
#include <unordered_map>
#include <unordered_set>

#include "lld_bow_score.h"
#include "lld_common.h"
#include "lld_wave.h"

namespace {

constexpr int kNb = LLD_KFDB_MAX_COVISIBLES;
constexpr int kFinishThreads = 1024;

struct KfSlot {
  int32_t off, n;                                // range of the word pool; n = 0: not in the database
  uint32_t seq;                                  // add sequence number (list order of every bucket)
  int32_t nnb;                                   // GetBestCovisibilityKeyFrames(10): the first nnb of nb
  int32_t nb[kNb];
  unsigned long long id;
};
static_assert(sizeof(KfSlot) == 64, "slot record");

struct KfRegs {
  unsigned long long loop_query, reloc_query;
  int32_t loop_words, reloc_words;
  float loop_score, reloc_score;
};

struct KfKept {
  int32_t slot;
  float si;
  unsigned long long key;                        // first query word << 32 | add seq = the position in lKFsSharingWords
};

struct KfCounters {
  int32_t n_listed, max_words, n_scored, n_kept, n_out, min_words, pad[2];
};

struct KfOut {
  unsigned long long id;
  float acc;
  int32_t pad;
};

struct Move {
  int32_t from, to, n;
};

// bestAccScore's `if(accScore>bestAccScore)`: the later value replaces only when strictly greater, so every partial starting
// from the initial value and combined this way gives the sequential result.
__device__ inline float keep_greater(float a, float b) { return b > a ? b : a; }

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ kernels

__global__ __launch_bounds__(256) void kfdb_scatter(const int32_t* __restrict__ idx, const KfSlot* __restrict__ rec, int m,
                                                    KfSlot* __restrict__ slot) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) slot[idx[i]] = rec[i];
}

__global__ __launch_bounds__(256) void kfdb_compact(const Move* __restrict__ moves, const int32_t* __restrict__ wsrc,
                                                    const double* __restrict__ vsrc, int32_t* __restrict__ wdst,
                                                    double* __restrict__ vdst) {
  const Move M = moves[blockIdx.x];
  for (int j = threadIdx.x; j < M.n; j += blockDim.x) {
    wdst[M.to + j] = wsrc[M.from + j];
    vdst[M.to + j] = vsrc[M.from + j];
  }
}

__global__ __launch_bounds__(256) void kfdb_prep(const int32_t* __restrict__ qword, int nq, const int32_t* __restrict__ cslot,
                                                 int nc, int32_t* __restrict__ qpos, int32_t* __restrict__ conn,
                                                 KfCounters* __restrict__ C) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, stride = gridDim.x * blockDim.x;
  for (int i = t; i < nq; i += stride) qpos[qword[i]] = i;
  for (int i = t; i < nc; i += stride) conn[cslot[i]] = 1;
  if (t == 0) *C = KfCounters{};
}

__global__ __launch_bounds__(256) void kfdb_walk(const KfSlot* __restrict__ slot, int n_slots, const int32_t* __restrict__ pword,
                                                 const int32_t* __restrict__ qpos, const int32_t* __restrict__ conn,
                                                 KfRegs* __restrict__ regs, unsigned long long qid, int loop,
                                                 int32_t* __restrict__ listed, int32_t* __restrict__ first, KfCounters* C) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= n_slots) return;
  const int off = slot[s].off, n = slot[s].n;
  if (n <= 0) return;
  int cnt = 0, mn = INT_MAX;
  for (int j = lane; j < n; j += 64) {
    const int p = qpos[pword[off + j]];
    if (p >= 0) { cnt++; mn = min(mn, p); }
  }
  cnt = lld_wave::sum(cnt);
  mn = lld_wave::min(mn);
  if (lane || cnt == 0) return;
  // The walk meets this keyframe cnt times.  Per encounter: a stamp != id resets words to 0 and (unless connected) stamps and
  // lists it; then words++.
  KfRegs& R = regs[s];
  bool list = false;
  if (loop) {
    if (R.loop_query == qid) R.loop_words += cnt;
    else if (conn[s]) R.loop_words = 1;          // never stamped: reset at every encounter
    else { R.loop_words = cnt; R.loop_query = qid; list = true; }
  } else {
    if (R.reloc_query == qid) R.reloc_words += cnt;
    else { R.reloc_words = cnt; R.reloc_query = qid; list = true; }
  }
  if (list) {
    listed[atomicAdd(&C->n_listed, 1)] = s;
    first[s] = mn;
    atomicMax(&C->max_words, cnt);
  }
}

__global__ __launch_bounds__(256) void kfdb_score(const KfSlot* __restrict__ slot, int n_slots, const int32_t* __restrict__ pword,
                                                  const double* __restrict__ pval, const int32_t* __restrict__ qpos,
                                                  const double* __restrict__ qval, KfRegs* __restrict__ regs, int loop, float min_score,
                                                  const int32_t* __restrict__ listed, const int32_t* __restrict__ first,
                                                  KfKept* __restrict__ kept, KfCounters* C) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= C->n_listed) return;
  const int s = listed[i];
  const int words = loop ? regs[s].loop_words : regs[s].reloc_words;
  const int min_words = (int)((float)C->max_words * 0.8f);      // int minCommonWords = maxCommonWords*0.8f
  if (words <= min_words) return;
  const KfSlot S = slot[s];
  const double score = lld_bow_l1_score_wave(qpos, qval, pword + S.off, pval + S.off, 0, S.n, lane);
  if (lane) return;
  const float si = (float)score;
  if (loop) regs[s].loop_score = si; else regs[s].reloc_score = si;
  atomicAdd(&C->n_scored, 1);
  if (!loop || si >= min_score) {
    const int k = atomicAdd(&C->n_kept, 1);
    kept[k] = KfKept{s, si, ((unsigned long long)(uint32_t)first[s] << 32) | S.seq};
  }
}

__global__ __launch_bounds__(kFinishThreads) void kfdb_finish(const KfSlot* __restrict__ slot, const KfRegs* __restrict__ regs,
                                                              unsigned long long qid, int loop, float min_score,
                                                              const KfKept* __restrict__ kept, float* __restrict__ acc_of,
                                                              int32_t* __restrict__ best_of, unsigned long long* minkey,
                                                              KfCounters* C, KfOut* __restrict__ out, int capacity,
                                                              int32_t* __restrict__ qpos, const int32_t* __restrict__ qword, int nq,
                                                              int32_t* __restrict__ conn, const int32_t* __restrict__ cslot, int nc) {
  __shared__ unsigned long long keys[LLD_KFDB_MAX_KEYFRAMES];
  const int t = threadIdx.x;
  const int nk = C->n_kept;
  const int min_words = (int)((float)C->max_words * 0.8f);
  float best_acc = loop ? min_score : 0.0f;
  for (int i = t; i < nk; i += kFinishThreads) {
    const KfKept e = kept[i];
    const KfSlot* S = slot + e.slot;             // nb[] read from memory: a copy indexed by j would go to scratch
    const int nnb = S->nnb;
    float acc = e.si, best = e.si;
    int b = e.slot;
    for (int j = 0; j < nnb; j++) {
      const int s2 = S->nb[j];
      const KfRegs R = regs[s2];
      float sc;
      if (loop) {
        if (R.loop_query != qid || R.loop_words <= min_words) continue;
        sc = R.loop_score;
      } else {
        if (R.reloc_query != qid) continue;      // no words test: a stale mRelocScore counts
        sc = R.reloc_score;
      }
      acc += sc;
      if (sc > best) { best = sc; b = s2; }
    }
    acc_of[i] = acc;
    best_of[i] = b;
    best_acc = keep_greater(best_acc, acc);
  }
  // bestAccScore over the workgroup (keys[] doubles as the exchange area before it holds keys)
  best_acc = lld_wave::max(best_acc);            // (keep_greater's rule lane against lane)
  float* red = (float*)keys;
  if ((t & 63) == 0) red[t >> 6] = best_acc;
  __syncthreads();
  if (t == 0) {
    float v = red[0];
    for (int w = 1; w < kFinishThreads / 64; w++) v = keep_greater(v, red[w]);
    red[kFinishThreads / 64] = v;
  }
  __syncthreads();
  const float min_retain = 0.75f * red[kFinishThreads / 64];
  __syncthreads();
  // spAlreadyAddedKF: the entry with the smallest key among those retained with the same pBestKF is the one that is output
  for (int i = t; i < nk; i += kFinishThreads)
    if (acc_of[i] > min_retain) atomicMin(&minkey[best_of[i]], kept[i].key);
  __syncthreads();
  for (int i = t; i < nk; i += kFinishThreads)
    if (acc_of[i] > min_retain &&
        __hip_atomic_load(&minkey[best_of[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kept[i].key)
      keys[atomicAdd(&C->n_out, 1)] = kept[i].key;
  __syncthreads();
  const int n = __hip_atomic_load(&C->n_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int npad = 1;
  while (npad < n) npad <<= 1;
  for (int i = n + t; i < npad; i += kFinishThreads) keys[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < npad; i += kFinishThreads) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = keys[i], b = keys[ixj];
          if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[ixj] = a; }
        }
      }
      __syncthreads();
    }
  // the output position of a kept entry is its key's rank (keys are unique)
  for (int i = t; i < nk; i += kFinishThreads) {
    const unsigned long long key = kept[i].key;
    if (!(acc_of[i] > min_retain) ||
        __hip_atomic_load(&minkey[best_of[i]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != key)
      continue;
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < capacity) out[lo] = KfOut{slot[best_of[i]].id, acc_of[i], 0};
  }
  __syncthreads();
  for (int i = t; i < nk; i += kFinishThreads)
    if (acc_of[i] > min_retain) minkey[best_of[i]] = ~0ull;
  for (int i = t; i < nq; i += kFinishThreads) qpos[qword[i]] = -1;
  for (int i = t; i < nc; i += kFinishThreads) conn[cslot[i]] = 0;
  if (t == 0) C->min_words = min_words;
}

// ------------------------------------------------------------------------------------------------------------------ host

namespace {

struct SlotHost {
  KfSlot rec;
  bool in_db;
};

}  // namespace

struct lld_kfdb {
  lld_ctx* ctx = nullptr;
  int n_words = 0;
  int max_kf = 0;
  int64_t max_words = 0;
  std::unordered_map<uint64_t, int> slot_of;
  std::vector<SlotHost> slots;
  int64_t pool_end = 0, live = 0;
  uint32_t next_seq = 0;
  int pool = 0;                                  // which of the two pools holds the vectors
  void* dmem = nullptr;
  KfSlot* d_slot = nullptr;
  KfRegs* d_regs = nullptr;
  unsigned long long* d_minkey = nullptr;
  int32_t* d_conn = nullptr; int32_t* d_listed = nullptr; int32_t* d_first = nullptr; int32_t* d_best = nullptr;
  float* d_acc = nullptr;
  KfKept* d_kept = nullptr;
  char* d_res = nullptr;                         // KfCounters, then KfOut[max_kf]
  int32_t* d_qpos = nullptr;
  int32_t* d_word[2] = {nullptr, nullptr};
  double* d_val[2] = {nullptr, nullptr};
  char* d_stage = nullptr; size_t d_stage_bytes = 0;
  char* h_stage = nullptr; size_t h_stage_bytes = 0;
  char* h_res = nullptr;
};

namespace {

constexpr size_t kResHead = 256;                 // KfCounters, padded

int grow_stage(lld_kfdb* db, size_t bytes) {
  if (bytes > db->h_stage_bytes) {
    if (db->h_stage) LLD_HIP_TRY(hipHostFree(db->h_stage));
    db->h_stage = nullptr; db->h_stage_bytes = 0;
    const size_t want = bytes + (bytes >> 2) + 4096;
    LLD_HIP_TRY(hipHostMalloc((void**)&db->h_stage, want, hipHostMallocDefault));
    db->h_stage_bytes = want;
  }
  if (bytes > db->d_stage_bytes) {
    if (db->d_stage) LLD_HIP_TRY(hipFree(db->d_stage));
    db->d_stage = nullptr; db->d_stage_bytes = 0;
    const size_t want = bytes + (bytes >> 2) + 4096;
    LLD_HIP_TRY(hipMalloc((void**)&db->d_stage, want));
    db->d_stage_bytes = want;
  }
  return LLD_OK;
}

bool words_ok(const lld_bow_vector* v, int n_words) {
  if (!v || v->n < 0 || (v->n > 0 && (!v->word || !v->value))) return false;
  for (int i = 0; i < v->n; i++)
    if (v->word[i] < 0 || v->word[i] >= n_words || (i && v->word[i] <= v->word[i - 1])) return false;
  return true;
}

// Ids the call would give a new slot (each once).
int64_t new_slots(const lld_kfdb* db, const std::vector<uint64_t>& ids) {
  std::unordered_set<uint64_t> fresh;
  for (uint64_t id : ids)
    if (!db->slot_of.count(id)) fresh.insert(id);
  return (int64_t)fresh.size();
}

int slot_for(lld_kfdb* db, uint64_t id) {
  auto it = db->slot_of.find(id);
  if (it != db->slot_of.end()) return it->second;
  const int s = (int)db->slots.size();
  SlotHost h{};
  h.rec.id = id;
  h.in_db = false;
  db->slots.push_back(h);
  db->slot_of.emplace(id, s);
  return s;
}

// Uploads the records of the dirty slots (one copy, one scatter launch) and waits.
int push_slots(lld_kfdb* db, const std::vector<int>& dirty) {
  if (dirty.empty()) return LLD_OK;
  const int m = (int)dirty.size();
  const size_t o_rec = lld_slab::pad((size_t)m * 4), bytes = o_rec + (size_t)m * sizeof(KfSlot);
  int rc = grow_stage(db, bytes);
  if (rc) return rc;
  int32_t* idx = (int32_t*)db->h_stage;
  KfSlot* rec = (KfSlot*)(db->h_stage + o_rec);
  for (int i = 0; i < m; i++) { idx[i] = dirty[i]; rec[i] = db->slots[dirty[i]].rec; }
  hipStream_t st = db->ctx->stream;
  LLD_HIP_TRY(hipMemcpyAsync(db->d_stage, db->h_stage, bytes, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(kfdb_scatter, dim3(std::min(1024, (m + 255) / 256)), dim3(256), 0, st, (const int32_t*)db->d_stage,
                     (const KfSlot*)(db->d_stage + o_rec), m, db->d_slot);
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipStreamSynchronize(st));
  return LLD_OK;
}

// Moves the vectors of the database to the front of the other pool, in slot order.
int compact(lld_kfdb* db, std::vector<int>* dirty) {
  std::vector<Move> mv;
  int64_t pos = 0;
  for (int s = 0; s < (int)db->slots.size(); s++) {
    KfSlot& r = db->slots[s].rec;
    if (!db->slots[s].in_db) continue;
    if (r.n > 0) mv.push_back(Move{r.off, (int32_t)pos, r.n});
    r.off = (int32_t)pos;
    pos += r.n;
    dirty->push_back(s);
  }
  const int src = db->pool, dst = 1 - db->pool;
  hipStream_t st = db->ctx->stream;
  if (!mv.empty()) {
    const size_t bytes = mv.size() * sizeof(Move);
    int rc = grow_stage(db, bytes);
    if (rc) return rc;
    std::memcpy(db->h_stage, mv.data(), bytes);
    LLD_HIP_TRY(hipMemcpyAsync(db->d_stage, db->h_stage, bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(kfdb_compact, dim3((unsigned)mv.size()), dim3(256), 0, st, (const Move*)db->d_stage, db->d_word[src],
                       db->d_val[src], db->d_word[dst], db->d_val[dst]);
    LLD_HIP_TRY(hipGetLastError());
    LLD_HIP_TRY(hipStreamSynchronize(st));     // the staging is rewritten by the caller next
  }
  db->pool = dst;
  db->pool_end = pos;
  return LLD_OK;
}

int run_query(lld_kfdb* db, uint64_t qid, const lld_bow_vector* q, int loop, int32_t n_conn, const uint64_t* connected, float min_score,
              lld_kfdb_result* out) {
  if (!db || !out || !words_ok(q, db->n_words) || out->capacity < 0 || (out->capacity > 0 && !out->kf_id)) return LLD_ERR_INVALID;
  if (loop && (n_conn < 0 || (n_conn > 0 && !connected))) return LLD_ERR_INVALID;
  std::vector<int32_t> cs;
  for (int i = 0; loop && i < n_conn; i++) {
    auto it = db->slot_of.find(connected[i]);
    if (it != db->slot_of.end()) cs.push_back(it->second);
  }
  const int nq = q->n, nc = (int)cs.size(), n_slots = (int)db->slots.size();
  const size_t o_qv = lld_slab::pad((size_t)nq * 4), o_cs = o_qv + lld_slab::pad((size_t)nq * 8), bytes = o_cs + (size_t)nc * 4;
  int rc = grow_stage(db, bytes);
  if (rc) return rc;
  char* h = db->h_stage;
  if (nq) { std::memcpy(h, q->word, (size_t)nq * 4); std::memcpy(h + o_qv, q->value, (size_t)nq * 8); }
  if (nc) std::memcpy(h + o_cs, cs.data(), (size_t)nc * 4);
  hipStream_t st = db->ctx->stream;
  LLD_HIP_TRY(hipSetDevice(db->ctx->device));
  if (bytes) LLD_HIP_TRY(hipMemcpyAsync(db->d_stage, h, bytes, hipMemcpyHostToDevice, st));
  const int32_t* qword = (const int32_t*)db->d_stage;
  const double* qval = (const double*)(db->d_stage + o_qv);
  const int32_t* cslot = (const int32_t*)(db->d_stage + o_cs);
  KfCounters* C = (KfCounters*)db->d_res;
  KfOut* O = (KfOut*)(db->d_res + kResHead);
  const int32_t* pw = db->d_word[db->pool];
  const double* pv = db->d_val[db->pool];
  const int pb = std::max(1, std::min(1024, (std::max(nq, nc) + 255) / 256));
  const int wb = std::max(1, (n_slots + 3) / 4);
  hipLaunchKernelGGL(kfdb_prep, dim3(pb), dim3(256), 0, st, qword, nq, cslot, nc, db->d_qpos, db->d_conn, C);
  hipLaunchKernelGGL(kfdb_walk, dim3(wb), dim3(256), 0, st, db->d_slot, n_slots, pw, db->d_qpos, db->d_conn, db->d_regs,
                     (unsigned long long)qid, loop, db->d_listed, db->d_first, C);
  hipLaunchKernelGGL(kfdb_score, dim3(wb), dim3(256), 0, st, db->d_slot, n_slots, pw, pv, db->d_qpos, qval, db->d_regs, loop, min_score,
                     db->d_listed, db->d_first, db->d_kept, C);
  const int cap = std::min(out->capacity, db->max_kf);
  hipLaunchKernelGGL(kfdb_finish, dim3(1), dim3(kFinishThreads), 0, st, db->d_slot, db->d_regs, (unsigned long long)qid, loop, min_score,
                     db->d_kept, db->d_acc, db->d_best, db->d_minkey, C, O, cap, db->d_qpos, qword, nq, db->d_conn, cslot, nc);
  LLD_HIP_TRY(hipGetLastError());
  LLD_HIP_TRY(hipMemcpyAsync(db->h_res, db->d_res, kResHead + (size_t)cap * sizeof(KfOut), hipMemcpyDeviceToHost, st));
  LLD_HIP_TRY(hipStreamSynchronize(st));
  const KfCounters& R = *(const KfCounters*)db->h_res;
  if (R.n_out < 0 || R.n_out > R.n_kept || R.n_kept > R.n_scored || R.n_scored > R.n_listed || R.n_listed > n_slots) return LLD_ERR_HIP;
  out->n_candidates = R.n_out;
  out->n_sharing = R.n_listed;
  out->max_common_words = R.max_words;
  out->min_common_words = R.n_listed ? R.min_words : 0;
  out->n_scored = R.n_scored;
  const KfOut* ho = (const KfOut*)(db->h_res + kResHead);
  const int w = std::min(R.n_out, cap);
  for (int i = 0; i < w; i++) {
    out->kf_id[i] = ho[i].id;
    if (out->acc_score) out->acc_score[i] = ho[i].acc;
  }
  return LLD_OK;
}

}  // namespace

extern "C" int lld_kfdb_create(lld_bow_vocab* voc, int32_t max_keyframes, int64_t max_words, lld_kfdb** out) {
  if (!voc || !out) return LLD_ERR_INVALID;
  *out = nullptr;
  if (max_keyframes < 1 || max_keyframes > LLD_KFDB_MAX_KEYFRAMES || max_words < 1 || max_words > INT_MAX) return LLD_ERR_INVALID;
  lld_bow_vocab_info info{};
  if (lld_bow_vocab_info_get(voc, &info) != LLD_OK) return LLD_ERR_INVALID;
  lld_kfdb* db = new lld_kfdb();
  db->ctx = lld_bow_vocab_context(voc);
  db->n_words = info.n_words;
  db->max_kf = max_keyframes;
  db->max_words = max_words;
  const size_t K = (size_t)max_keyframes, W = (size_t)max_words;
  const size_t res_bytes = kResHead + K * sizeof(KfOut);
  const size_t bytes = lld_slab::pad(K * sizeof(KfSlot)) + lld_slab::pad(K * sizeof(KfRegs)) + lld_slab::pad(K * 8) + 4 * lld_slab::pad(K * 4) +
                       lld_slab::pad(K * 4) + lld_slab::pad(K * sizeof(KfKept)) + lld_slab::pad(res_bytes) +
                       lld_slab::pad((size_t)info.n_words * 4) + 2 * (lld_slab::pad(W * 4) + lld_slab::pad(W * 8));
  hipStream_t st = db->ctx->stream;
  if (hipSetDevice(db->ctx->device) != hipSuccess || hipMalloc(&db->dmem, bytes) != hipSuccess) { db->dmem = nullptr; lld_kfdb_destroy(db); return LLD_ERR_ALLOC; }
  if (hipHostMalloc((void**)&db->h_res, res_bytes, hipHostMallocDefault) != hipSuccess) { db->h_res = nullptr; lld_kfdb_destroy(db); return LLD_ERR_ALLOC; }
  lld_slab S; S.base = (char*)db->dmem; S.size = bytes;
  db->d_slot = S.take<KfSlot>(K);
  db->d_regs = S.take<KfRegs>(K);
  db->d_minkey = S.take<unsigned long long>(K);
  db->d_conn = S.take<int32_t>(K); db->d_listed = S.take<int32_t>(K); db->d_first = S.take<int32_t>(K); db->d_best = S.take<int32_t>(K);
  db->d_acc = S.take<float>(K);
  db->d_kept = S.take<KfKept>(K);
  db->d_res = S.take<char>(res_bytes);
  db->d_qpos = S.take<int32_t>(info.n_words);
  for (int p = 0; p < 2; p++) { db->d_word[p] = S.take<int32_t>(W); db->d_val[p] = S.take<double>(W); }
  if (S.used > S.size) { lld_kfdb_destroy(db); return LLD_ERR_ALLOC; }
  // registers start at 0 (KeyFrame.cc:38; the scores too, see the deviation in the header); qpos -1, min-keys all ones
  if (hipMemsetAsync(db->d_slot, 0, K * sizeof(KfSlot), st) != hipSuccess || hipMemsetAsync(db->d_regs, 0, K * sizeof(KfRegs), st) != hipSuccess ||
      hipMemsetAsync(db->d_minkey, 0xFF, K * 8, st) != hipSuccess || hipMemsetAsync(db->d_conn, 0, K * 4, st) != hipSuccess ||
      hipMemsetAsync(db->d_qpos, 0xFF, (size_t)info.n_words * 4, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    lld_kfdb_destroy(db);
    return LLD_ERR_HIP;
  }
  *out = db;
  return LLD_OK;
}

extern "C" void lld_kfdb_destroy(lld_kfdb* db) {
  if (!db) return;
  if (db->dmem) (void)hipFree(db->dmem);
  if (db->d_stage) (void)hipFree(db->d_stage);
  if (db->h_stage) (void)hipHostFree(db->h_stage);
  if (db->h_res) (void)hipHostFree(db->h_res);
  delete db;
}

extern "C" int lld_kfdb_add(lld_kfdb* db, int32_t n, const uint64_t* kf_id, const lld_bow_vector* vecs) {
  if (!db || n < 0 || (n > 0 && (!kf_id || !vecs))) return LLD_ERR_INVALID;
  if (n == 0) return LLD_OK;
  std::unordered_set<uint64_t> seen;
  int64_t total = 0;
  for (int i = 0; i < n; i++) {
    if (!words_ok(&vecs[i], db->n_words)) return LLD_ERR_INVALID;
    auto it = db->slot_of.find(kf_id[i]);
    if ((it != db->slot_of.end() && db->slots[it->second].in_db) || !seen.insert(kf_id[i]).second) return LLD_ERR_INVALID;
    total += vecs[i].n;
  }
  if ((int64_t)db->slots.size() + new_slots(db, std::vector<uint64_t>(kf_id, kf_id + n)) > db->max_kf) return LLD_ERR_INVALID;
  if (db->live + total > db->max_words) return LLD_ERR_INVALID;
  LLD_HIP_TRY(hipSetDevice(db->ctx->device));
  std::vector<int> dirty;
  int rc;
  if (db->pool_end + total > db->max_words && (rc = compact(db, &dirty))) return rc;
  if ((uint64_t)db->next_seq + (uint64_t)n > UINT32_MAX) {       // renumber the database in add order
    std::vector<std::pair<uint32_t, int>> order;
    for (int s = 0; s < (int)db->slots.size(); s++)
      if (db->slots[s].in_db) order.push_back({db->slots[s].rec.seq, s});
    std::sort(order.begin(), order.end());
    for (size_t k = 0; k < order.size(); k++) { db->slots[order[k].second].rec.seq = (uint32_t)k; dirty.push_back(order[k].second); }
    db->next_seq = (uint32_t)order.size();
  }
  const size_t o_val = lld_slab::pad((size_t)total * 4), bytes = o_val + (size_t)total * 8;
  if ((rc = grow_stage(db, bytes))) return rc;
  int64_t pos = 0;
  for (int i = 0; i < n; i++) {
    const int s = slot_for(db, kf_id[i]);
    SlotHost& h = db->slots[s];
    h.in_db = true;
    h.rec.off = (int32_t)(db->pool_end + pos);
    h.rec.n = vecs[i].n;
    h.rec.seq = db->next_seq++;
    if (vecs[i].n) {
      std::memcpy(db->h_stage + pos * 4, vecs[i].word, (size_t)vecs[i].n * 4);
      std::memcpy(db->h_stage + o_val + pos * 8, vecs[i].value, (size_t)vecs[i].n * 8);
    }
    pos += vecs[i].n;
    dirty.push_back(s);
  }
  hipStream_t st = db->ctx->stream;
  if (total) {
    LLD_HIP_TRY(hipMemcpyAsync(db->d_word[db->pool] + db->pool_end, db->h_stage, (size_t)total * 4, hipMemcpyHostToDevice, st));
    LLD_HIP_TRY(hipMemcpyAsync(db->d_val[db->pool] + db->pool_end, db->h_stage + o_val, (size_t)total * 8, hipMemcpyHostToDevice, st));
    LLD_HIP_TRY(hipStreamSynchronize(st));     // push_slots rewrites the staging
  }
  db->pool_end += total;
  db->live += total;
  return push_slots(db, dirty);
}

extern "C" int lld_kfdb_erase(lld_kfdb* db, int32_t n, const uint64_t* kf_id) {
  if (!db || n < 0 || (n > 0 && !kf_id)) return LLD_ERR_INVALID;
  std::vector<int> dirty;
  for (int i = 0; i < n; i++) {
    auto it = db->slot_of.find(kf_id[i]);
    if (it == db->slot_of.end() || !db->slots[it->second].in_db) continue;      // not in the database: nothing to erase
    SlotHost& h = db->slots[it->second];
    if ((int64_t)h.rec.off + h.rec.n == db->pool_end) db->pool_end = h.rec.off;    // the last vector: its space is reused at once
    db->live -= h.rec.n;
    h.in_db = false;
    h.rec.n = 0;
    dirty.push_back(it->second);
  }
  if (db->live == 0) db->pool_end = 0;
  LLD_HIP_TRY(hipSetDevice(db->ctx->device));
  return push_slots(db, dirty);
}

extern "C" int lld_kfdb_clear(lld_kfdb* db) {
  if (!db) return LLD_ERR_INVALID;
  std::vector<int> dirty;
  for (int s = 0; s < (int)db->slots.size(); s++)
    if (db->slots[s].in_db) { db->slots[s].in_db = false; db->slots[s].rec.n = 0; dirty.push_back(s); }
  db->live = 0;
  db->pool_end = 0;
  LLD_HIP_TRY(hipSetDevice(db->ctx->device));
  return push_slots(db, dirty);
}

extern "C" int lld_kfdb_set_covisibles(lld_kfdb* db, int32_t n, const uint64_t* kf_id, const int32_t* start, const uint64_t* neighbour) {
  if (!db || n < 0 || (n > 0 && (!kf_id || !start))) return LLD_ERR_INVALID;
  if (n == 0) return LLD_OK;
  if (start[0] < 0) return LLD_ERR_INVALID;
  std::vector<uint64_t> ids;
  for (int i = 0; i < n; i++) {
    if (start[i + 1] < start[i]) return LLD_ERR_INVALID;
    if (start[i + 1] > start[i] && !neighbour) return LLD_ERR_INVALID;
    ids.push_back(kf_id[i]);
    for (int j = start[i]; j < std::min(start[i + 1], start[i] + kNb); j++) ids.push_back(neighbour[j]);
  }
  if ((int64_t)db->slots.size() + new_slots(db, ids) > db->max_kf) return LLD_ERR_INVALID;
  std::vector<int> dirty;
  const int before = (int)db->slots.size();
  for (int i = 0; i < n; i++) {
    const int s = slot_for(db, kf_id[i]);
    const int m = std::min(start[i + 1] - start[i], kNb);
    int nb[kNb];
    for (int j = 0; j < m; j++) nb[j] = slot_for(db, neighbour[start[i] + j]);
    KfSlot& r = db->slots[s].rec;
    r.nnb = m;
    for (int j = 0; j < kNb; j++) r.nb[j] = j < m ? nb[j] : -1;
    dirty.push_back(s);
  }
  for (int s = before; s < (int)db->slots.size(); s++) dirty.push_back(s);     // new neighbour slots: their ids
  LLD_HIP_TRY(hipSetDevice(db->ctx->device));
  return push_slots(db, dirty);
}

extern "C" int lld_kfdb_detect_loop_candidates(lld_kfdb* db, uint64_t query_id, const lld_bow_vector* q, int32_t n_connected,
                                               const uint64_t* connected, float min_score, lld_kfdb_result* out) {
  return run_query(db, query_id, q, 1, n_connected, connected, min_score, out);
}

extern "C" int lld_kfdb_detect_relocalization_candidates(lld_kfdb* db, uint64_t query_id, const lld_bow_vector* q, lld_kfdb_result* out) {
  return run_query(db, query_id, q, 0, 0, nullptr, 0.0f, out);
}
