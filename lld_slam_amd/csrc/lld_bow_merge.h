// lld_bow_merge.h — the device bodies of ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (src/ORBmatcher.cc:159-288) shared by
// the one-keyframe stage (lld_frame_track_bow.hip) and the batched one of Tracking::Relocalization (lld_frame_reloc.hip).
//
// The reference walks the common nodes of the two FeatureVectors in ascending node id (:180-264).  Inside a node every keyframe feature with
// a good MapPoint, in list order, scans the node's frame features in list order, skipping those an earlier keyframe feature took (:209-210),
// and keeps best and second best with strict `<` (:216-225).  A frame feature belongs to exactly one node, so nodes are independent and the
// only order dependence is inside a node:
//
//   bow_match_node       one wavefront per keyframe node.  It finds its node id in the frame's node list (binary search: the merge-join, on
//                        the device, of a FeatureVector that never left HBM), then goes serially over the node's keyframe features while its
//                        lanes hold the node's frame features (chunks of 64 when a node has more; the first chunk's descriptors stay in
//                        registers).  Occupancy is one bit per chunk in a lane register; the keyframe side is read 64 features at a time
//                        into registers and broadcast lane by lane, so no global load sits on the serial path of a node of up to 64 + 64
//                        features.  Exact in one pass.
//   bow_finish_block     one workgroup after all nodes: the rotation histogram of the accepted matches (:236-246), ComputeThreeMaxima
//                        (:1601-1642), the removal of the other bins (:267-285), and vpMapPointMatches written into the tables of `A`.
#ifndef LLD_BOW_MERGE_H
#define LLD_BOW_MERGE_H

#include "lld_common.h"
#include "lld_track_internal.h"
#include "lld_wave.h"

namespace lld_bow_merge {

using lld_track::ApplyDev;
using lld_track::BowSearchDev;

constexpr int kHisto = 30;                       // HISTO_LENGTH, src/ORBmatcher.cc:39
constexpr int kThLow = 50;                       // TH_LOW, :37
constexpr int kPosBits = 12;                     // position of a frame feature inside its node: < LLD_ORB_MAX_KEYPOINTS
constexpr unsigned kNone = (256u << kPosBits) | ((1u << kPosBits) - 1);   // bestDist = 256, no index
constexpr int kMatchWaves = 4;
constexpr int kFinishThreads = 1024;
constexpr int kFinishPerThread = LLD_ORB_MAX_KEYPOINTS / kFinishThreads;
static_assert((1 << kPosBits) >= LLD_ORB_MAX_KEYPOINTS, "position bits");
static_assert(LLD_ORB_MAX_KEYPOINTS <= 64 * 64, "one occupancy bit per chunk of 64 frame features in a 64-bit lane register");

__device__ __forceinline__ uint4 bcast(const uint4& v, int src) {
  return make_uint4((unsigned)__shfl((int)v.x, src), (unsigned)__shfl((int)v.y, src), (unsigned)__shfl((int)v.z, src), (unsigned)__shfl((int)v.w, src));
}

// keyframe node `w` of B on the calling wavefront (whole wavefronts only: nothing here synchronises the workgroup)
__device__ __forceinline__ void bow_match_node(const BowSearchDev& B, int w, int lane) {
  // KFit->first == Fit->first: the keyframe node's place in the frame's ascending node list, if it has one
  const int nid = B.kf_node[w];
  int lo = 0, hi = *B.f_n_nodes;
  const int fn = hi;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (B.f_node[mid] < nid) lo = mid + 1; else hi = mid;
  }
  if (lo >= fn || B.f_node[lo] != nid) return;
  const int fs = B.f_node_start[lo], nf = B.f_node_start[lo + 1] - fs;
  const int ks = B.kf_node_start[w], nk = B.kf_node_start[w + 1] - ks;
  if (nf <= 0 || nk <= 0) return;
  const uint4* fdesc = reinterpret_cast<const uint4*>(B.f_desc);
  const uint4* kdesc = reinterpret_cast<const uint4*>(B.kf_desc);
  // the first 64 frame features of the node: index and descriptor stay in registers
  int idx0 = 0;
  uint4 a0 = make_uint4(0, 0, 0, 0), b0 = a0;
  if (lane < nf) { idx0 = B.f_feature[fs + lane]; a0 = fdesc[2 * (size_t)idx0]; b0 = fdesc[2 * (size_t)idx0 + 1]; }
  unsigned long long occ = 0;                    // bit c: vpMapPointMatches[the lane's frame feature of chunk c] is set
  const int n_chunks = (nf + 63) >> 6;
  for (int k0 = 0; k0 < nk; k0 += 64) {
    // 64 keyframe features at a time, one per lane
    int rk_l = 0, pid_l = -1;
    uint4 ka = make_uint4(0, 0, 0, 0), kb = ka;
    if (k0 + lane < nk) {
      rk_l = B.kf_feature[ks + k0 + lane];
      pid_l = B.kf_point_id[rk_l];
      ka = kdesc[2 * (size_t)rk_l]; kb = kdesc[2 * (size_t)rk_l + 1];
    }
    const int cnt = min(64, nk - k0);
    for (int j = 0; j < cnt; j++) {
      if (__shfl(pid_l, j) < 0) continue;        // if(!pMP) continue; if(pMP->isBad()) continue;  (:193-197)
      const int rk = __shfl(rk_l, j);
      const uint4 da = bcast(ka, j), db = bcast(kb, j);
      unsigned b1 = kNone, b2 = 256;             // (bestDist1 << kPosBits | position), bestDist2
      for (int c = 0; c < n_chunks; c++) {
        const int p = (c << 6) + lane;
        if (p >= nf || ((occ >> c) & 1ull)) continue;
        unsigned dist;
        if (c == 0) dist = lld_wave::hamming256(a0, b0, da, db);
        else {
          const int idx = B.f_feature[fs + p];
          dist = lld_wave::hamming256(fdesc[2 * (size_t)idx], fdesc[2 * (size_t)idx + 1], da, db);
        }
        // strict < for both, ascending position inside the lane (:216-225); dist = 256 can pass neither test
        if (dist < (b1 >> kPosBits)) { b2 = b1 >> kPosBits; b1 = (dist << kPosBits) | (unsigned)p; }
        else if (dist < b2) b2 = dist;
      }
      // across lanes: the smaller key is the smaller distance, then the earlier position (the first candidate in order wins a tie); the second
      // best is the second smallest distance of the whole list, whatever the order
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned o1 = (unsigned)__shfl_xor((int)b1, o), o2 = (unsigned)__shfl_xor((int)b2, o);
        const unsigned loser = max(b1, o1) >> kPosBits;
        b1 = min(b1, o1); b2 = min(min(b2, o2), loser);
      }
      const int bd1 = (int)(b1 >> kPosBits);
      if (bd1 <= kThLow && (float)bd1 < __fmul_rn(B.nnratio, (float)(int)b2)) {          // :228-230
        const int p = (int)(b1 & ((1u << kPosBits) - 1));
        if ((p & 63) == lane) {
          occ |= 1ull << (p >> 6);
          const int idx = (p < 64) ? idx0 : B.f_feature[fs + p];
          B.taken[idx] = rk;                     // vpMapPointMatches[bestIdxF] = pMP
        }
      }
    }
  }
}

// The calling workgroup (kFinishThreads lanes) finishes the search B: hist [kHisto] and ctl [4] are its LDS.
__device__ __forceinline__ void bow_finish_block(const BowSearchDev& B, const ApplyDev& A, int* hist, int* ctl) {
  const int tid = threadIdx.x;
  if (tid < kHisto) hist[tid] = 0;
  if (tid < 4) ctl[tid] = tid == 0 ? 0 : -1;     // n kept, ind1, ind2, ind3
  __syncthreads();
  int kf[kFinishPerThread], bin[kFinishPerThread];
#pragma unroll
  for (int e = 0; e < kFinishPerThread; e++) {
    const int k = e * kFinishThreads + tid;
    kf[e] = k < B.nt ? B.taken[k] : -1;
    bin[e] = -1;
    if (kf[e] >= 0 && B.check_orientation) {     // :236-246
      float rot = __fsub_rn(B.kf_angle[kf[e]], B.f_angle[k]);
      if (rot < 0.f) rot = __fadd_rn(rot, 360.0f);
      int b = (int)roundf(__fmul_rn(rot, 1.0f / kHisto));
      if (b == kHisto) b = 0;
      b = min(max(b, 0), kHisto - 1);            // the reference asserts the range
      bin[e] = b;
      atomicAdd(&hist[b], 1);
    }
  }
  __syncthreads();
  if (tid == 0 && B.check_orientation) {         // ComputeThreeMaxima, :1601-1642
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < kHisto; i++) {
      const int s = hist[i];
      if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
      else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
      else if (s > max3) { max3 = s; ind3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { ind3 = -1; }
    ctl[1] = ind1; ctl[2] = ind2; ctl[3] = ind3;
  }
  __syncthreads();
  int kept = 0;
#pragma unroll
  for (int e = 0; e < kFinishPerThread; e++) {
    const int q = kf[e];
    if (q < 0) continue;
    if (B.check_orientation && bin[e] != ctl[1] && bin[e] != ctl[2] && bin[e] != ctl[3]) continue;   // :275-284
    const int k = e * kFinishThreads + tid;
    A.kp_has[k] = 1; A.kp_id[k] = A.q_id[q]; A.kp_obs[k] = A.q_obs ? A.q_obs[q] : 1;
    A.kp_world[3 * k] = A.q_pos[3 * q]; A.kp_world[3 * k + 1] = A.q_pos[3 * q + 1]; A.kp_world[3 * k + 2] = A.q_pos[3 * q + 2];
    kept++;
  }
  kept = lld_wave::sum(kept);
  if ((tid & 63) == 0 && kept) atomicAdd(&ctl[0], kept);
  __syncthreads();
  if (tid == 0) { A.counts[0] = ctl[0]; A.counts[1] = ctl[0]; A.counts[2] = 0; }
}

}  // namespace lld_bow_merge

#endif
