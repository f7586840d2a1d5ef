// lld_bow_score.h — L1Scoring::score of one candidate BowVector against a query held in a qpos table, by one wavefront.  Shared by
// lld_bow_score (lld_bow.hip) and the keyframe database (lld_kfdb.hip), so both run the same arithmetic.
#ifndef LLD_BOW_SCORE_H
#define LLD_BOW_SCORE_H

#include <hip/hip_runtime.h>

#include <cstdint>

__device__ inline double lld_readlane_f64(double x, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
  return __hiloint2double(hi, lo);
}

// ScoringObject.cpp:23-66 with v1 = query, v2 = candidate words cword/cval[s, e) (strictly ascending).  qpos[word] is the word's
// position in qval, -1 for a word the query lacks.  All 64 lanes of the wavefront call it with the same s and e; the common-word
// terms are computed in parallel and summed by every lane in ascending candidate position (= ascending word id), then -score/2.0.
// The result is the same on every lane.
__device__ inline double lld_bow_l1_score_wave(const int32_t* __restrict__ qpos, const double* __restrict__ qval,
                                               const int32_t* __restrict__ cword, const double* __restrict__ cval, int s, int e,
                                               int lane) {
  double score = 0.0;
  for (int base = s; base < e; base += 64) {
    const int j = base + lane;
    bool common = false;
    double term = 0.0;
    if (j < e) {
      const int p = qpos[cword[j]];
      if (p >= 0) {
        const double vi = qval[p], wi = cval[j];
        term = fabs(vi - wi) - fabs(vi) - fabs(wi);
        common = true;
      }
    }
    unsigned long long m = __ballot(common);
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      score += lld_readlane_f64(term, b);
    }
  }
  return -score / 2.0;
}

#endif
