// lld_localmapping_adapter.cc — see lld_localmapping_adapter.h.
#include "lld_localmapping_adapter.h"

#include <cmath>
#include <utility>

namespace lld_adapter {

namespace {

using lld_slam::Mat;

// C (3 x n) = A (3 x 3) * B (3 x n): the float products summed in double in index order from the first, rounded to float once
Mat mul3(const Mat& A, const Mat& B) {
  Mat C(3, B.cols);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < B.cols; j++) {
      double s = (double)A.at<float>(i, 0) * (double)B.at<float>(0, j);
      for (int k = 1; k < 3; k++) s += (double)A.at<float>(i, k) * (double)B.at<float>(k, j);
      C.at<float>(i, j) = (float)s;
    }
  return C;
}

Mat transpose3(const Mat& A) {
  Mat T(3, 3);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) T.at<float>(i, j) = A.at<float>(j, i);
  return T;
}

// Mat::inv() of a float 3x3: the cofactors times 1/det in double, rounded; det == 0 gives the zero matrix
Mat inv3(const Mat& A) {
  const double a0 = A.at<float>(0), a1 = A.at<float>(1), a2 = A.at<float>(2), a3 = A.at<float>(3), a4 = A.at<float>(4), a5 = A.at<float>(5),
               a6 = A.at<float>(6), a7 = A.at<float>(7), a8 = A.at<float>(8);
  const double det = (a0 * (a4 * a8 - a5 * a7) - a1 * (a3 * a8 - a5 * a6)) + a2 * (a3 * a7 - a4 * a6);
  Mat o(3, 3);
  if (det == 0.0) return o;
  const double d = 1.0 / det;
  const double cof[9] = {(a4 * a8 - a5 * a7), (a2 * a7 - a1 * a8), (a1 * a5 - a2 * a4), (a5 * a6 - a3 * a8), (a0 * a8 - a2 * a6),
                         (a2 * a3 - a0 * a5), (a3 * a7 - a4 * a6), (a1 * a6 - a0 * a7), (a0 * a4 - a1 * a3)};
  for (int q = 0; q < 9; q++) o.at<float>(q) = (float)(cof[q] * d);
  return o;
}

void fill_record(const KeyFrame* pKF, float median_depth, lld_new_points_kf* r) {
  *r = lld_new_points_kf();
  const Mat R = pKF->GetRotation(), t = pKF->GetTranslation();
  for (int q = 0; q < 9; q++) r->Rcw[q] = R.at<float>(q);
  for (int q = 0; q < 3; q++) r->tcw[q] = t.at<float>(q);
  r->fx = pKF->fx; r->fy = pKF->fy; r->cx = pKF->cx; r->cy = pKF->cy; r->mb = pKF->mb; r->mbf = pKF->mbf;
  r->scale_factor = pKF->mfScaleFactor; r->median_depth = median_depth;
  const size_t n = pKF->mvScaleFactors.size() < (size_t)LLD_ORB_MAX_LEVELS ? pKF->mvScaleFactors.size() : (size_t)LLD_ORB_MAX_LEVELS;
  r->n_levels = (int32_t)pKF->mvScaleFactors.size();                          // above LLD_ORB_MAX_LEVELS the library refuses the call
  for (size_t q = 0; q < n; q++) { r->scale_factors[q] = pKF->mvScaleFactors[q]; r->level_sigma2[q] = pKF->mvLevelSigma2[q]; }
}

void fill_keys(const KeyFrame* pKF, lld_amd::NewPointsKeys* k) {
  const size_t n = pKF->mvKeysUn.size();
  k->xy.resize(2 * n); k->raw_xy.resize(2 * n); k->octave.resize(n);
  for (size_t i = 0; i < n; i++) {
    k->xy[2 * i] = pKF->mvKeysUn[i].pt.x; k->xy[2 * i + 1] = pKF->mvKeysUn[i].pt.y;
    k->raw_xy[2 * i] = pKF->mvKeys[i].pt.x; k->raw_xy[2 * i + 1] = pKF->mvKeys[i].pt.y;
    k->octave[i] = pKF->mvKeysUn[i].octave;
  }
  k->ur = pKF->mvuRight; k->depth = pKF->mvDepth;
}

}  // namespace

Mat ComputeF12(KeyFrame*& pKF1, KeyFrame*& pKF2) {
  const Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation(), R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
  const Mat R12 = mul3(R1w, transpose3(R2w));                                 // R1w*R2w.t()
  Mat t12 = mul3(R12, t2w);                                                   // -R1w*R2w.t()*t2w+t1w
  for (int r = 0; r < 3; r++) t12.at<float>(r) = -t12.at<float>(r) + t1w.at<float>(r);
  Mat t12x(3, 3);                                                             // SkewSymmetricMatrix (:665-672)
  t12x.at<float>(0, 1) = -t12.at<float>(2); t12x.at<float>(0, 2) = t12.at<float>(1);
  t12x.at<float>(1, 0) = t12.at<float>(2); t12x.at<float>(1, 2) = -t12.at<float>(0);
  t12x.at<float>(2, 0) = -t12.at<float>(1); t12x.at<float>(2, 1) = t12.at<float>(0);
  return mul3(mul3(mul3(inv3(transpose3(pKF1->mK)), t12x), R12), inv3(pKF2->mK));   // K1.t().inv()*t12x*R12*K2.inv()
}

int CreateNewMapPoints(const lld_amd::Context& ctx, KeyFrame* mpCurrentKeyFrame, Map* mpMap, bool mbMonocular,
                       std::list<MapPoint*>& mlpRecentAddedMapPoints, const std::function<bool()>& CheckNewKeyFrames, NewPointsTrace* trace) {
  // Retrieve neighbor keyframes in covisibility graph (:211-214)
  int nn = 10;
  if (mbMonocular) nn = 20;
  const std::vector<KeyFrame*> vpNeighKFs = mpCurrentKeyFrame->GetBestCovisibilityKeyFrames(nn);

  ORBmatcher matcher(ctx.get(), 0.6f, false);

  lld_amd::NewPointsBatch b;
  fill_record(mpCurrentKeyFrame, 0.f, &b.kf1);
  b.monocular = mbMonocular;
  fill_keys(mpCurrentKeyFrame, &b.keys1);
  b.kf2.resize(1); b.key_start.assign(2, 0); b.match_start.assign(2, 0);
  const Mat Ow1 = mpCurrentKeyFrame->GetCameraCenter();

  int nnew = 0;
  std::vector<MapPoint*> vpNew;

  // Search matches with epipolar restriction and triangulate
  for (size_t i = 0; i < vpNeighKFs.size(); i++) {
    if (i > 0 && CheckNewKeyFrames()) {                                         // :240-241
      if (trace) trace->returned_early = true;
      break;
    }
    KeyFrame* pKF2 = vpNeighKFs[i];

    // Check first that baseline is not too short (:245-262); the library applies the same rule to the pair
    const Mat Ow2 = pKF2->GetCameraCenter();
    const float vBaseline[3] = {Ow2.at<float>(0) - Ow1.at<float>(0), Ow2.at<float>(1) - Ow1.at<float>(1), Ow2.at<float>(2) - Ow1.at<float>(2)};
    double s = (double)vBaseline[0] * (double)vBaseline[0];
    s += (double)vBaseline[1] * (double)vBaseline[1];
    s += (double)vBaseline[2] * (double)vBaseline[2];
    const float baseline = (float)std::sqrt(s);
    float medianDepthKF2 = 0.f;
    bool skip;
    if (!mbMonocular) skip = baseline < pKF2->mb;
    else {
      medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
      const float ratioBaselineDepth = baseline / medianDepthKF2;
      skip = ratioBaselineDepth < 0.01;
    }
    if (trace) { trace->skipped.push_back(skip ? 1 : 0); trace->n_matches.push_back(0); trace->n_new.push_back(0); }
    if (skip) continue;

    // Compute Fundamental Matrix (:265)
    const Mat F12 = ComputeF12(mpCurrentKeyFrame, pKF2);

    // Search matches that fullfil epipolar constraint (:268-269)
    std::vector<std::pair<size_t, size_t> > vMatchedIndices;
    matcher.SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, vMatchedIndices, false);
    const int nmatches = (int)vMatchedIndices.size();
    if (trace) trace->n_matches.back() = nmatches;
    if (nmatches == 0) continue;

    // Triangulate each match (:287-432): one call, one pair
    fill_record(pKF2, medianDepthKF2, &b.kf2[0]);
    fill_keys(pKF2, &b.keys2);
    b.key_start[1] = (int32_t)pKF2->mvKeysUn.size();
    b.match_start[1] = nmatches;
    b.matches.resize(2 * (size_t)nmatches);
    for (int ikp = 0; ikp < nmatches; ikp++) {
      b.matches[2 * ikp] = (int32_t)vMatchedIndices[ikp].first;
      b.matches[2 * ikp + 1] = (int32_t)vMatchedIndices[ikp].second;
    }
    lld_amd::NewPointsOutput o;
    lld_amd::TriangulateNewPoints(ctx, b, o);

    for (size_t q = 0; q < o.new_match.size(); q++) {                           // Triangulation is succesfull (:434-450)
      const int ikp = o.new_match[q];
      const int idx1 = (int)vMatchedIndices[ikp].first, idx2 = (int)vMatchedIndices[ikp].second;
      const Mat x3D(3, 1, &o.x3d[3 * (size_t)ikp]);
      MapPoint* pMP = new MapPoint(x3D, mpCurrentKeyFrame, mpMap);

      pMP->AddObservation(mpCurrentKeyFrame, idx1);
      pMP->AddObservation(pKF2, idx2);

      mpCurrentKeyFrame->AddMapPoint(pMP, idx1);
      pKF2->AddMapPoint(pMP, idx2);

      vpNew.push_back(pMP);                                                     // ComputeDistinctiveDescriptors / UpdateNormalAndDepth: below

      mpMap->AddMapPoint(pMP);
      mlpRecentAddedMapPoints.push_back(pMP);

      nnew++;
    }
    if (trace) trace->n_new.back() = (int)o.new_match.size();
  }
  RefreshMapPoints(ctx, vpNew, LLD_LANDMARK_DESCRIPTOR | LLD_LANDMARK_NORMAL_DEPTH);   // :443-445 for all new points
  return nnew;
}

}  // namespace lld_adapter
