// lld_covis_lists.h — what the two covisibility calls share from "the connected keyframes of query q with their weights are known" onward
// (lld_covisibility on flat tables, lld_covisibility.hip; lld_map_covisibility on the resident map, lld_map_covis.hip): the staged and packed
// lists as one device argument block (Lists), the culling tally's gate and verdict, the pack kernel behind pack_launch, and on the host the
// validation of a lld_covisibility_out, the layout of outputs and scratch on an UploadBlock, the timed upload / launches / download
// (lld_round_trip.h's, with the pack kernel behind the query kernel) and the copy-back.  Everything that is not inline here is defined
// once, in lld_covisibility.hip.  Nothing here is exported.
//
// A query kernel owes the pack kernel, per query q with off = stage_off[q]: cnt_conn[q] connected keyframes in list order in st_kf / st_w
// [off, off + cnt_conn), and cnt_ord[q] keys weight << 32 | rank in st_key [off, ...) in the order they go out, rank being the position in
// st_kf; besides n_max, kf_max, updated (and n_mps, n_red, redundant through publish_cull), which are outputs already.
#ifndef LLD_COVIS_LISTS_H
#define LLD_COVIS_LISTS_H

#include "lld_common.h"
#include "lld_round_trip.h"
#include "lld_upload_block.h"

namespace lld_covis {

using lld_track::Span;
using lld_track::UploadBlock;
typedef unsigned long long u64;

struct Lists {
  const int32_t* stage_off;                  // [n_queries+1] the staging range of each query
  int32_t n_queries;
  int32_t* st_kf; int32_t* st_w; u64* st_key;                               // staging
  int32_t* cnt_conn; int32_t* cnt_ord; int32_t* n_max; int32_t* kf_max; uint8_t* updated;
  int32_t* n_mps; int32_t* n_red; uint8_t* redundant;
  int32_t cap_conn, cap_ord;
  int32_t* conn_start; int32_t* ord_start; int32_t* totals;                 // packed outputs
  int32_t* conn_kf; int32_t* conn_w; int32_t* ord_kf; int32_t* ord_w;
};

// KeyFrameCulling counts a map point of the keyframe when the sensor is monocular or its depth is known and inside mThDepth
__device__ __forceinline__ bool depth_counts(int monocular, float depth, float th_depth) { return monocular || !(depth > th_depth || depth < 0.f); }
// ... and the keyframe is redundant when nRedundantObservations > 0.9*nMPs: int against double
__device__ __forceinline__ void publish_cull(const Lists& L, int q, int nm, int nr, double ratio) {
  L.n_mps[q] = nm; L.n_red[q] = nr;
  L.redundant[q] = ((double)nr > ratio * (double)nm) ? 1 : 0;
}

// LLD_ERR_INVALID when `out` lacks an array the flags ask for
int check_out(const lld_covisibility_out* out, bool conn, bool cull);
// one workgroup per query: conn_start / ord_start / totals from the per-query counts, then the staged lists to their packed places
void pack_launch(hipStream_t st, const Lists& L);

// The shared arrays of one call on the caller's UploadBlock.  The caller declares its own inputs, then outputs(); its own outputs, then
// scratch(); its own scratch, then bind().  So the downloaded range [out_off, out_off + out_bytes) is one piece with the caller's outputs in it.
struct Plan {
  bool conn = false, cull = false;
  int32_t nq = 0, cap_conn = 0, cap_ord = 0;
  size_t stage_total = 0, out_off = 0, out_bytes = 0;
  Span<int32_t> stage_off, conn_start, ord_start, totals, n_max, kf_max, n_mps, n_red, conn_kf, conn_w, ord_kf, ord_w, cnt_conn, cnt_ord, st_kf, st_w;
  Span<uint8_t> updated, redundant;
  Span<u64> st_key;
  // stage_total: the sum of the staging ranges (0 without conn); it also bounds what the device can pack, so the capacities sent are cut to it
  void outputs(UploadBlock& B, const lld_covisibility_out* out, bool conn, bool cull, int32_t nq, long long stage_total);
  void scratch(UploadBlock& B);
  // the context's pinned and device blocks under B, stage_off (nq + 1 entries, read with conn only) staged, every pointer of L set
  int bind(lld_ctx* ctx, UploadBlock& B, const int32_t* stage_off_host, Lists& L) const;
  // LLD_ERR_INVALID with only n_conn / n_ordered written when a capacity is short
  int copy_back(const UploadBlock& B, lld_covisibility_out* out) const;
};

// One upload, launch_query(stream), the pack kernel (conn), one download, then the stream is waited for (lld_round_trip.h).  phase_ms, when
// given, receives the HIP-event times of upload, kernels and download.
template <class LaunchQuery>
int run(hipStream_t sm, const UploadBlock& B, const Plan& P, const Lists& L, float* phase_ms, LaunchQuery launch_query) {
  return lld_rt::round_trip(sm, B, P.out_off, P.out_bytes, phase_ms, [&](hipStream_t s) {
    launch_query(s);
    if (P.conn) pack_launch(s, L);
    return LLD_OK;
  });
}

}  // namespace lld_covis

#endif
