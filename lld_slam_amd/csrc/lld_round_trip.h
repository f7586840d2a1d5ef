// lld_round_trip.h — one call on one UploadBlock (lld_upload_block.h) as every single-shot entry point runs it: one upload, the caller's
// launches, one download, one wait, and the HIP-event times of the three for the callers that report phase_ms.  The covisibility calls
// (lld_covis_lists.h), the resident map's window, apply and refresh calls and the landmark calls of lld_landmark.hip go through it.
// Host code; nothing here is exported.
#ifndef LLD_ROUND_TRIP_H
#define LLD_ROUND_TRIP_H

#include <algorithm>

#include "lld_common.h"
#include "lld_upload_block.h"

namespace lld_rt {

using lld_track::Span;
using lld_track::UploadBlock;

struct Events {                              // destroyed on every way out
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  ~Events() { for (int k = 0; k < 4; ++k) if (e[k]) (void)hipEventDestroy(e[k]); }
};

// Upload B.up_bytes, launch(stream) - which returns a status, so a memset the kernels need can sit in it -, download
// [down_off, down_off + down_bytes) of the block, then the stream is waited for.  phase_ms, when given, receives the HIP-event times of
// upload, launches and download.
template <class Launch>
int round_trip(hipStream_t sm, const UploadBlock& B, size_t down_off, size_t down_bytes, float* phase_ms, Launch launch) {
  Events events;
  hipEvent_t* ev = events.e;
  const bool timed = phase_ms != nullptr;
  if (timed) for (int k = 0; k < 4; ++k) LLD_HIP_TRY(hipEventCreate(&ev[k]));
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[0], sm));
  LLD_HIP_TRY(hipMemcpyAsync(B.d, B.h, B.up_bytes, hipMemcpyHostToDevice, sm));
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[1], sm));
  const int st = launch(sm);
  if (st) return st;
  LLD_HIP_TRY(hipGetLastError());
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[2], sm));
  LLD_HIP_TRY(hipMemcpyAsync(B.h + down_off, B.d + down_off, down_bytes, hipMemcpyDeviceToHost, sm));
  if (timed) LLD_HIP_TRY(hipEventRecord(ev[3], sm));
  LLD_HIP_TRY(hipStreamSynchronize(sm));
  if (timed) for (int k = 0; k < 3; ++k) LLD_HIP_TRY(hipEventElapsedTime(&phase_ms[k], ev[k], ev[k + 1]));
  return LLD_OK;
}
// ... of a block whose results sit right behind the upload (UploadBlock::end_download)
template <class Launch>
int round_trip(hipStream_t sm, const UploadBlock& B, float* phase_ms, Launch launch) {
  return round_trip(sm, B, B.up_bytes, B.down_bytes, phase_ms, launch);
}

// n elements of a downloaded array to the caller; an output the caller did not ask for (null) is skipped
template <class T> void copy_out(T* dst, const UploadBlock& B, const Span<T>& s, size_t n) { if (dst && n) std::memcpy(dst, B.host(s), n * sizeof(T)); }

// the grid of n items at `per` to a workgroup, never empty
inline dim3 blocks(size_t n, int per) { return dim3((unsigned)std::max<size_t>((n + per - 1) / per, 1)); }

}  // namespace lld_rt

#endif
