// lld_upload_block.h — one block of arrays described once: the pinned staging a stage packs, the device block it is copied into and the
// device-only scratch behind the copied prefix share ONE list of declarations.  take<T>(n, per) declares n elements of `per` T's each; byte
// size, 256-byte alignment and offset follow from that alone, and the typed host / device pointers come from the same Span.  Host only, no
// HIP, no heap.  (lld_slab of lld_common.h hands out pointers into one base that must exist first; here the offsets serve two bases and size both.)
#ifndef LLD_UPLOAD_BLOCK_H
#define LLD_UPLOAD_BLOCK_H

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace lld_track {

inline size_t al(size_t b) { return (b + 255) & ~size_t(255); }

template <class T> struct Span { size_t off = 0, n = 0; };   // n T's at byte offset `off` of the block; n = 0 takes no bytes

struct UploadBlock {
  size_t size = 0, up_bytes = 0;             // bytes declared so far; the prefix that travels (end_upload)
  char* h = nullptr; char* d = nullptr;      // pinned host base (the prefix that travels), device base (the whole block)
  template <class T> Span<T> take(size_t n, size_t per = 1) { const Span<T> s{size, n * per}; size += al(s.n * sizeof(T)); return s; }
  void end_upload() { up_bytes = size; }     // what was declared so far is uploaded, what follows is device-only scratch
  // a call that also fetches results declares them right behind the upload and ends them here: the pinned base then spans travel_bytes()
  size_t down_bytes = 0;
  void end_download() { down_bytes = size - up_bytes; }
  size_t travel_bytes() const { return up_bytes + down_bytes; }
  void bind(char* host, char* dev) { h = host; d = dev; }
  template <class T> T* host(const Span<T>& s) const { return reinterpret_cast<T*>(h + s.off); }
  template <class T> T* dev(const Span<T>& s) const { return reinterpret_cast<T*>(d + s.off); }
  // the caller's array into the staging; a null source fills the array's own bytes with `fill`
  template <class T>
  void stage(const Span<T>& s, const T* src, int fill = 0) const {
    if (!s.n) return;
    if (src) std::memcpy(h + s.off, src, s.n * sizeof(T)); else std::memset(h + s.off, fill, s.n * sizeof(T));
  }
};

}  // namespace lld_track

#endif
