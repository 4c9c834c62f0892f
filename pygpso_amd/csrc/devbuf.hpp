// Who owns a context's device memory.  Host side only; api.hip is the one file of the library that includes this
// (tools/devbuf_check.cpp compiles it on its own, over host memory).  A DevBuf frees what it owns when it is destroyed,
// dropped or assigned over; a view -- a slice of another buffer, the posterior arena's -- owns nothing and is never
// re-sized on its own.  Buffers only grow.  DESIGN.md, "Who frees what".
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace gpso {

// the step of a (re)allocation that failed, and the allocator's own code for it (a hipError_t in the library)
enum class BufStep { Ok, View, Alloc, Copy, Sync, Free };
struct BufStatus {
  BufStep step = BufStep::Ok;
  int err = 0;
  explicit operator bool() const { return step != BufStep::Ok; }
};

// A: where the memory comes from.  Static members, 0 for success:
//   int alloc(void** p, size_t bytes);  int free(void* p, size_t bytes);
//   int copy(void* dst, const void* src, size_t bytes, A::Stream s);   (may be asynchronous on s)
//   int sync(A::Stream s);   (everything enqueued on s so far has finished)
template <class A>
class DevBufT {
  void* p_ = nullptr;
  size_t bytes_ = 0;
  bool view_ = false;

  int release() {
    const int e = (p_ && !view_) ? A::free(p_, bytes_) : 0;
    p_ = nullptr;
    bytes_ = 0;
    view_ = false;
    return e;
  }

 public:
  using Stream = typename A::Stream;
  // readable everywhere, written by the members of this class alone
  void* const& p = p_;
  const size_t& bytes = bytes_;
  const bool& view = view_;

  DevBufT() = default;
  DevBufT(DevBufT&& o) noexcept
      : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)), view_(std::exchange(o.view_, false)) {}
  DevBufT& operator=(DevBufT&& o) noexcept {
    if (this != &o) {
      (void)release();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
      view_ = std::exchange(o.view_, false);
    }
    return *this;
  }
  ~DevBufT() { (void)release(); }

  // back to empty.  The caller knows that nothing on the device still reads the block
  void drop() { (void)release(); }

  // this buffer becomes the view [off, off + bytes) of `whole` (an empty one for bytes = 0)
  void slice(const DevBufT& whole, size_t off, size_t bytes) {
    (void)release();
    p_ = bytes ? static_cast<char*>(whole.p_) + off : nullptr;
    bytes_ = bytes;
    view_ = true;
  }

  // Room for at least `bytes` (16 for 0): nothing happens while the buffer is large enough, a view is refused and left
  // as it is.  The stream is synchronised before an old block is freed -- kernels on it may still be reading it.
  // keep = false: the old block goes first, so that the two never exist together; its contents are lost.
  // keep = true: the old bytes are copied to the front of the new block, then the old one goes.
  BufStatus ensure(size_t bytes, Stream s, bool keep = false) {
    if (bytes == 0) bytes = 16;
    if (bytes_ >= bytes) return {};
    if (view_) return {BufStep::View, 0};
    int e;
    if (p_ && !keep) {
      if ((e = A::sync(s))) return {BufStep::Sync, e};
      if ((e = release())) return {BufStep::Free, e};
    }
    DevBufT grown;
    if ((e = A::alloc(&grown.p_, bytes))) {
      grown.p_ = nullptr;
      return {BufStep::Alloc, e};
    }
    grown.bytes_ = bytes;
    if (p_) {
      if ((e = A::copy(grown.p_, p_, bytes_, s))) return {BufStep::Copy, e};
      if ((e = A::sync(s))) return {BufStep::Sync, e};
    }
    *this = std::move(grown);
    return {};
  }
};

#if defined(__HIPCC__)
// bytes of device memory the DevBufs of this process hold now (gpso_last_count(ctx, 4))
inline std::atomic<int64_t> g_dev_bytes_held{0};

struct HipAlloc {
  using Stream = hipStream_t;
  static int alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) g_dev_bytes_held.fetch_add((int64_t)bytes, std::memory_order_relaxed);
    return (int)e;
  }
  static int free(void* p, size_t bytes) {
    g_dev_bytes_held.fetch_sub((int64_t)bytes, std::memory_order_relaxed);
    return (int)hipFree(p);
  }
  static int copy(void* dst, const void* src, size_t bytes, Stream s) {
    return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
  }
  static int sync(Stream s) { return (int)hipStreamSynchronize(s); }
};
using DevBuf = DevBufT<HipAlloc>;
#endif

}  // namespace gpso
