// buffers.h -- the engine's owning arrays: DevBuf<T> in HBM, PinBuf<T> in
// page-locked host memory.  One allocation per array, its capacity counted in
// elements of T; freed by the destructor (the owner makes the device current).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <type_traits>

#include "otmatch.h"

namespace otm {

template <class T, bool Pinned>
class Buffer {
 public:
  T* p = nullptr;

  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { reset(); }

  size_t cap() const { return bytes_ / sizeof(T); }  // elements that fit
  size_t bytes() const { return bytes_; }            // the allocation, whole

  void reset() {
    if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    bytes_ = 0;
  }
  // hands the allocation to the caller (the index's tables go to graph_allocs)
  T* release() {
    T* q = p;
    p = nullptr;
    bytes_ = 0;
    return q;
  }

  // At least n elements (none: 16 bytes); the contents are not kept on growth,
  // which frees first and allocates a quarter more than asked, against
  // regrowth.  *fresh (when given): whether this call made a new allocation.
  int ensure(size_t n, std::string* err, bool* fresh = nullptr) {
    if (fresh) *fresh = false;
    const size_t bytes = n * sizeof(T) ? n * sizeof(T) : 16;
    if (bytes_ >= bytes) return OTM_OK;
    if (fresh) *fresh = true;
    return alloc(bytes + bytes / 4, err);
  }
  // ... with no headroom: what is sized once (the work counters)
  int ensure_exact(size_t n, std::string* err) { return bytes_ >= n * sizeof(T) ? OTM_OK : alloc(n * sizeof(T), err); }

  // Grows an on-demand tier's table (the huge search and candidate tiers): the
  // new allocation first, so that running out of HBM keeps the old table, and
  // the failed hipMalloc's error taken off the runtime so the batch's later
  // hipGetLastError checks do not report it.  OTM_TEST_GROW_OOM (tests only)
  // asks for a size no device has, to drive that path for real.
  int ensure_grow(size_t n, std::string* err) {
    const size_t bytes = n * sizeof(T) ? n * sizeof(T) : 16;
    if (bytes_ >= bytes) return OTM_OK;
    const char* oom = std::getenv("OTM_TEST_GROW_OOM");
    return alloc(oom && *oom && *oom != '0' ? (size_t)1 << 62 : bytes + bytes / 4, err, true);
  }

 private:
  size_t bytes_ = 0;

  int alloc(size_t want, std::string* err, bool keep_old_on_failure = false) {
    if (!keep_old_on_failure) reset();
    void* q = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&q, want, hipHostMallocDefault) : hipMalloc(&q, want);
    if (e != hipSuccess) {
      if (keep_old_on_failure) (void)hipGetLastError();
      *err = std::string(keep_old_on_failure ? "hipMalloc (tier table): "
                         : Pinned            ? "hipHostMalloc(&b.p, want, hipHostMallocDefault): "
                                             : "hipMalloc(&b.p, want): ") +
             hipGetErrorString(e);
      return OTM_EDEVICE;
    }
    reset();
    p = (T*)q;
    bytes_ = want;
    return OTM_OK;
  }
};
template <class T>
using DevBuf = Buffer<T, false>;
template <class T>
using PinBuf = Buffer<T, true>;

// Sizes b for n elements and points a kernel argument struct's field (T* or
// const T*) at it: a field and its buffer agree on T, or this does not compile.
template <class F, class T, bool Pinned>
int bind_buf(F*& field, Buffer<T, Pinned>& b, size_t n, std::string* err, bool* fresh = nullptr) {
  static_assert(std::is_same<typename std::remove_const<F>::type, T>::value, "the field's type is the buffer's");
  const int rc = b.ensure(n, err, fresh);
  field = b.p;
  return rc;
}
// ... of an on-demand tier (ensure_grow): n == 0 while the tier has no tables
// yet, which allocates nothing
template <class T>
int bind_grow(T*& field, DevBuf<T>& b, size_t n, std::string* err) {
  const int rc = n ? b.ensure_grow(n, err) : OTM_OK;
  field = b.p;
  return rc;
}

}  // namespace otm
