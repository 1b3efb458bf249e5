// The one owner of a context's device memory, pinned memory, streams and events (host only).  sogm_ctx, sogm_planner,
// sogm_dsp and sogm_gridmap each hold one.  An acquisition writes the raw handle into the caller's field, which the
// launch code goes on reading, and records it; release_all() is the whole teardown.  A set-up that fills several
// fields on first use runs under a Resources::Setup: if a step fails, whatever it acquired is released and the
// fields are null again, so the field that guards it is never left set by a set-up that did not finish.
// Touched at create, destroy, first use and regrow only: never on a per-tick path.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace sogm {
class Resources {
 public:
  Resources() = default;
  Resources(const Resources &)            = delete;
  Resources &operator=(const Resources &) = delete;

  // `zero`: a null-stream hipMemset behind the allocation (not synchronised: the caller's set-up ends with one
  // hipStreamSynchronize(nullptr) for all of them)
  template <class T>
  hipError_t device(T **out, size_t bytes, bool zero = false) {
    void      *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess && zero && p) e = hipMemset(p, 0, bytes);
    return hold(DEVICE, p, (void **)out, e);
  }
  // `n` elements of T; a request of no bytes takes 16 (a table may be empty, its pointer is never null)
  template <class T>
  hipError_t array(T **out, size_t n) {
    return device(out, n ? n * sizeof(T) : 16);
  }
  template <class T>
  hipError_t pinned(T **out, size_t bytes, unsigned flags) {
    void      *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, flags);
    return hold(PINNED, p, (void **)out, e);
  }
  hipError_t stream(hipStream_t *out) {  // non-blocking
    hipStream_t s = nullptr;
    hipError_t  e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    return hold(STREAM, s, (void **)out, e);
  }
  hipError_t stream_masked(hipStream_t *out, uint32_t mask_words, const uint32_t *mask) {
    hipStream_t s = nullptr;
    hipError_t  e = hipExtStreamCreateWithCUMask(&s, mask_words, mask);
    return hold(STREAM, s, (void **)out, e);
  }
  hipError_t event(hipEvent_t *out, unsigned flags = hipEventDisableTiming) {
    hipEvent_t v = nullptr;
    hipError_t e = hipEventCreateWithFlags(&v, flags);
    return hold(EVENT, v, (void **)out, e);
  }

  // Releases the handle in *field (a stream is synchronised first) and nulls the field.  A null handle, or one that is
  // not held (any more), is left alone: releasing twice is harmless.
  template <class H>
  void release(H *field) {
    for (size_t i = held_.size(); i-- > 0;)
      if (held_[i].handle == (void *)*field && *field) {
        free_handle(held_[i]);
        held_.erase(held_.begin() + (std::ptrdiff_t)i);
        break;
      }
    *field = nullptr;
  }

  // streams currently held (sogm_debug_streams_held): every one of them takes a place in the runtime's pool of hardware queues
  int streams_held() const {
    int n = 0;
    for (const Held &h : held_) n += h.kind == STREAM ? 1 : 0;
    return n;
  }

  size_t mark() const { return held_.size(); }
  // Releases everything acquired since `mark`: streams (each synchronised, then destroyed), then events, then memory,
  // within a kind in reverse order of acquisition.  A field that still holds its handle is nulled.
  void rollback(size_t mark) {
    for (int pass = 0; pass < 3; ++pass)
      for (size_t i = held_.size(); i-- > mark;) {
        const Held &h = held_[i];
        if ((h.kind == STREAM ? 0 : h.kind == EVENT ? 1 : 2) != pass) continue;
        free_handle(h);
        if (*h.field == h.handle) *h.field = nullptr;
      }
    held_.resize(mark);
  }
  void release_all() { rollback(0); }

  // An all-or-nothing set-up: the mark is taken here, and leaving the scope without `return setup.done();` — an error
  // return from the middle, SOGM_HIP_CHECK's included — rolls back to it.
  class Setup {
   public:
    explicit Setup(Resources &r) : r_(r), mark_(r.mark()) {}
    ~Setup() {
      if (!done_) r_.rollback(mark_);
    }
    Setup(const Setup &)            = delete;
    Setup &operator=(const Setup &) = delete;
    int done() {  // (0 = SOGM_OK)
      done_ = true;
      return 0;
    }

   private:
    Resources &r_;
    size_t     mark_;
    bool       done_ = false;
  };

 private:
  enum Kind : unsigned char { STREAM, EVENT, DEVICE, PINNED };
  struct Held {
    Kind   kind;
    void  *handle;
    void **field;
  };
  std::vector<Held> held_;

  static void free_handle(const Held &h) {
    switch (h.kind) {
      case STREAM:
        (void)hipStreamSynchronize((hipStream_t)h.handle);
        (void)hipStreamDestroy((hipStream_t)h.handle);
        break;
      case EVENT: (void)hipEventDestroy((hipEvent_t)h.handle); break;
      case DEVICE: (void)hipFree(h.handle); break;
      case PINNED: (void)hipHostFree(h.handle); break;
    }
  }
  hipError_t hold(Kind kind, void *handle, void **field, hipError_t e) {
    const Held h{kind, handle, field};
    if (e == hipSuccess && handle) {
      try {
        held_.push_back(h);
      } catch (...) {
        e = hipErrorOutOfMemory;
      }
    }
    if (e != hipSuccess) {
      if (handle) free_handle(h);
      return e;
    }
    *field = handle;
    return hipSuccess;
  }
};
}  // namespace sogm
