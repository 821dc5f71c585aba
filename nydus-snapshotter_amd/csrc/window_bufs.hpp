// window_bufs.hpp — what one call of a windowed host pipeline holds (Check:
// check.hip; Verity build and verify: verity.hip), and the two steps they share
// around it.  The pipeline: a private non-blocking stream, two staging windows
// of the engine's pool -- host threads fill one (host_window.hpp) while the GPU
// works on the other -- and verdict words that come back behind a system-scope
// fence.  Not installed.
#pragma once

#include <vector>

#include "engine_internal.hpp"

namespace ngpu {

// The big buffers of a window -- pinned host memory and as much HBM -- are a
// staging slot of the engine (staging_take / staging_give, pack.hip: the pool
// the streaming Packs keep theirs in; pinning 256 MiB costs more than copying
// it), so a second call, or a Pack after it, pins nothing.  Everything else a
// call allocates (dmalloc / hmalloc) is its own.  All of it is released on
// every return path, after the stream has drained: a pageable target of an
// async copy on `s` must therefore be declared before the WindowBufs.
struct WindowBufs {
  ngpu_engine *const e;
  hipStream_t s = nullptr;
  hipEvent_t done[2] = {}, fence = nullptr;  // done[k]: window k's work on s has ended
  ngpu_staging_buf win[2];
  std::vector<void *> dev, host;
  explicit WindowBufs(ngpu_engine *e) : e(e) {}
  WindowBufs(const WindowBufs &) = delete;
  WindowBufs &operator=(const WindowBufs &) = delete;
  ~WindowBufs() {
    DeviceGuard g(e->device);
    if (s) (void)hipStreamSynchronize(s);
    for (ngpu_staging_buf &b : win) staging_give(e, b);
    for (void *p : dev) (void)hipFree(p);
    for (void *p : host) (void)hipHostFree(p);
    for (hipEvent_t ev : {done[0], done[1], fence})
      if (ev) (void)hipEventDestroy(ev);
    if (s) (void)hipStreamDestroy(s);
  }
  // The stream, the fence and nbuf <= 2 windows of `bytes` with their events
  // (the caller has set the device).  what: "check" / "verity", for the message.
  int open(int nbuf, uint64_t bytes, const char *what) {
    HIP_TRY(e, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    HIP_TRY(e, hipEventCreateWithFlags(&fence, hipEventDisableTiming));
    for (int k = 0; k < nbuf; ++k) {
      HIP_TRY(e, hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
      if (!staging_take(e, bytes, &win[k])) return no_windows(bytes, what);
    }
    return 0;
  }
  int no_windows(uint64_t bytes, const char *what) const {
    return fail(e, NGPU_ENOMEM, "%s: two windows of %llu bytes", what, (unsigned long long)bytes);
  }
  template <class T>
  bool dmalloc(T **p, uint64_t bytes) {
    if (hipMalloc((void **)p, bytes ? bytes : 64) != hipSuccess) return (void)hipGetLastError(), false;
    dev.push_back(*p);
    return true;
  }
  template <class T>
  bool hmalloc(T **p, uint64_t bytes) {
    if (hipHostMalloc((void **)p, bytes ? bytes : 64, hipHostMallocDefault) != hipSuccess)
      return (void)hipGetLastError(), false;
    host.push_back(*p);
    return true;
  }
  // The verdict tail of the window in buffer k: the fence (a system-scope
  // release before the host's copy), `bytes` verdict bytes D2H into pinned h,
  // then done[k].
  int verdict_back(int k, void *h, const void *d, uint64_t bytes) {
    HIP_TRY(e, hipEventRecord(fence, s));
    HIP_TRY(e, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipEventRecord(done[k], s));
    return 0;
  }
};

// The body of a C ABI entry point of these pipelines through guarded(): a
// host allocation that failed is reported as "<what>: out of memory".
template <class F>
int guarded_entry(ngpu_engine *e, const char *what, F &&f) {
  const int rc = guarded(f);
  if (rc == NGPU_ENOMEM) fail(e, rc, "%s: out of memory", what);
  return rc;
}

}  // namespace ngpu
