// host_window.hpp — the host-side pieces the windowed pipelines share
// (check.hip's Check, verity.hip's Verity build and verify): the reader loop,
// the reader pool, the thread-count rule and the bitmap scan.  Checked on the
// CPU by tests/cpp/host_window_test.cpp under ASan/UBSan and TSan (no GPU).
// Header-only, host-only, no HIP.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

namespace ngpu {

// ngpu_read_at_fn (nydus_gpu.h): bytes read (> 0) or a negative error.
using read_at_fn = int64_t (*)(void *ctx, void *buf, uint64_t len, uint64_t off);

// The n bytes at `off` of the reader into dst; short reads are continued.
// false: the reader failed, returned nothing, or more than it was asked for.
inline bool read_exact(read_at_fn ra, void *ctx, uint8_t *dst, uint64_t n, uint64_t off) {
  while (n) {
    const int64_t r = ra(ctx, dst, n, off);
    if (r <= 0 || (uint64_t)r > n) return false;
    dst += r;
    off += (uint64_t)r;
    n -= (uint64_t)r;
  }
  return true;
}

// f(q) once for every q < items, on min(threads, items) threads, the caller's
// among them; all joined on return.  The threads take the next index until
// none is left; there is no early exit (a functor that wants one keeps a flag
// and returns at once when it is set).  Every thread calls its own copy of f:
// what f holds by value is per thread (a scratch buffer), what it refers to is
// shared.
template <class F>
void run_indexed(uint32_t threads, uint64_t items, F f) {
  std::atomic<uint64_t> next{0};
  auto work = [&next, items, f]() mutable {
    for (uint64_t q; (q = next.fetch_add(1, std::memory_order_relaxed)) < items;) f(q);
  };
  const uint32_t T = (uint32_t)std::min<uint64_t>(threads, items);
  std::vector<std::thread> pool;
  for (uint32_t t = 1; t < T; ++t) pool.emplace_back(work);
  work();
  for (auto &t : pool) t.join();
}

// The `threads` option of a host pipeline: 0 -> min(16, cores), at most 256.
inline uint32_t host_threads(uint32_t asked) {
  if (!asked) asked = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  return std::min(asked, 256u);
}

// f(i) for every set bit lo <= i < hi of the bitmap, ascending, until it
// returns false.
template <class F>
void each_set_bit(const uint64_t *words, uint64_t lo, uint64_t hi, F f) {
  for (uint64_t i = lo; i < hi; ++i) {
    const uint64_t rest = words[i >> 6] >> (i & 63);
    if (!rest) {
      i |= 63;
      continue;
    }
    i += (uint64_t)__builtin_ctzll(rest);
    if (i >= hi || !f(i)) return;
  }
}

}  // namespace ngpu
