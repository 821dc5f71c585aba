// host_window_test.cpp — the host pieces the windowed pipelines share
// (csrc/host_window.hpp) on the CPU, run by tests/test_host_window.py under
// ASan/UBSan and under TSan.  usage: host_window_test SEED -> "ok <cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <random>
#include <set>
#include <thread>
#include <vector>

#include "check_plan.hpp"
#include "host_window.hpp"

using namespace ngpu;

static int tc = 0;  // cases passed so far

#define REQUIRE(c)                                                \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s (line %d, case %d)\n", #c, __LINE__, tc); \
      return false;                                               \
    }                                                             \
  } while (0)

// ---- each_set_bit -----------------------------------------------------------
// Against a bit-by-bit loop: every set bit of [lo, hi) ascending, none outside;
// then a callback that stops after the k-th hit, for every k.
static bool bits_case(const std::vector<uint64_t> &bm, uint64_t lo, uint64_t hi) {
  std::vector<uint64_t> want, got;
  for (uint64_t i = lo; i < hi; ++i)
    if (bm[i / 64] >> (i % 64) & 1) want.push_back(i);
  each_set_bit(bm.data(), lo, hi, [&](uint64_t i) { return got.push_back(i), true; });
  REQUIRE(got == want);
  for (uint64_t k = 1; k <= want.size() + 1; k += 1 + want.size() / 7) {
    uint64_t calls = 0, last = 0;
    each_set_bit(bm.data(), lo, hi, [&](uint64_t i) { return last = i, ++calls < k; });
    REQUIRE(calls == std::min<uint64_t>(k, want.size()));
    if (calls) REQUIRE(last == want[calls - 1]);
  }
  ++tc;
  return true;
}

// The decoder as it was before it was written on each_set_bit.
static uint64_t decode_ref(const uint64_t *words, uint64_t n, uint64_t *out, uint64_t cap) {
  uint64_t total = 0;
  for (uint64_t w = 0; w < (n + 63) / 64; ++w) {
    uint64_t m = words[w];
    if (w == n / 64 && (n & 63)) m &= (1ull << (n & 63)) - 1;
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      if (total < cap) out[total] = w * 64 + (uint64_t)b;
      ++total;
    }
  }
  return total;
}

static bool test_bits(std::mt19937_64 &rng) {
  const std::vector<uint64_t> zeros(5, 0), ones(5, ~0ull);
  // lo and hi on and off word boundaries, lo == hi, ranges inside one word
  const uint64_t edges[][2] = {{0, 0},   {0, 64},   {0, 320},   {64, 128},  {64, 64},   {1, 63},
                               {3, 3},   {70, 90},  {63, 65},   {0, 1},     {319, 320}, {100, 320},
                               {64, 65}, {127, 128}, {128, 191}, {5, 257},   {320, 320}};
  for (auto &r : edges) {
    if (!bits_case(zeros, r[0], r[1]) || !bits_case(ones, r[0], r[1])) return false;
    // only the bits just below lo and at hi are set: nothing is reported
    std::vector<uint64_t> bm(6, 0);
    if (r[0]) bm[(r[0] - 1) / 64] |= 1ull << ((r[0] - 1) % 64);
    bm[r[1] / 64] |= 1ull << (r[1] % 64);
    uint64_t calls = 0;
    each_set_bit(bm.data(), r[0], r[1], [&](uint64_t) { return ++calls, true; });
    REQUIRE(calls == 0);
    // ... and with the first and last bit of the range set too: exactly those
    if (r[0] < r[1]) {
      bm[r[0] / 64] |= 1ull << (r[0] % 64);
      bm[(r[1] - 1) / 64] |= 1ull << ((r[1] - 1) % 64);
      if (!bits_case(bm, r[0], r[1])) return false;
    }
  }
  for (int it = 0; it < 200; ++it) {
    const uint64_t words = 1 + rng() % 8, bits = words * 64;
    std::vector<uint64_t> bm(words);
    const int density = (int)(rng() % 3);
    for (auto &w : bm) w = density == 0 ? rng() : density == 1 ? (rng() & rng() & rng() & rng()) : (rng() | rng());
    if (it % 5 == 0) bm[rng() % words] = 0;
    const uint64_t lo = rng() % (bits + 1), hi = lo + rng() % (bits - lo + 1);
    if (!bits_case(bm, lo, hi)) return false;
  }
  // check_decode_bitmap gives the ordinals it gave before
  for (uint64_t n : {0, 1, 63, 64, 65, 129})
    for (int fill = 0; fill < 4; ++fill) {
      std::vector<uint64_t> bm((n + 63) / 64 + 1);
      for (auto &w : bm) w = fill == 0 ? 0 : fill == 1 ? ~0ull : rng() & (fill == 2 ? ~0ull : rng());
      for (uint64_t cap : {(uint64_t)0, n / 2, n, n + 1}) {
        std::vector<uint64_t> a(cap + 1, ~0ull), b(cap + 1, ~0ull);
        REQUIRE(check_decode_bitmap(bm.data(), n, a.data(), cap) == decode_ref(bm.data(), n, b.data(), cap));
        REQUIRE(a == b);
        ++tc;
      }
    }
  return true;
}

// ---- run_indexed ------------------------------------------------------------
static bool test_pool() {
  const std::thread::id me = std::this_thread::get_id();
  for (uint32_t threads : {1u, 3u, 256u})
    for (uint64_t items : {(uint64_t)0, (uint64_t)1, (uint64_t)7, (uint64_t)1000}) {
      const uint64_t want = std::min<uint64_t>(threads, items);
      std::vector<std::atomic<uint32_t>> taken(items);
      for (auto &t : taken) t = 0;
      std::mutex mu;
      std::set<std::thread::id> who;
      std::atomic<uint64_t> here{0};
      // a thread holds its first index until `want` threads have one (or,
      // were they never to come, for five seconds), so every thread of the
      // pool is seen, however short the work
      const auto give_up = std::chrono::steady_clock::now() + std::chrono::seconds(5);
      run_indexed(threads, items, [&](uint64_t q) {
        taken[q].fetch_add(1, std::memory_order_relaxed);
        {
          std::lock_guard<std::mutex> g(mu);
          if (who.insert(std::this_thread::get_id()).second) here.fetch_add(1);
        }
        while (here.load() < want && std::chrono::steady_clock::now() < give_up) std::this_thread::yield();
      });
      // all joined: plain reads from here on
      for (uint64_t q = 0; q < items; ++q) REQUIRE(taken[q] == 1);  // every index exactly once
      REQUIRE(who.size() == want);                                  // min(threads, items) threads ...
      REQUIRE(!items || who.count(me));                             // ... the caller's among them
      ++tc;
    }
  {  // no thread beyond those: each waits a fifth of a second for one more to show up
    std::mutex mu;
    std::set<std::thread::id> who;
    std::atomic<uint64_t> here{0};
    const auto give_up = std::chrono::steady_clock::now() + std::chrono::milliseconds(200);
    run_indexed(3, 1000, [&](uint64_t) {
      {
        std::lock_guard<std::mutex> g(mu);
        if (who.insert(std::this_thread::get_id()).second) here.fetch_add(1);
      }
      while (here.load() < 4 && std::chrono::steady_clock::now() < give_up) std::this_thread::yield();
    });
    REQUIRE(who.size() == 3);
    ++tc;
  }
  // what the functor holds by value is per thread, what it refers to is shared
  std::atomic<uint64_t> sum{0};
  run_indexed(3, 1000, [&sum, mine = std::vector<uint64_t>()](uint64_t q) mutable {
    mine.push_back(q);  // raced on if two threads shared it (TSan)
    sum.fetch_add(q, std::memory_order_relaxed);
  });
  REQUIRE(sum == 999 * 1000 / 2);
  ++tc;
  return true;
}

// ---- read_exact -------------------------------------------------------------
struct Src {
  const uint8_t *p;
  uint64_t size, calls;
  int mode;  // 0: at most 4099 bytes a call; 1: returns 0; 2: returns -1; 3: more than asked
};
static int64_t src_read(void *ctx, void *buf, uint64_t len, uint64_t off) {
  Src *s = (Src *)ctx;
  ++s->calls;
  if (s->mode == 1) return 0;
  if (s->mode == 2) return -1;
  if (s->mode == 3) return (int64_t)len + 1;  // (writes nothing)
  if (off >= s->size) return -1;
  const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(len, 4099), s->size - off);
  memcpy(buf, s->p + off, n);
  return (int64_t)n;
}

static bool test_read(std::mt19937_64 &rng) {
  std::vector<uint8_t> data(100000);
  for (auto &b : data) b = (uint8_t)rng();
  for (uint64_t n : {(uint64_t)1, (uint64_t)4099, (uint64_t)4100, (uint64_t)50000, (uint64_t)100000}) {
    const uint64_t off = rng() % (data.size() - n + 1);
    Src s{data.data(), data.size(), 0, 0};
    std::vector<uint8_t> dst(n + 1, 0xA5);
    REQUIRE(read_exact(src_read, &s, dst.data(), n, off));
    REQUIRE(!memcmp(dst.data(), data.data() + off, n) && dst[n] == 0xA5);
    REQUIRE(s.calls == (n + 4098) / 4099);  // short reads are continued, nothing is read twice
    ++tc;
  }
  for (int mode : {1, 2, 3}) {
    Src s{data.data(), data.size(), 0, mode};
    std::vector<uint8_t> dst(64);
    REQUIRE(!read_exact(src_read, &s, dst.data(), 64, 0));
    REQUIRE(s.calls == 1);
    s.calls = 0;
    REQUIRE(read_exact(src_read, &s, dst.data(), 0, 0) && s.calls == 0);  // n == 0: no call
    ++tc;
  }
  {  // past the end of the source after a good piece
    Src s{data.data(), 5000, 0, 0};
    std::vector<uint8_t> dst(6000);
    REQUIRE(!read_exact(src_read, &s, dst.data(), 6000, 0));
    ++tc;
  }
  return true;
}

int main(int argc, char **argv) {
  std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
  if (!test_bits(rng) || !test_pool() || !test_read(rng)) return 1;
  const uint32_t d = host_threads(0);
  if (d < 1 || d > 16 || host_threads(300) != 256 || host_threads(3) != 3) {
    printf("FAILED host_threads: %u %u %u\n", d, host_threads(300), host_threads(3));
    return 1;
  }
  printf("ok %d\n", ++tc);
  return 0;
}
