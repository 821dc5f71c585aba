// check_plan_test.cpp — Check's window planner and bitmap decoder
// (csrc/check_plan.hpp) on the CPU, run by tests/test_check_plan.py under
// ASan/UBSan.  usage: check_plan_test SEED -> "ok <cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "check_plan.hpp"

using namespace ngpu;

#define REQUIRE(c)                                             \
  do {                                                         \
    if (!(c)) {                                                \
      printf("FAILED %s (line %d, case %d)\n", #c, __LINE__, tc); \
      return 1;                                                \
    }                                                          \
  } while (0)

int main(int argc, char **argv) {
  std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
  int tc = 0;
  // ---- planner -------------------------------------------------------------
  for (; tc < 200; ++tc) {
    const uint32_t chunk = 1u << (12 + rng() % 9);  // 4 KiB .. 1 MiB
    const uint64_t window = chunk + rng() % (8ull * chunk);
    const uint64_t n = rng() % 400;
    std::vector<CheckItem> it(n);
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t r = rng() % 8;
      it[i].usize = r == 0 ? chunk : r == 1 ? 1 : 1 + (uint32_t)(rng() % chunk);
      it[i].blob = (uint32_t)(rng() % 3);
      it[i].order = 3 * i + 1;
    }
    if (n && tc % 4 == 0) it[rng() % n].usize = (uint32_t)std::min<uint64_t>(window, 0xFFFFFFFFu);  // a chunk
    // exactly the size of the window is planned (below: fits, alone or not)
    std::vector<CheckWindow> wins;
    std::vector<uint64_t> off;
    REQUIRE(check_plan_windows(it.data(), n, window, &wins, &off));
    REQUIRE(off.size() == n);
    REQUIRE(wins.empty() == (n == 0));
    uint64_t next = 0;
    for (const CheckWindow &w : wins) {
      REQUIRE(w.count > 0);
      REQUIRE(w.first == next);  // every chunk in exactly one window, list order
      REQUIRE(w.bytes <= window);
      uint64_t end = 0;
      for (uint64_t i = w.first; i < w.first + w.count; ++i) {
        REQUIRE(off[i] % 16 == 0);
        REQUIRE(off[i] >= end);            // no overlap
        REQUIRE(off[i] < end + 16);        // no gap beyond the alignment
        end = off[i] + it[i].usize;
        REQUIRE(end <= window);            // never split, never past the window
      }
      REQUIRE(end == w.bytes);
      next = w.first + w.count;
      // greedy: the next chunk did not fit behind this window's last one
      if (next < n) REQUIRE((w.bytes + 15) / 16 * 16 + it[next].usize > window);
    }
    REQUIRE(next == n);
  }
  {  // what the caller must have bounded
    std::vector<CheckWindow> wins;
    std::vector<uint64_t> off;
    CheckItem big{4097, 0, 0}, empty{0, 0, 0}, fit{4096, 0, 0};
    REQUIRE(!check_plan_windows(&big, 1, 4096, &wins, &off));
    REQUIRE(!check_plan_windows(&empty, 1, 4096, &wins, &off));
    REQUIRE(check_plan_windows(&fit, 1, 4096, &wins, &off) && wins.size() == 1 && wins[0].bytes == 4096);
    CheckItem two[2] = {fit, fit};
    REQUIRE(check_plan_windows(two, 2, 4096, &wins, &off) && wins.size() == 2 && off[1] == 0);
  }
  // ---- bitmap decoder ------------------------------------------------------
  for (; tc < 400; ++tc) {
    const uint64_t n = tc == 200 ? 0 : rng() % 1500;
    const uint64_t words = (n + 63) / 64;
    std::vector<uint64_t> bm(words);
    const int density = (int)(rng() % 4);
    for (auto &w : bm) w = density == 0 ? 0 : density == 1 ? ~0ull : density == 2 ? rng() : (rng() & rng() & rng());
    uint64_t pop = 0;
    for (uint64_t i = 0; i < n; ++i) pop += bm[i / 64] >> (i % 64) & 1;
    const uint64_t cap = rng() % (n + 2);
    std::vector<uint64_t> out(cap + 1, ~0ull);  // one guard slot past the cap
    const uint64_t total = check_decode_bitmap(bm.data(), n, out.data(), cap);
    REQUIRE(total == pop);  // bits past n in the last word are not counted
    REQUIRE(out[cap] == ~0ull);
    const uint64_t k = total < cap ? total : cap;
    uint64_t seen = 0;
    for (uint64_t j = 0; j < k; ++j) {
      REQUIRE(out[j] < n);
      REQUIRE(bm[out[j] / 64] >> (out[j] % 64) & 1);
      if (j) REQUIRE(out[j] > out[j - 1]);
      // the first k set bits: none skipped
      for (uint64_t i = j ? out[j - 1] + 1 : 0; i < out[j]; ++i) REQUIRE(!(bm[i / 64] >> (i % 64) & 1));
      ++seen;
    }
    REQUIRE(seen == k);
  }
  printf("ok %d\n", tc);
  return 0;
}
