// node_retire_plan_test.cpp — the host plan of retiring a partitioned node dict
// (csrc/node_retire_plan.hpp) on the CPU, run by tests/test_node_retire_plan.py
// under ASan/UBSan: the scratch layout, the verdict over the parts' counters, the
// capacities of the result and the global rank the compaction writes.
// usage: node_retire_plan_test -> "ok <checks>".
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <initializer_list>
#include <utility>
#include <vector>

#include "node_retire_plan.hpp"

using namespace ngpu;

static int checks = 0;
#define REQUIRE(c)                                   \
  do {                                               \
    ++checks;                                        \
    if (!(c)) {                                      \
      printf("FAILED %s (line %d)\n", #c, __LINE__); \
      return 1;                                      \
    }                                                \
  } while (0)

// Every array at its offset with its size: aligned, in order, back to back with
// no overlap, and `bytes` is the end of the last one.
static int check_layout(uint64_t m_o, uint64_t m, uint32_t W, uint64_t bw, uint64_t rw) {
  const NodeRetireScratch s = node_retire_scratch_layout(m_o, m, W, bw, rw);
  const uint64_t nw = (m_o + 63) / 64, gnw = (m + 63) / 64;
  const uint64_t lt = (nw + 255) / 256, gt = (gnw + 255) / 256;
  REQUIRE(dict_retire_scan_tiles(m_o) == lt && dict_retire_scan_tiles(m) == gt);
  struct Arr { uint64_t off, size, align; };
  std::vector<Arr> a = {{s.words, 8 * nw, 8},        {s.sums, 8 * (lt + 1), 8},
                        {s.own, 8 * gnw, 8},         {s.gather, 8 * gnw * W, 8},
                        {s.gwords, 8 * gnw, 8},      {s.gsums, 8 * (gt + 1), 8},
                        {s.ctr, 8 * kNodeRetireCtrWords, 8},
                        {s.cnt, 4 * nw, 4},          {s.gcnt, 4 * gnw, 4},
                        {s.bits, 4 * bw, 4},         {s.remap, 4 * rw, 4}};
  uint64_t sum = 0;
  for (const Arr &x : a) {
    REQUIRE(x.off % x.align == 0);
    sum += x.size;
  }
  std::sort(a.begin(), a.end(), [](const Arr &x, const Arr &y) {
    return x.off != y.off ? x.off < y.off : x.size < y.size;
  });
  REQUIRE(a.front().off == 0);
  for (size_t i = 0; i + 1 < a.size(); ++i) REQUIRE(a[i].off + a[i].size <= a[i + 1].off);
  REQUIRE(a.back().off + a.back().size == s.bytes);
  REQUIRE(s.bytes == sum);  // exact: no padding between the arrays
  // the bound the header states
  REQUIRE(s.bytes == 8 * (W + 2ull) * gnw + 4 * gnw + 12 * nw +
                         8 * (lt + gt + 2 + kNodeRetireCtrWords) + 4 * (bw + rw));
  return 0;
}

static std::vector<uint64_t> counters(uint32_t W, const std::vector<uint64_t> &s, uint64_t S) {
  std::vector<uint64_t> c((size_t)W * kNodeRetireCtrWords, 0);
  for (uint32_t o = 0; o < W; ++o) {
    c[(size_t)o * kNodeRetireCtrWords + kNodeRetireLocal] = s[o];
    c[(size_t)o * kNodeRetireCtrWords + kNodeRetireGlobal] = S;
  }
  return c;
}

int main() {
  for (uint64_t m : std::vector<uint64_t>{0, 1, 63, 64, 65, 16384, 16385, 2 * 16384ull * 256 + 1})
    for (uint32_t W : {1u, 2u, 8u, 64u})
      for (uint64_t m_o : std::vector<uint64_t>{0, m / 2, m})
        for (auto br : {std::pair<uint64_t, uint64_t>{1, 0}, {1, 1}, {3, 65}, {1u << 15, 1u << 20}})
          if (check_layout(m_o, m, W, br.first, br.second)) return 1;

  // the verdict: accepted
  {
    const std::vector<uint64_t> s = {5, 0, 7};  // one part keeps nothing
    const std::vector<uint64_t> c = counters(3, s, 12);
    const NodeRetireVerdict v = node_retire_verdict(3, c.data(), 20);
    REQUIRE(v.ok() && v.S == 12 && v.s == s);
    const NodeRetireCaps caps = node_retire_caps(v);
    REQUIRE(caps.rec_cap.size() == 3 && caps.table_cap.size() == 3);
    for (int o = 0; o < 3; ++o) {
      REQUIRE(caps.rec_cap[o] == dict_retire_rec_cap(s[o]));
      REQUIRE(caps.table_cap[o] == dict_retire_table_cap(s[o]));
    }
    REQUIRE(caps.rec_cap[1] == 0 && caps.rec_cap[2] == 10 && caps.table_cap[2] == 64);
    REQUIRE(caps.place_cap == dict_retire_rec_cap(12) && caps.place_cap == 18);
  }
  {
    const std::vector<uint64_t> c = counters(8, std::vector<uint64_t>(8, 0), 0);  // S == 0
    const NodeRetireVerdict v = node_retire_verdict(8, c.data(), 1000);
    REQUIRE(v.ok() && v.S == 0);
    const NodeRetireCaps caps = node_retire_caps(v);
    REQUIRE(caps.place_cap == 0 && caps.rec_cap[7] == 0 && caps.table_cap[7] == dict_retire_table_cap(0));
  }
  {
    const std::vector<uint64_t> c = counters(1, {9}, 9);  // S == m
    REQUIRE(node_retire_verdict(1, c.data(), 9).ok());
    const std::vector<uint64_t> e = counters(2, {0, 0}, 0);  // m == 0
    REQUIRE(node_retire_verdict(2, e.data(), 0).ok());
  }
  // the verdict: each counter non-zero, on each part
  for (int k : {kNodeRetireBadGid, kNodeRetireDupBit, kNodeRetireOverlap})
    for (uint32_t o = 0; o < 3; ++o) {
      std::vector<uint64_t> c = counters(3, {5, 0, 7}, 12);
      c[(size_t)o * kNodeRetireCtrWords + k] = 1;
      const NodeRetireVerdict v = node_retire_verdict(3, c.data(), 20);
      REQUIRE(!v.ok() && v.refusal == kNodeRetireCounter && v.bad == o && v.which == k);
    }
  // the sum of s_o is not S (an id held twice makes it larger, a lost row smaller)
  for (uint64_t S : std::vector<uint64_t>{11, 13}) {
    const std::vector<uint64_t> c = counters(3, {5, 0, 7}, S);
    const NodeRetireVerdict v = node_retire_verdict(3, c.data(), 20);
    REQUIRE(!v.ok() && v.refusal == kNodeRetireSum && v.bad == 3);
  }
  {  // the parts disagree about S
    std::vector<uint64_t> c = counters(3, {5, 0, 7}, 12);
    c[2 * kNodeRetireCtrWords + kNodeRetireGlobal] = 11;
    const NodeRetireVerdict v = node_retire_verdict(3, c.data(), 20);
    REQUIRE(!v.ok() && v.refusal == kNodeRetireSum && v.bad == 2);
  }
  {  // S > m
    const std::vector<uint64_t> c = counters(2, {6, 7}, 13);
    const NodeRetireVerdict v = node_retire_verdict(2, c.data(), 12);
    REQUIRE(!v.ok() && v.refusal == kNodeRetireTooMany);
  }

  // the global rank: against a count over the bits, across word boundaries
  {
    const uint64_t m = 3 * 64 + 5;
    std::vector<uint64_t> w((m + 63) / 64, 0);
    std::vector<uint32_t> pre(w.size(), 0);
    for (uint64_t g = 0; g < m; ++g)
      if (g % 3 != 1 && g != 64 && g != 127) w[g >> 6] |= 1ull << (g & 63);
    for (size_t j = 1; j < w.size(); ++j) pre[j] = pre[j - 1] + (uint32_t)__builtin_popcountll(w[j - 1]);
    uint64_t rank = 0;
    for (uint64_t g = 0; g < m; ++g) {
      if (node_retire_new_gid(w.data(), pre.data(), g) != rank) REQUIRE(!"global rank");
      rank += (w[g >> 6] >> (g & 63)) & 1;
    }
    ++checks;
  }
  printf("ok %d\n", checks);
  return 0;
}
