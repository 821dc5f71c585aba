// node_remode_plan_test.cpp — the host plan of node dict remode
// (csrc/node_remode_plan.hpp) on the CPU, run by tests/test_node_remode_plan.py
// under ASan/UBSan: the join's window cuts, the storage capacities, both scratch
// layouts, the split's verdict, the slices' verdict that bounds the join's copies,
// and the join's verdict over crafted counters.
// usage: node_remode_plan_test -> "ok <checks>".
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "node_remode_plan.hpp"

using namespace ngpu;
using U64s = std::initializer_list<uint64_t>;

static int checks = 0;
#define REQUIRE(c)                                   \
  do {                                               \
    ++checks;                                        \
    if (!(c)) {                                      \
      printf("FAILED %s (line %d)\n", #c, __LINE__); \
      return 1;                                      \
    }                                                \
  } while (0)

// The windows of m ids at `asked` ids per window tile [0, m) in order, each at most
// c wide and only the last one narrower.
static int check_cuts(uint64_t m, uint64_t asked) {
  const uint64_t c = remode_window_records(asked, m);
  REQUIRE(c >= 1 && (m == 0 || c <= m));
  REQUIRE(asked == 0 || m == 0 || c == std::min(asked, m));
  const uint64_t nw = remode_windows(m, c);
  REQUIRE(nw == (m + c - 1) / c);
  REQUIRE(remode_cut(m, c, 0) == 0 || nw == 0);
  REQUIRE(remode_cut(m, c, nw) == m && remode_cut(m, c, nw + 7) == m);
  // every window when there are few, the edges when there are many
  for (uint64_t t = 0; t < nw; t = (nw > 4096 && t == 2048 ? nw - 2048 : t + 1)) {
    const uint64_t a = remode_cut(m, c, t), b = remode_cut(m, c, t + 1);
    REQUIRE(a == t * c && a < b && b - a <= c);
    REQUIRE(b - a == c || t + 1 == nw);
  }
  return 0;
}

struct Arr { uint64_t off, size, align; };
static int check_arrays(std::vector<Arr> a, uint64_t bytes) {
  uint64_t sum = 0;
  for (const Arr &x : a) {
    REQUIRE(x.off % x.align == 0);
    sum += x.size;
  }
  std::stable_sort(a.begin(), a.end(), [](const Arr &x, const Arr &y) {
    return x.off != y.off ? x.off < y.off : x.size < y.size;
  });
  REQUIRE(a.front().off == 0);
  for (size_t i = 0; i + 1 < a.size(); ++i) REQUIRE(a[i].off + a[i].size <= a[i + 1].off);
  REQUIRE(a.back().off + a.back().size == bytes && sum == bytes);  // exact: no padding
  return 0;
}

static int check_layouts(uint64_t m, uint64_t asked) {
  const uint64_t nw = (m + 63) / 64, tiles = dict_retire_scan_tiles(m);
  const RemodeSplitScratch s = remode_split_scratch_layout(m);
  if (check_arrays({{s.words, 8 * nw, 8}, {s.sums, 8 * (tiles + 1), 8}, {s.cnt, 4 * nw, 4}}, s.bytes)) return 1;
  REQUIRE(remode_split_total_at(s, m) == s.sums + 8 * tiles && remode_split_total_at(s, m) + 8 <= s.cnt);
  REQUIRE(s.bytes >= 8);
  const uint64_t c = remode_window_records(asked, m), wins = remode_windows(m, c);
  const RemodeJoinScratch j = remode_join_scratch_layout(m, c);
  if (check_arrays({{j.stage[0], 64 * c, 64}, {j.stage[1], 64 * c, 64}, {j.bits, 8 * nw, 8},
                    {j.ctr, 8 * kRemodeCtrWords, 8}, {j.off, 8 * (wins + 1), 8}}, j.bytes))
    return 1;
  REQUIRE(j.ctr == j.bits + 8 * nw);  // the bitmap and the counters are zeroed as one
  REQUIRE(j.off - j.bits == 8 * nw + 8 * kRemodeCtrWords);
  return 0;
}

static int check_caps() {
  for (uint64_t s : U64s{0, 1, 2, 3, 63, 64, 65, 4097, 1000000, 0xFFFFFFFEull}) {
    const RemodeCaps c = remode_caps(s);
    REQUIRE(c.rec_cap == dict_retire_rec_cap(s) && c.table_cap == dict_retire_table_cap(s));
    REQUIRE(c.rec_cap >= s && c.rec_cap <= kDictMaxEntries - 1);
    REQUIRE(s > 1000000 || c.rec_cap == s + s / 2);
    REQUIRE(c.table_cap >= 2 * c.rec_cap + 16 && (c.table_cap & (c.table_cap - 1)) == 0);
    // an in-place extend of s / 2 rows fits (dict_grow_plan's share rule)
    const DictGrowPlan g = dict_grow_plan(s, s, c.rec_cap, c.table_cap, s > 1000000 ? 0 : s / 2);
    REQUIRE(g.ok && g.share);
  }
  return 0;
}

static int check_split_verdict() {
  const uint64_t clean[3] = {5, 0, 7};
  REQUIRE(remode_split_verdict(3, clean, 12).ok());
  RemodeVerdict v = remode_split_verdict(3, clean, 13);  // one short
  REQUIRE(v.refusal == kRemodeSplitSum && v.bad == 3 && v.got == 12 && v.want == 13);
  v = remode_split_verdict(3, clean, 11);  // one over
  REQUIRE(v.refusal == kRemodeSplitSum && v.bad == 3 && v.got == 12 && v.want == 11);
  const uint64_t wrap[2] = {~0ull, 2};  // a sum that would wrap to 1
  v = remode_split_verdict(2, wrap, 1);
  REQUIRE(v.refusal == kRemodeSplitSum && v.bad == 0);
  REQUIRE(remode_split_verdict(0, clean, 0).ok() && !remode_split_verdict(0, clean, 1).ok());
  const uint64_t none[2] = {0, 0};
  REQUIRE(remode_split_verdict(2, none, 0).ok());
  REQUIRE(remode_refusal(kRemodeSplitSum)[0] && !remode_refusal(kRemodeOk)[0]);
  return 0;
}

// Two parts holding the ids of `ids[o]` (ascending), m ids, c per window: the offsets
// a binary search would give.
static std::vector<std::vector<uint64_t>> offsets(const std::vector<std::vector<uint64_t>> &ids, uint64_t m,
                                                  uint64_t c) {
  const uint64_t nw = remode_windows(m, c);
  std::vector<std::vector<uint64_t>> off(ids.size(), std::vector<uint64_t>(nw + 1, 0));
  for (size_t o = 0; o < ids.size(); ++o)
    for (uint64_t t = 0; t <= nw; ++t)
      off[o][t] = (uint64_t)(std::lower_bound(ids[o].begin(), ids[o].end(), remode_cut(m, c, t)) - ids[o].begin());
  return off;
}

static int check_slices() {
  const uint64_t m = 10;
  for (uint64_t c : U64s{1, 3, 9, 10}) {
    const std::vector<std::vector<uint64_t>> ids = {{0, 2, 3, 7}, {1, 4, 5, 6, 8, 9}};
    const uint64_t m_o[2] = {4, 6};
    REQUIRE(remode_join_slices(2, m, c, offsets(ids, m, c), m_o).ok());
  }
  {  // an id past the end: the last window comes up short
    const std::vector<std::vector<uint64_t>> ids = {{0, 2, 3, 7}, {1, 4, 5, 6, 8, 12}};
    const uint64_t m_o[2] = {4, 6};
    const RemodeVerdict v = remode_join_slices(2, m, 3, offsets(ids, m, 3), m_o);
    REQUIRE(v.refusal == kRemodeSliceSum && v.window == 3 && v.got == 0 && v.want == 1);
  }
  {  // an id held twice and one missing, c = 1: a window with two rows
    const std::vector<std::vector<uint64_t>> ids = {{0, 2, 3, 7}, {1, 3, 5, 6, 8, 9}};
    const uint64_t m_o[2] = {4, 6};
    const RemodeVerdict v = remode_join_slices(2, m, 1, offsets(ids, m, 1), m_o);
    REQUIRE(v.refusal == kRemodeSliceSum && v.window == 3 && v.got == 2 && v.want == 1);
    // in one window the row counts add up: the scatter's counters have to tell
    REQUIRE(remode_join_slices(2, m, 10, offsets(ids, m, 10), m_o).ok());
  }
  {  // offsets that do not ascend, do not start at 0, or leave the part
    const uint64_t m_o[2] = {4, 6};
    std::vector<std::vector<uint64_t>> off = {{0, 3, 2, 4}, {0, 2, 4, 6}};
    RemodeVerdict v = remode_join_slices(2, 12, 4, off, m_o);
    REQUIRE(v.refusal == kRemodeSliceOrder && v.bad == 0);
    off = {{0, 1, 2, 4}, {1, 4, 6, 6}};
    v = remode_join_slices(2, 12, 4, off, m_o);
    REQUIRE(v.refusal == kRemodeSliceOrder && v.bad == 1);
    off = {{0, 1, 2, 5}, {0, 3, 6, 6}};
    v = remode_join_slices(2, 12, 4, off, m_o);
    REQUIRE(v.refusal == kRemodeSliceOrder && v.bad == 0);
    off = {{0, 1, 2}, {0, 3, 6, 6}};  // too few cuts
    REQUIRE(remode_join_slices(2, 12, 4, off, m_o).refusal == kRemodeSliceOrder);
    // a slice wider than its window never passes, whatever the others hold
    const uint64_t big[2] = {~0ull, ~0ull};
    off = {{0, ~0ull, ~0ull, ~0ull}, {0, 5, 5, 5}};
    REQUIRE(remode_join_slices(2, 12, 4, off, big).refusal == kRemodeSliceSum);
  }
  {  // no entries: no window, one cut
    const uint64_t m_o[2] = {0, 0};
    REQUIRE(remode_join_slices(2, 0, 1, {{0}, {0}}, m_o).ok());
  }
  return 0;
}

static int check_join_verdict() {
  const uint64_t m = 1000;
  std::vector<uint64_t> ctr(3 * kRemodeCtrWords, 0);
  for (int j = 0; j < 3; ++j) ctr[j * kRemodeCtrWords + kRemodeSet] = m;
  REQUIRE(remode_join_verdict(3, ctr.data(), m).ok());
  struct Case { int word; uint64_t value; RemodeRefusal want; };
  for (const Case &k : {Case{kRemodeBadGid, 1, kRemodePastEnd}, Case{kRemodeOutside, 2, kRemodeOutsideWin},
                        Case{kRemodeDupBit, 1, kRemodeHeldTwice}, Case{kRemodeSet, m - 1, kRemodeMissing},
                        Case{kRemodeSet, m + 1, kRemodeMissing}})
    for (uint32_t j = 0; j < 3; ++j) {
      std::vector<uint64_t> x = ctr;
      x[j * kRemodeCtrWords + k.word] = k.value;
      const RemodeVerdict v = remode_join_verdict(3, x.data(), m);
      REQUIRE(v.refusal == k.want && v.bad == j && v.got == k.value);
      REQUIRE(remode_refusal(v.refusal)[0]);
    }
  // an id held twice leaves a position unwritten too: the counter is named, not the count
  std::vector<uint64_t> x = ctr;
  x[kRemodeDupBit] = 1;
  x[kRemodeSet] = m - 1;
  REQUIRE(remode_join_verdict(3, x.data(), m).refusal == kRemodeHeldTwice);
  // the first replica that fails is the one named
  x = ctr;
  x[1 * kRemodeCtrWords + kRemodeSet] = 0;
  x[2 * kRemodeCtrWords + kRemodeBadGid] = 1;
  REQUIRE(remode_join_verdict(3, x.data(), m).bad == 1);
  const uint64_t empty[kRemodeCtrWords] = {0, 0, 0, 0};
  REQUIRE(remode_join_verdict(1, empty, 0).ok() && remode_join_verdict(0, empty, 5).ok());
  return 0;
}

int main() {
  for (uint64_t c : U64s{0, 1, 2, 64, 100, 4096})
    for (uint64_t m : U64s{0, 1, c ? c - 1 : 0, c, c + 1, 2 * c, 2 * c + 1, 4097})
      if (check_cuts(m, c)) return 1;
  if (check_cuts(0xFFFFFFFEull, 1)) return 1;  // a large dict, one id per window
  if (check_cuts(0xFFFFFFFEull, 0)) return 1;
  REQUIRE(remode_window_records(0, 5000000) == kRemodeDefaultWindow);
  REQUIRE(remode_window_records(0, 100) == 100 && remode_window_records(7, 0) == 1);
  for (uint64_t m : U64s{0, 1, 63, 64, 65, 16383, 16384, 16385, 32769, 1000003})
    for (uint64_t c : U64s{0, 1, 64, 100, m, m + 1})
      if (check_layouts(m, c)) return 1;
  if (check_caps() || check_split_verdict() || check_slices() || check_join_verdict()) return 1;
  printf("ok %d\n", checks);
  return 0;
}
