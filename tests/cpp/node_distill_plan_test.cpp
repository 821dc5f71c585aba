// node_distill_plan_test.cpp — the host plan of distilling a partitioned node dict
// (csrc/node_distill_plan.hpp) on the CPU, run by tests/test_node_distill_plan.py
// under ASan/UBSan: a part's scratch layout, the counters of the whole dict summed
// over the parts, a part whose counters are not sane, and the union of the parts'
// live bitmaps through distill_blob_plan under each flag.
// usage: node_distill_plan_test -> "ok <checks>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "node_distill_plan.hpp"

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

// Every array at its offset with its size: aligned, back to back with no overlap,
// `bytes` the end of the last one; the counters of both kinds side by side, refs
// right after the live words (each pair is zeroed, and the first copied, as one).
static int check_layout(uint64_t m_o, uint64_t m, uint32_t W, uint32_t nb) {
  const NodeDistillScratch s = node_distill_scratch_layout(m_o, m, W, nb);
  const NodeRetireScratch &r = s.r;
  const uint64_t nw = (m_o + 63) / 64, gnw = (m + 63) / 64, lw = distill_live_words(nb);
  const uint64_t lt = dict_retire_scan_tiles(m_o), gt = dict_retire_scan_tiles(m);
  REQUIRE(lt == (nw + 255) / 256 && gt == (gnw + 255) / 256);
  REQUIRE(lw == (nb ? (nb + 31) / 32 : 1));
  struct Arr { uint64_t off, size, align; };
  std::vector<Arr> a = {{r.words, 8 * nw, 8},        {r.sums, 8 * (lt + 1), 8},
                        {r.own, 8 * gnw, 8},         {r.gather, 8 * gnw * W, 8},
                        {r.gwords, 8 * gnw, 8},      {r.gsums, 8 * (gt + 1), 8},
                        {r.ctr, 8 * kNodeRetireCtrWords, 8},
                        {s.stats, 8 * kDistillStatWords, 8},
                        {r.cnt, 4 * nw, 4},          {r.gcnt, 4 * gnw, 4},
                        {r.remap, 4ull * nb, 4},     {s.live, 4 * lw, 4},
                        {s.refs, 4 * m_o, 4}};
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
  REQUIRE(a.back().off + a.back().size == s.bytes);
  REQUIRE(s.bytes == sum && r.bytes == s.bytes);  // exact: no padding between the arrays
  REQUIRE(r.bits == r.remap);                     // the retire bitmap has no words here
  REQUIRE(s.stats == r.ctr + 8 * kNodeRetireCtrWords);
  REQUIRE(s.refs == s.live + 4 * lw && s.zero_bytes == 4 * lw + 4 * m_o);
  REQUIRE(s.live + s.zero_bytes == s.bytes);
  // a retire's arrays, plus refs, the counters and the live words
  const NodeRetireScratch base = node_retire_scratch_layout(m_o, m, W, 0, nb);
  REQUIRE(s.bytes == base.bytes + 4 * m_o + 8 * kDistillStatWords + 4 * lw);
  return 0;
}

// A part's block of counters: w winners of which b are below the minimum, the
// largest count mx, the winners' buckets in h (adding up to w), s_o = w - b.
static void part_block(std::vector<uint64_t> &back, uint32_t o, uint64_t w, uint64_t b, uint64_t mx,
                       std::initializer_list<uint64_t> h, uint64_t S) {
  uint64_t *c = &back[(size_t)o * kNodeDistillBackWords];
  c[kNodeRetireLocal] = w - b;
  c[kNodeRetireGlobal] = S;
  uint64_t *st = c + kNodeRetireCtrWords;
  st[kDistillDistinct] = w;
  st[kDistillBelowMin] = b;
  st[kDistillMaxRefs] = mx;
  int k = 0;
  for (uint64_t x : h) st[kDistillHist + k++] = x;
}

static std::vector<uint8_t> table_of(const std::vector<uint32_t> &ids) {
  std::vector<uint8_t> t(256 * ids.size(), 0);
  for (size_t b = 0; b < ids.size(); ++b) memset(&t[256 * b], (int)ids[b], 64);
  return t;
}

int main() {
  REQUIRE(kNodeDistillBackWords == 40 && 8 * kNodeDistillBackWords <= 512);
  for (uint64_t m : std::vector<uint64_t>{0, 1, 63, 64, 65, 16384, 16385, 2 * 16384ull * 256 + 1})
    for (uint32_t W : {1u, 2u, 8u, 64u})
      for (uint64_t m_o : std::vector<uint64_t>{0, 1, 63, 64, 65, m / 2, m})
        for (uint32_t nb : {0u, 1u, 32u, 33u, 1u << 20})
          if (m_o <= m && check_layout(m_o, m, W, nb)) return 1;
  for (uint64_t m_o : std::vector<uint64_t>{16383, 16384, 16385, 16384ull * 256, 16384ull * 256 + 1})
    if (check_layout(m_o, 3 * m_o + 5, 3, 9)) return 1;

  // ---- the summed info: three parts, one of them with no row ----
  {
    const uint32_t W = 3, nb = 40;
    const uint64_t lw = distill_live_words(nb);
    REQUIRE(lw == 2);
    std::vector<uint64_t> back((size_t)W * kNodeDistillBackWords, 0);
    part_block(back, 0, 10, 4, 9, {4, 5, 0, 1}, 13);
    part_block(back, 2, 7, 0, 70, {0, 0, 3, 0, 0, 0, 4}, 13);
    const std::vector<uint64_t> m_o = {30, 0, 200}, s_o = {6, 0, 7};
    // blob 3 live on part 0 only, blob 35 on part 2 only, blob 7 on both
    std::vector<uint32_t> live(W * lw, 0);
    live[0 * lw + 0] = (1u << 3) | (1u << 7);
    live[2 * lw + 0] = 1u << 7;
    live[2 * lw + 1] = 1u << (35 - 32);
    const NodeDistillSum x = node_distill_sum(W, back.data(), live.data(), nb, m_o.data(), s_o.data());
    REQUIRE(x.ok(W));
    REQUIRE(x.stats[kDistillDistinct] == 17 && x.stats[kDistillBelowMin] == 4 && x.stats[kDistillMaxRefs] == 70);
    const uint64_t want[8] = {4, 5, 3, 1, 0, 0, 4, 0};
    uint64_t h = 0;
    for (int k = 0; k < 32; ++k) {
      REQUIRE(x.stats[kDistillHist + k] == (k < 8 ? want[k] : 0));
      h += x.stats[kDistillHist + k];
    }
    REQUIRE(h == x.stats[kDistillDistinct]);
    REQUIRE(distill_stats_sane(x.stats, 230, 13));
    REQUIRE(x.live.size() == lw && x.live[0] == ((1u << 3) | (1u << 7)) && x.live[1] == (1u << 3));
    ngpu_dict_distill_info info;
    memset(&info, 0xA5, sizeof info);
    const DistillBlobPlan p = distill_blob_plan(nb, x.live.data(), 0, nullptr);
    distill_info_fill(&info, 230, x.stats, nb, p.n_kept);
    REQUIRE(info.entries_in == 230 && info.distinct == 17 && info.shadowed == 213 && info.below_min == 4);
    REQUIRE(info.entries_out == 13 && info.max_refs == 70 && info.blobs_in == 40 && info.blobs_out == 3);
    REQUIRE(info.refs_hist[6] == 4 && info.refs_hist[2] == 3);

    // ---- a part whose counters are not sane is refused, whichever it is ----
    for (uint32_t o : {0u, 2u}) {
      std::vector<uint64_t> bad = back;
      bad[(size_t)o * kNodeDistillBackWords + kNodeRetireCtrWords + kDistillHist + 9] += 1;  // buckets != distinct
      REQUIRE(node_distill_sum(W, bad.data(), live.data(), nb, m_o.data(), s_o.data()).bad_part == o);
      std::vector<uint64_t> s2 = s_o;
      s2[o] += 1;  // the scan's survivors != distinct - below_min
      REQUIRE(node_distill_sum(W, back.data(), live.data(), nb, m_o.data(), s2.data()).bad_part == o);
      std::vector<uint64_t> m2 = m_o;
      m2[o] = 5;   // more digests than rows
      REQUIRE(node_distill_sum(W, back.data(), live.data(), nb, m2.data(), s_o.data()).bad_part == o);
    }
    {  // counters on the part that has no row; the first bad part is the one named
      std::vector<uint64_t> bad = back;
      bad[1 * kNodeDistillBackWords + kNodeRetireCtrWords + kDistillMaxRefs] = 1;
      bad[2 * kNodeDistillBackWords + kNodeRetireCtrWords + kDistillMaxRefs] = 201;
      const NodeDistillSum y = node_distill_sum(W, bad.data(), live.data(), nb, m_o.data(), s_o.data());
      REQUIRE(!y.ok(W) && y.bad_part == 1);
    }
  }
  {  // no part, and parts with nothing
    const uint64_t none = 0;
    const uint32_t no_live[2] = {0, 0};
    std::vector<uint64_t> back(2 * kNodeDistillBackWords, 0);
    const uint64_t z[2] = {0, 0};
    const NodeDistillSum x = node_distill_sum(2, back.data(), no_live, 0, z, z);
    REQUIRE(x.ok(2) && x.live.size() == 1 && x.live[0] == 0 && x.stats[kDistillMaxRefs] == 0);
    REQUIRE(node_distill_sum(0, &none, no_live, 0, z, z).ok(0));
  }

  // ---- the union of the live bitmaps through distill_blob_plan, under each flag ----
  {
    // ids: A B A C D; part 0's survivors are in blob 0 (A) alone, part 1's in blob
    // 2 (the later A) and blob 3 (C): blob 3 is live on part 1 only; blob 1 (B) has
    // rows on part 0 and no survivor; blob 4 (D) has no row at all
    const uint32_t W = 2, nb = 5;
    const std::vector<uint8_t> t = table_of({0xA, 0xB, 0xA, 0xC, 0xD});
    std::vector<uint64_t> back((size_t)W * kNodeDistillBackWords, 0);
    part_block(back, 0, 4, 0, 2, {2, 2}, 7);
    part_block(back, 1, 3, 0, 1, {3}, 7);
    const uint64_t m_o[2] = {9, 3}, s_o[2] = {4, 3};
    const uint32_t live[2] = {1u << 0, (1u << 2) | (1u << 3)};
    const NodeDistillSum x = node_distill_sum(W, back.data(), live, nb, m_o, s_o);
    REQUIRE(x.ok(W) && x.live[0] == 0xDu);
    DistillBlobPlan p = distill_blob_plan(nb, x.live.data(), 0, t.data());
    REQUIRE(p.ok && p.n_kept == 3);
    REQUIRE(p.remap == (std::vector<uint32_t>{0, kRetiredBlob, 1, 2, kRetiredBlob}) && p.rows == p.remap);
    p = distill_blob_plan(nb, x.live.data(), NGPU_DICT_DISTILL_KEEP_BLOBS, t.data());
    REQUIRE(p.ok && p.n_kept == 5 && p.remap == (std::vector<uint32_t>{0, 1, 2, 3, 4}) && p.rows == p.remap);
    // the two A, whose survivors sit on different parts, become one row
    p = distill_blob_plan(nb, x.live.data(), NGPU_DICT_DISTILL_MERGE_BLOB_IDS, t.data());
    REQUIRE(p.ok && p.n_kept == 2);
    REQUIRE(p.remap == (std::vector<uint32_t>{0, kRetiredBlob, 0, 1, kRetiredBlob}));
    REQUIRE(p.rows == (std::vector<uint32_t>{0, kRetiredBlob, kRetiredBlob, 1, kRetiredBlob}));
    // part 0 alone would have dropped blob 3, part 1 alone blob 0
    p = distill_blob_plan(nb, &live[0], 0, t.data());
    REQUIRE(p.remap[3] == kRetiredBlob && p.remap[0] == 0);
    p = distill_blob_plan(nb, &live[1], 0, t.data());
    REQUIRE(p.remap[0] == kRetiredBlob && p.remap[3] == 1);
    // the later A live on part 1 only: MERGE keeps the earliest A's row for it
    const uint32_t live2[2] = {0, 1u << 2};
    const NodeDistillSum y = node_distill_sum(W, back.data(), live2, nb, m_o, s_o);
    p = distill_blob_plan(nb, y.live.data(), NGPU_DICT_DISTILL_MERGE_BLOB_IDS, t.data());
    REQUIRE(p.n_kept == 1 && p.remap[0] == 0 && p.remap[2] == 0 && p.rows[0] == 0 && p.rows[2] == kRetiredBlob);
  }
  printf("ok %d\n", checks);
  return 0;
}
