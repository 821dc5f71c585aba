// dict_retire_plan_test.cpp — dict retire's blob bitmap, blob remap and storage
// sizing (csrc/dict_retire_plan.hpp) on the CPU, run by
// tests/test_dict_retire_plan.py under ASan/UBSan.
// usage: dict_retire_plan_test -> "ok <checks>".
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "dict_grow_plan.hpp"
#include "dict_retire_plan.hpp"

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

// The plan against a plain model: gone[b] by a scan of the list, ranks by a count.
static int check_plan(uint32_t nb, const std::vector<uint32_t> &list) {
  const DictRetirePlan p = dict_retire_plan(nb, list.data(), (uint32_t)list.size());
  REQUIRE(p.ok);
  REQUIRE(p.bitmap.size() == (nb ? (nb + 31) / 32 : 1));
  REQUIRE(p.remap.size() == nb);
  std::vector<uint8_t> gone(nb, 0);
  for (uint32_t b : list) gone[b] = 1;
  uint32_t rank = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    const bool bit = (p.bitmap[b >> 5] >> (b & 31)) & 1;
    if (bit != (gone[b] != 0)) REQUIRE(!"bitmap bit");
    if (p.remap[b] != (gone[b] ? kRetiredBlob : rank)) REQUIRE(!"remap entry");
    rank += !gone[b];
  }
  ++checks;
  REQUIRE(p.n_kept == rank);
  // no bit past the last blob
  for (uint64_t b = nb; b < 32ull * p.bitmap.size(); ++b)
    if ((p.bitmap[b >> 5] >> (b & 31)) & 1) REQUIRE(!"bit past the last blob");
  return 0;
}

int main() {
  // remap and bitmap at 1, 63, 64, 65 and 2^20 blobs: the first, the last, a
  // middle one, all, none, every second one, and duplicates in the list
  for (uint32_t nb : {1u, 2u, 31u, 32u, 33u, 63u, 64u, 65u, 1u << 20}) {
    std::vector<uint32_t> all, second;
    for (uint32_t b = 0; b < nb; ++b) {
      all.push_back(b);
      if (b & 1) second.push_back(b);
    }
    const std::vector<std::vector<uint32_t>> lists = {
        {}, {0}, {nb - 1}, {nb / 2}, {0, nb - 1}, {nb / 2, nb / 2, nb / 2}, {nb - 1, 0, nb - 1, 0},
        all, second};
    for (const auto &l : lists)
      if (check_plan(nb, l)) return 1;
  }
  // what the numbers are, spelled out once
  {
    const uint32_t l[] = {3, 1, 3};
    const DictRetirePlan p = dict_retire_plan(5, l, 3);
    REQUIRE(p.ok && p.n_kept == 3 && p.bitmap.size() == 1 && p.bitmap[0] == 0xA);
    REQUIRE(p.remap[0] == 0 && p.remap[1] == kRetiredBlob && p.remap[2] == 1);
    REQUIRE(p.remap[3] == kRetiredBlob && p.remap[4] == 2);
  }
  // retire all: nothing is kept; none: the identity
  {
    const uint32_t l[] = {0, 1, 2};
    DictRetirePlan p = dict_retire_plan(3, l, 3);
    REQUIRE(p.ok && p.n_kept == 0);
    p = dict_retire_plan(3, nullptr, 0);
    REQUIRE(p.ok && p.n_kept == 3 && p.remap[0] == 0 && p.remap[1] == 1 && p.remap[2] == 2);
    REQUIRE(p.bitmap[0] == 0);
  }
  // a dict of no blobs: one (zero) bitmap word for the kernel to read, no remap
  {
    const DictRetirePlan p = dict_retire_plan(0, nullptr, 0);
    REQUIRE(p.ok && p.n_kept == 0 && p.bitmap.size() == 1 && p.bitmap[0] == 0 && p.remap.empty());
  }
  // an index that equals the blob count (or lies past it) is refused, wherever it stands
  for (uint32_t nb : {0u, 1u, 63u, 64u, 65u, 1u << 20}) {
    const uint32_t l[] = {0, nb, 0};
    DictRetirePlan p = dict_retire_plan(nb, l + 1, 1);
    REQUIRE(!p.ok && p.bad == nb && p.bitmap.empty() && p.remap.empty());
    if (nb) {
      p = dict_retire_plan(nb, l, 3);
      REQUIRE(!p.ok && p.bad == nb);
    }
    const uint32_t big[] = {0xFFFFFFFFu};
    REQUIRE(!dict_retire_plan(nb, big, 1).ok);
  }
  REQUIRE(!dict_retire_plan((1u << 20) + 1, nullptr, 0).ok);
  // capacities: s + s / 2 record slots and dict_alloc's table for that many
  REQUIRE(dict_retire_rec_cap(0) == 0 && dict_retire_table_cap(0) == 16);
  REQUIRE(dict_retire_rec_cap(1) == 1 && dict_retire_table_cap(1) == 32);   // 2 + 16
  REQUIRE(dict_retire_rec_cap(2) == 3 && dict_retire_table_cap(2) == 32);   // 6 + 16
  REQUIRE(dict_retire_rec_cap(3) == 4 && dict_retire_table_cap(3) == 32);   // 8 + 16
  REQUIRE(dict_retire_rec_cap(200000000ull) == 300000000ull);
  REQUIRE(dict_retire_table_cap(200000000ull) == 1ull << 30);  // 600,000,016 -> 2^30
  REQUIRE(dict_retire_rec_cap(0xFFFFFFFEull) == 0xFFFFFFFEull);  // no slot past the last valid id
  REQUIRE(dict_retire_table_cap(0xFFFFFFFEull) == 1ull << 34);
  // the same storage a fork of an extend with k = 0 gets
  for (uint64_t s : {0ull, 1ull, 2ull, 3ull, 64ull, 1000ull, 200000000ull, 0xFFFFFFFEull}) {
    const DictGrowPlan f = dict_grow_plan(s, s + 1, 0, 0, 0);
    REQUIRE(f.ok && !f.share);
    REQUIRE(f.rec_cap == dict_retire_rec_cap(s) && f.table_cap == dict_retire_table_cap(s));
  }
  // a retire followed by extends of up to s / 2 rows in all appends in place
  // (dict_grow_plan's share branch); one row more forks
  for (uint64_t s : {0ull, 1ull, 2ull, 3ull, 7ull, 64ull, 1000ull, 1000001ull, 200000000ull}) {
    const uint64_t rc = dict_retire_rec_cap(s), tc = dict_retire_table_cap(s);
    for (uint64_t k : {(uint64_t)0, (uint64_t)1, s / 4, s / 2}) {
      if (k > s / 2) continue;
      const DictGrowPlan p = dict_grow_plan(s, s, rc, tc, k);
      REQUIRE(p.ok && p.share && p.rec_cap == rc && p.table_cap == tc);
    }
    REQUIRE(!dict_grow_plan(s, s, rc, tc, s / 2 + 1).share);
    // two steps: s / 4 then the rest
    const uint64_t k1 = s / 4, k2 = s / 2 - k1;
    REQUIRE(dict_grow_plan(s + k1, s + k1, rc, tc, k2).share);
  }
  // the host side of the compaction: rows by keep words and prefixes, in word
  // ranges as the threads take them, against a plain scan
  for (uint64_t m : {1ull, 63ull, 64ull, 65ull, 128ull, 1000ull, 4096ull * 64 + 7}) {
    const uint64_t nw = (m + 63) / 64;
    for (int pattern = 0; pattern < 4; ++pattern) {
      std::vector<uint64_t> words(nw), src(m), want;
      std::vector<uint32_t> prefix(nw);
      uint64_t lcg = 12345 + m + pattern;
      for (uint64_t w = 0; w < nw; ++w) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        // all kept, none kept, random words, whole words of ones between random ones
        words[w] = pattern == 0 ? ~0ull : pattern == 1 ? 0 : (pattern == 3 && (w & 1)) ? ~0ull : lcg;
        // bits at or past m: garbage the helper must ignore
        prefix[w] = (uint32_t)want.size();
        for (uint64_t b = 0; b < 64 && w * 64 + b < m; ++b)
          if ((words[w] >> b) & 1) want.push_back(w * 64 + b + 1000);
      }
      for (uint64_t i = 0; i < m; ++i) src[i] = i + 1000;
      const uint64_t s = want.size();
      for (uint64_t piece : {(uint64_t)1, (uint64_t)3, kRetireHostPiece, nw + 5}) {
        std::vector<uint64_t> dst(s + 1, 7);  // exactly s rows and a guard
        for (uint64_t a = 0; a < nw; a += piece)
          dict_retire_compact_rows(words.data(), prefix.data(), a, a + piece < nw ? a + piece : nw, m,
                                   src.data(), dst.data(), s);
        REQUIRE(dst[s] == 7);
        dst.pop_back();
        REQUIRE(dst == want);
      }
      // a result shorter than the bits say (never on a sound call): nothing past it is written
      if (s >= 2) {
        std::vector<uint64_t> dst(s, 7);
        dict_retire_compact_rows(words.data(), prefix.data(), 0, nw, m, src.data(), dst.data(), s / 2);
        for (uint64_t j = s / 2; j < s; ++j)
          if (dst[j] != 7) REQUIRE(!"row written past s");
        ++checks;
      }
    }
  }
  // ---- the scratch layout: the offsets written out by hand ----
  for (uint64_t m : {0ull, 1ull, 63ull, 64ull, 65ull, 16383ull, 16384ull, 16385ull})
    for (uint64_t bw : {1ull, 2ull, 32768ull})        // bitmap words: at least one
      for (uint64_t rw : {0ull, 1ull, 1000ull}) {     // remap words: one per blob
        const uint64_t nw = (m + 63) / 64, nt = (nw + 255) / 256;
        const RetireScratch s = retire_scratch_layout(m, bw, rw);
        REQUIRE(dict_retire_scan_tiles(m) == nt);
        REQUIRE(s.words == 0 && s.sums == 8 * nw && s.cnt == 8 * nw + 8 * (nt + 1));
        REQUIRE(s.bits == 8 * nw + 8 * (nt + 1) + 4 * nw && s.remap == s.bits + 4 * bw);
        REQUIRE(s.bytes == 8 * nw + 8 * (nt + 1) + 4 * nw + 4 * bw + 4 * rw);
        REQUIRE(s.words % 8 == 0 && s.sums % 8 == 0 && s.cnt % 4 == 0 && s.bits % 4 == 0 && s.remap % 4 == 0);
        REQUIRE(s.words + 8 * nw <= s.sums && s.sums + 8 * (nt + 1) <= s.cnt && s.cnt + 4 * nw <= s.bits &&
                s.bits + 4 * bw <= s.remap && s.remap + 4 * rw <= s.bytes);
      }
  printf("ok %d\n", checks);
  return 0;
}
