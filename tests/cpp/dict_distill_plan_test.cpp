// dict_distill_plan_test.cpp — dict distill's host half
// (csrc/dict_distill_plan.hpp) on the CPU: the live bitmap -> blob remap step
// under the two flags, the scratch layout, the histogram bucket edges and the
// assembly of the info.  Run by tests/test_dict_distill_plan.py under ASan/UBSan.
// usage: dict_distill_plan_test -> "ok <checks>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dict_distill_plan.hpp"

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

static std::vector<uint32_t> bits_of(uint32_t nb, const std::vector<uint8_t> &live) {
  std::vector<uint32_t> w(distill_live_words(nb), 0);
  for (uint32_t b = 0; b < nb; ++b)
    if (live[b]) w[b >> 5] |= 1u << (b & 31);
  return w;
}

// 256-B blob rows whose first 64 bytes spell ids[b]; the rest tells the rows apart.
static std::vector<uint8_t> table_of(const std::vector<uint32_t> &ids) {
  std::vector<uint8_t> t(256 * ids.size(), 0);
  for (size_t b = 0; b < ids.size(); ++b) {
    snprintf((char *)&t[256 * b], 65, "%064x", ids[b]);
    t[256 * b + 64] = 0;
    memcpy(&t[256 * b + 100], &b, sizeof b);
  }
  return t;
}

// Default rule against a plain model: a blob stays iff live, ranks by a count.
static int check_default(uint32_t nb, const std::vector<uint8_t> &live) {
  const std::vector<uint32_t> w = bits_of(nb, live);
  const DistillBlobPlan p = distill_blob_plan(nb, w.data(), 0, nullptr);
  REQUIRE(p.ok);
  REQUIRE(p.remap.size() == nb && p.rows.size() == nb);
  uint32_t rank = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t want = live[b] ? rank : kRetiredBlob;
    if (p.remap[b] != want || p.rows[b] != want) REQUIRE(!"remap entry");
    rank += live[b] != 0;
  }
  ++checks;
  REQUIRE(p.n_kept == rank);
  return 0;
}

int main() {
  // ---- live bitmap -> remap: no blob live, all live, the last dead, 2^20 blobs ----
  for (uint32_t nb : {0u, 1u, 31u, 32u, 33u, 63u, 64u, 65u, 1000u, 1u << 20}) {
    if (check_default(nb, std::vector<uint8_t>(nb, 0))) return 1;
    if (check_default(nb, std::vector<uint8_t>(nb, 1))) return 1;
    if (!nb) continue;
    std::vector<uint8_t> live(nb, 1);
    live[nb - 1] = 0;
    if (check_default(nb, live)) return 1;
    live.assign(nb, 0);
    live[nb - 1] = 1;
    if (check_default(nb, live)) return 1;
    for (uint32_t b = 0; b < nb; ++b) live[b] = (b * 2654435761u >> 13) & 1;
    if (check_default(nb, live)) return 1;
    live[nb / 2] = 0;  // one left empty in the middle
    if (check_default(nb, live)) return 1;
  }
  {
    const std::vector<uint32_t> w((kDictMaxBlobs + 32) / 32 + 1, 0);
    REQUIRE(!distill_blob_plan(kDictMaxBlobs + 1, w.data(), 0, nullptr).ok);
  }
  // ---- KEEP_BLOBS: the identity whatever is live ----
  for (uint32_t nb : {0u, 1u, 65u}) {
    const std::vector<uint32_t> w = bits_of(nb, std::vector<uint8_t>(nb, 0));
    const std::vector<uint8_t> t = table_of(std::vector<uint32_t>(nb, 7));
    const DistillBlobPlan p = distill_blob_plan(nb, w.data(), NGPU_DICT_DISTILL_KEEP_BLOBS, t.data());
    REQUIRE(p.ok && p.n_kept == nb && p.remap.size() == nb && p.rows == p.remap);
    for (uint32_t b = 0; b < nb; ++b) REQUIRE(p.remap[b] == b);
  }
  // ---- MERGE_BLOB_IDS ----
  {
    // ids: A B A C A B; only blob 2 (the middle A) and blob 3 (C) have survivors
    const std::vector<uint8_t> t = table_of({0xA, 0xB, 0xA, 0xC, 0xA, 0xB});
    std::vector<uint32_t> w = bits_of(6, {0, 0, 1, 1, 0, 0});
    DistillBlobPlan p = distill_blob_plan(6, w.data(), NGPU_DICT_DISTILL_MERGE_BLOB_IDS, t.data());
    REQUIRE(p.ok && p.n_kept == 2);
    // the earliest A is the row kept, and every A maps to it; both B die
    REQUIRE(p.rows == (std::vector<uint32_t>{0, kRetiredBlob, kRetiredBlob, 1, kRetiredBlob, kRetiredBlob}));
    REQUIRE(p.remap == (std::vector<uint32_t>{0, kRetiredBlob, 0, 1, 0, kRetiredBlob}));
    // a merge of blobs that all die: the A go, B through its second blob stays
    w = bits_of(6, {0, 0, 0, 0, 0, 1});
    p = distill_blob_plan(6, w.data(), NGPU_DICT_DISTILL_MERGE_BLOB_IDS, t.data());
    REQUIRE(p.ok && p.n_kept == 1);
    REQUIRE(p.rows == (std::vector<uint32_t>{kRetiredBlob, 0, kRetiredBlob, kRetiredBlob, kRetiredBlob, kRetiredBlob}));
    REQUIRE(p.remap == (std::vector<uint32_t>{kRetiredBlob, 0, kRetiredBlob, kRetiredBlob, kRetiredBlob, 0}));
    // nothing live at all
    w = bits_of(6, {0, 0, 0, 0, 0, 0});
    p = distill_blob_plan(6, w.data(), NGPU_DICT_DISTILL_MERGE_BLOB_IDS, t.data());
    REQUIRE(p.ok && p.n_kept == 0);
    for (uint32_t b = 0; b < 6; ++b) REQUIRE(p.remap[b] == kRetiredBlob && p.rows[b] == kRetiredBlob);
    // without the flag the same table merges nothing
    w = bits_of(6, {0, 0, 1, 1, 0, 0});
    p = distill_blob_plan(6, w.data(), 0, t.data());
    REQUIRE(p.remap == (std::vector<uint32_t>{kRetiredBlob, kRetiredBlob, 0, 1, kRetiredBlob, kRetiredBlob}));
    REQUIRE(p.rows == p.remap);
    // ids that differ only in their last byte are not merged
    std::vector<uint8_t> t2 = table_of({0xA, 0xA});
    t2[256 + 63] ^= 1;
    w = bits_of(2, {1, 1});
    p = distill_blob_plan(2, w.data(), NGPU_DICT_DISTILL_MERGE_BLOB_IDS, t2.data());
    REQUIRE(p.n_kept == 2 && p.remap == (std::vector<uint32_t>{0, 1}));
    // 2^20 blobs of 1024 ids, every blob live
    const uint32_t nb = 1u << 20;
    std::vector<uint32_t> ids(nb);
    for (uint32_t b = 0; b < nb; ++b) ids[b] = b & 1023;
    const std::vector<uint8_t> big = table_of(ids);
    w = bits_of(nb, std::vector<uint8_t>(nb, 1));
    p = distill_blob_plan(nb, w.data(), NGPU_DICT_DISTILL_MERGE_BLOB_IDS, big.data());
    REQUIRE(p.ok && p.n_kept == 1024);
    for (uint32_t b = 0; b < nb; ++b) {
      if (p.remap[b] != (b & 1023)) REQUIRE(!"merged remap");
      if (p.rows[b] != (b < 1024 ? b : kRetiredBlob)) REQUIRE(!"merged rows");
    }
  }
  // ---- the scratch layout ----
  for (uint64_t m : {0ull, 1ull, 64ull, 65ull, 16384ull, 16385ull}) {
    for (uint32_t nb : {0u, 1u, 33u, 1u << 20}) {
      const DistillScratch s = distill_scratch_layout(m, nb);
      const uint64_t nw = (m + 63) / 64, nt = dict_retire_scan_tiles(m), lw = distill_live_words(nb);
      REQUIRE(nt == (m == 0 ? 0u : m <= 16384 ? 1u : 2u));
      REQUIRE(s.words == 0 && s.sums == 8 * nw);
      // the scan's total, the counters and the live bitmap are one contiguous copy
      REQUIRE(s.back == s.sums + 8 * nt && s.stats == s.back + 8);
      REQUIRE(s.live == s.stats + 8 * kDistillStatWords);
      REQUIRE(s.back_bytes == 8 + 8 * kDistillStatWords + 4 * lw && s.back_bytes <= 8 + 280 + (128u << 10));
      REQUIRE(s.cnt == s.back + s.back_bytes && s.remap == s.cnt + 4 * nw);
      REQUIRE(s.refs == s.remap + 4ull * nb && s.bytes == s.refs + 4 * m);
      REQUIRE(s.sums % 8 == 0 && s.stats % 8 == 0 && s.cnt % 4 == 0 && s.refs % 4 == 0);
    }
  }
  REQUIRE(kDistillStatWords == 35);
  // ---- histogram bucket edges ----
  REQUIRE(distill_bucket(1) == 0 && distill_bucket(2) == 1 && distill_bucket(3) == 1);
  REQUIRE(distill_bucket(4) == 2 && distill_bucket(7) == 2 && distill_bucket(8) == 3);
  REQUIRE(distill_bucket(0x7FFFFFFFu) == 30 && distill_bucket(0x80000000u) == 31);
  REQUIRE(distill_bucket(0xFFFFFFFFu) == 31);
  // ---- the info ----
  {
    uint64_t st[kDistillStatWords] = {};
    st[kDistillDistinct] = 10;
    st[kDistillBelowMin] = 4;
    st[kDistillMaxRefs] = 9;
    st[kDistillHist + 0] = 4;
    st[kDistillHist + 1] = 5;
    st[kDistillHist + 3] = 1;
    REQUIRE(distill_stats_sane(st, 30, 6));
    REQUIRE(!distill_stats_sane(st, 30, 7));   // survivors != distinct - below_min
    REQUIRE(!distill_stats_sane(st, 9, 6));    // more digests than rows
    st[kDistillHist + 3] = 2;
    REQUIRE(!distill_stats_sane(st, 30, 6));   // the buckets do not add up
    st[kDistillHist + 3] = 1;
    ngpu_dict_distill_info info;
    memset(&info, 0xA5, sizeof info);
    distill_info_fill(&info, 30, st, 7, 3);
    REQUIRE(sizeof info == 312);
    REQUIRE(info.entries_in == 30 && info.distinct == 10 && info.shadowed == 20 && info.below_min == 4);
    REQUIRE(info.entries_out == 6 && info.blobs_in == 7 && info.blobs_out == 3 && info.max_refs == 9);
    REQUIRE(info.reserved == 0 && info.refs_hist[0] == 4 && info.refs_hist[1] == 5 && info.refs_hist[3] == 1);
    REQUIRE(info.refs_hist[2] == 0 && info.refs_hist[31] == 0);
    uint64_t zero[kDistillStatWords] = {};
    REQUIRE(distill_stats_sane(zero, 0, 0));
    distill_info_fill(&info, 0, zero, 0, 0);
    REQUIRE(info.entries_in == 0 && info.max_refs == 0 && info.entries_out == 0);
  }
  printf("ok %d\n", checks);
  return 0;
}
