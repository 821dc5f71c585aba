// dict_save_plan_test.cpp — dict save's host plan (csrc/dict_save_plan.hpp) on the
// CPU, run by tests/test_dict_save_plan.py under ASan/UBSan: the file layout at the
// edges of the entry and blob counts, the header bytes, the window cuts, and every
// refusal of the options.
// usage: dict_save_plan_test -> "ok <checks>".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <vector>

#include "dict_save_plan.hpp"

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

static int check_layout() {
  for (uint64_t k : {0ull, 1ull, 1ull << 20, 0xFFFFFFFEull})
    for (uint64_t b : {0ull, 1ull, 15ull, 16ull, 17ull, 1ull << 20}) {
      ngpu_dict_save_info l;
      memset(&l, 0xAB, sizeof l);
      REQUIRE(dict_save_layout(k, b, &l));
      REQUIRE(l.entries == k && l.blobs == b && l.windows == 0);
      REQUIRE(l.blob_table_offset == (b ? 4096u : 0u));
      REQUIRE(l.blob_table_size == 256 * b);
      // the chunk table starts on the first 4096 boundary at or past the blob rows' end
      REQUIRE(l.chunk_table_offset % 4096 == 0);
      REQUIRE(l.chunk_table_offset >= 4096 + 256 * b && l.chunk_table_offset < 4096 + 256 * b + 4096);
      REQUIRE(l.chunk_table_size == 80 * k);
      REQUIRE(l.bytes == l.chunk_table_offset + 80 * k);
      REQUIRE(dict_save_blob_pad(l) == l.chunk_table_offset - 4096 - 256 * b);
      REQUIRE(dict_save_blob_pad(l) < 4096);
    }
  ngpu_dict_save_info l;
  REQUIRE(dict_save_layout(5, 0, &l) && l.chunk_table_offset == 4096 && l.bytes == 4096 + 400);
  REQUIRE(dict_save_layout(5, 16, &l) && l.chunk_table_offset == 8192 && dict_save_blob_pad(l) == 0);
  REQUIRE(dict_save_layout(5, 17, &l) && l.chunk_table_offset == 12288 && dict_save_blob_pad(l) == 4096 - 256);
  REQUIRE(dict_save_layout(0xFFFFFFFEull, 1u << 20, &l));
  REQUIRE(l.bytes == 4096 + (256ull << 20) + 80ull * 0xFFFFFFFEull);
  REQUIRE(l.blob_table_size <= 0xFFFFFFFFull);  // the header's 32-bit field holds it
  // past the limits: refused, and the answer is zeroed
  for (auto kb : {std::initializer_list<uint64_t>{0xFFFFFFFFull, 0}, {1ull << 40, 1}, {~0ull, 0},
                  {1, (1ull << 20) + 1}, {0, 0xFFFFFFFFull}}) {
    memset(&l, 0xAB, sizeof l);
    REQUIRE(!dict_save_layout(kb.begin()[0], kb.begin()[1], &l));
    REQUIRE(l.bytes == 0 && l.entries == 0 && l.chunk_table_offset == 0);
  }
  return 0;
}

static int check_header() {
  ngpu_dict_save_info l;
  REQUIRE(dict_save_layout(1000, 17, &l));
  std::vector<uint8_t> h(4096, 0xCD), z(4096, 0);
  dict_save_header(l, 0x8, 0x100000, h.data());
  auto u32 = [&](size_t at) { uint32_t v; memcpy(&v, h.data() + at, 4); return v; };
  auto u64 = [&](size_t at) { uint64_t v; memcpy(&v, h.data() + at, 8); return v; };
  REQUIRE(u32(1024) == 0xE0F5E1E2u);
  REQUIRE(u64(1152) == 0x8 && u64(1160) == 4096 && u32(1168) == 17 * 256 && u32(1172) == 0x100000);
  REQUIRE(u64(1176) == 12288 && u64(1184) == 80000 && u64(1192) == 0 && u32(1200) == 0);
  // everything else is zero
  memset(h.data() + 1024, 0, 4);
  memset(h.data() + 1152, 0, 52);
  REQUIRE(h == z);
  REQUIRE(dict_save_layout(3, 0, &l));
  dict_save_header(l, 0x4, 0x10000, h.data());
  REQUIRE(u64(1152) == 0x4 && u64(1160) == 0 && u32(1168) == 0 && u64(1176) == 4096 && u64(1184) == 240);
  return 0;
}

// The windows of [first, m) tile it in order, each of window_records but the last.
static int check_cuts(uint64_t first, uint64_t m, uint64_t requested, uint64_t dflt) {
  const uint64_t k = m - first;
  const uint64_t wr = dict_save_window_records(requested, dflt, k);
  REQUIRE(wr >= 1 && (k == 0 || wr <= k));
  if (requested && requested <= k) REQUIRE(wr == requested);
  const uint64_t nw = dict_save_windows(k, wr);
  REQUIRE(nw == (k + wr - 1) / wr);
  REQUIRE(dict_save_cut(first, m, wr, 0) == (k ? first : m));
  uint64_t at = first;
  for (uint64_t w = 0; w < nw; ++w) {
    const uint64_t a = dict_save_cut(first, m, wr, w), b = dict_save_cut(first, m, wr, w + 1);
    if (a != at || b <= a || b - a > wr || (w + 1 < nw && b - a != wr)) REQUIRE(!"window cut");
    at = b;
  }
  REQUIRE(at == m);
  REQUIRE(dict_save_cut(first, m, wr, nw) == m && dict_save_cut(first, m, wr, nw + 5) == m);
  return 0;
}

static int check_windows() {
  for (uint64_t k : {0ull, 1ull, 2ull, 63ull, 64ull, 65ull, 4097ull})
    for (uint64_t first : {0ull, 5ull, 1ull << 31}) {
      std::vector<uint64_t> wrs = {0, 1, 7, 64, k, k + 1};
      if (k) wrs.push_back(k - 1);
      for (uint64_t wr : wrs)
        if (check_cuts(first, first + k, wr, 1000)) return 1;
    }
  // the largest dict in one default window and in windows of one record
  REQUIRE(dict_save_windows(0xFFFFFFFEull, 1) == 0xFFFFFFFEull);
  REQUIRE(dict_save_cut(0, 0xFFFFFFFEull, 1, 0xFFFFFFFDull) == 0xFFFFFFFDull);
  REQUIRE(dict_save_window_records(0, 0, 10) == 1);      // a default of 0 still moves
  REQUIRE(dict_save_window_records(0, 2796202, 100) == 100);
  REQUIRE(dict_save_window_records(~0ull, 5, 100) == 100);
  REQUIRE(dict_save_windows(0, 1) == 0);
  return 0;
}

static int check_refusals() {
  ngpu_dict_save_options o;
  memset(&o, 0, sizeof o);
  REQUIRE(dict_save_check(o, 0, 0, false) == kSaveOk);
  REQUIRE(dict_save_check(o, 10, 3, true) == kSaveOk);
  REQUIRE(dict_save_check(o, 0, 3, false) == kSaveOk);   // no records: nothing is dropped
  REQUIRE(dict_save_check(o, 10, 0, false) == kSaveOk);  // no blobs either
  REQUIRE(dict_save_check(o, 10, 3, false) == kSaveNoBlobTable);
  o.flags = NGPU_DICT_SAVE_NO_BLOB_TABLE;
  REQUIRE(dict_save_check(o, 10, 3, false) == kSaveOk);
  REQUIRE(dict_save_blob_rows(o, 3, false) == 0 && dict_save_blob_rows(o, 3, true) == 0);
  for (uint32_t f : {0x2u, 0x3u, 0x80000000u, 0xFFFFFFFEu}) {
    o.flags = f;
    REQUIRE(dict_save_check(o, 10, 3, true) == kSaveBadFlags);
  }
  o.flags = 0;
  for (int r = 0; r < 2; ++r) {
    o.reserved[r] = 1;
    REQUIRE(dict_save_check(o, 10, 3, true) == kSaveBadReserved);
    o.reserved[r] = 1ull << 63;
    REQUIRE(dict_save_check(o, 10, 3, true) == kSaveBadReserved);
    o.reserved[r] = 0;
  }
  o.first_entry = 10;
  REQUIRE(dict_save_check(o, 10, 3, true) == kSaveOk);  // an empty tail
  o.first_entry = 11;
  REQUIRE(dict_save_check(o, 10, 3, true) == kSaveBadFirstEntry);
  o.first_entry = ~0ull;
  REQUIRE(dict_save_check(o, 10, 3, true) == kSaveBadFirstEntry);
  o.first_entry = 4;
  o.first_blob = 3;
  REQUIRE(dict_save_check(o, 10, 3, true) == kSaveOk);
  REQUIRE(dict_save_blob_rows(o, 3, true) == 0);
  o.first_blob = 1;
  REQUIRE(dict_save_blob_rows(o, 3, true) == 2 && dict_save_blob_rows(o, 3, false) == 0);
  o.first_blob = 4;
  REQUIRE(dict_save_check(o, 10, 3, true) == kSaveBadFirstBlob);
  o.first_blob = 0xFFFFFFFFu;
  REQUIRE(dict_save_check(o, 10, 3, true) == kSaveBadFirstBlob);
  o.first_blob = 0;
  o.first_entry = 0;
  REQUIRE(dict_save_check(o, 0xFFFFFFFFull, 1, true) == kSaveTooLarge);
  REQUIRE(dict_save_check(o, 1, (1u << 20) + 1, true) == kSaveTooLarge);
  REQUIRE(dict_save_check(o, 0xFFFFFFFEull, 1u << 20, true) == kSaveOk);
  for (int r = kSaveBadFlags; r <= kSaveTooLarge; ++r) REQUIRE(dict_save_refusal((DictSaveRefusal)r)[0] != 0);
  REQUIRE(dict_save_refusal(kSaveOk)[0] == 0);
  return 0;
}

int main() {
  if (check_layout() || check_header() || check_windows() || check_refusals()) return 1;
  printf("ok %d\n", checks);
  return 0;
}
