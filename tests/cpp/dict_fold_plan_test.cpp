// dict_fold_plan_test.cpp — dict fold's host bookkeeping (csrc/dict_fold_plan.hpp)
// on the CPU, run by tests/test_dict_fold_plan.py under ASan/UBSan: the blob-table
// and placement decision tables, the layer-cut check, and the restatement of the
// kernels (keep words, prefixes, record positions, blob ranks) against a
// brute-force loop over random kinds and layer cuts.
// usage: dict_fold_plan_test -> "ok <checks>".
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "dict_fold_plan.hpp"

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

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return lcg_state >> 33;
}

// The map against the plainest statement of the header's words: walk the chunks
// layer by layer, count.
static int check_map(const std::vector<uint32_t> &kinds, const std::vector<uint64_t> &first) {
  const uint64_t n = kinds.size(), L = first.size() - 1;
  uint64_t bad = ~0ull;
  REQUIRE(dict_fold_layers_ok(first.data(), L, n, &bad));
  const DictFoldMap f = dict_fold_map(kinds.data(), n, first.data(), L);
  REQUIRE(f.ok);
  REQUIRE(f.words.size() == (n + 63) / 64 && f.prefix.size() == f.words.size() && f.lrank.size() == L);
  uint64_t k = 0, b = 0;
  for (uint64_t l = 0; l < L; ++l) {
    bool any = false;
    if (f.lrank[l] != b) REQUIRE(!"layer rank");
    for (uint64_t c = first[l]; c < first[l + 1]; ++c) {
      if (kinds[c] != 0) continue;
      any = true;
      if (f.position(c) != k) REQUIRE(!"record position");
      if (DictFoldMap::layer_of(first.data(), L, c) != l) REQUIRE(!"layer of a chunk");
      ++k;
    }
    b += any;
  }
  ++checks;
  REQUIRE(f.k == k && f.b == b);
  for (uint64_t c = 0, r = 0; c <= n; ++c) {  // rank(c): NEW chunks before c
    if (f.rank(c, n) != r) REQUIRE(!"rank");
    if (c < n) r += kinds[c] == 0;
  }
  // no keep bit past n
  if (n % 64) REQUIRE((f.words.back() >> (n % 64)) == 0);
  // one layer (no cuts) sees the same positions and at most one blob
  const DictFoldMap one = dict_fold_map(kinds.data(), n, nullptr, 77);
  REQUIRE(one.ok && one.k == k && one.b == (k ? 1u : 0u) && one.lrank.size() == 1 && one.lrank[0] == 0);
  REQUIRE(one.words == f.words && one.prefix == f.prefix);
  return 0;
}

int main() {
  // ---- the blob table rule (ngpu_dict_extend's) ----
  // base_blobs, base_has, call_has, k, n_blobs
  REQUIRE(dict_table_rule(0, false, false, 5, 0) == kTableNone);   // a base of 0 blobs goes with either
  REQUIRE(dict_table_rule(0, false, true, 5, 2) == kTableKept);
  REQUIRE(dict_table_rule(0, false, false, 0, 0) == kTableNone);
  REQUIRE(dict_table_rule(3, true, true, 5, 2) == kTableKept);     // both sides
  REQUIRE(dict_table_rule(3, false, false, 5, 2) == kTableNone);   // neither: a count only
  REQUIRE(dict_table_rule(3, true, false, 5, 2) == kTableBaseOnly);  // exactly one side: refused
  REQUIRE(dict_table_rule(3, true, false, 5, 0) == kTableBaseOnly);
  REQUIRE(dict_table_rule(3, false, true, 5, 2) == kTableCallOnly);
  REQUIRE(dict_table_rule(3, true, false, 0, 0) == kTableKept);    // a call that adds nothing
  REQUIRE(dict_table_rule(3, false, false, 0, 0) == kTableNone);
  REQUIRE(dict_table_rule(3, false, true, 0, 1) == kTableCallOnly);  // (a table row is something)
  REQUIRE(dict_table_rule(0, true, false, 5, 1) == kTableBaseOnly);  // 0 blobs but a (0-row) table kept
  // ---- the placement rule ----
  // base_m, base_keeps, given, n_placements, k
  REQUIRE(dict_fold_place_rule(100, true, true, 7, 7) == kPlaceKept);
  REQUIRE(dict_fold_place_rule(100, true, true, 6, 7) == kPlaceCount);
  REQUIRE(dict_fold_place_rule(100, true, true, 8, 7) == kPlaceCount);
  REQUIRE(dict_fold_place_rule(100, true, false, 0, 7) == kPlaceMissing);
  REQUIRE(dict_fold_place_rule(100, false, true, 7, 7) == kPlaceUnwanted);
  REQUIRE(dict_fold_place_rule(100, false, false, 0, 7) == kPlaceNone);
  REQUIRE(dict_fold_place_rule(0, false, true, 7, 7) == kPlaceKept);   // an empty base goes with either
  REQUIRE(dict_fold_place_rule(0, false, false, 0, 7) == kPlaceNone);
  REQUIRE(dict_fold_place_rule(100, true, false, 0, 0) == kPlaceBase);   // k == 0: the base
  REQUIRE(dict_fold_place_rule(100, true, true, 0, 0) == kPlaceBase);
  REQUIRE(dict_fold_place_rule(100, false, true, 0, 0) == kPlaceBase);
  REQUIRE(dict_fold_place_rule(100, false, true, 1, 0) == kPlaceCount);  // the count comes first
  REQUIRE(dict_fold_place_rule(100, false, true, 6, 7) == kPlaceCount);
  // ---- layer cuts ----
  {
    uint64_t bad = 99;
    const uint64_t ok1[] = {0, 10}, ok2[] = {0, 0, 4, 4, 10, 10};
    REQUIRE(dict_fold_layers_ok(ok1, 1, 10, &bad) && dict_fold_layers_ok(ok2, 5, 10, &bad) && bad == 99);
    const uint64_t z[] = {0, 0};
    REQUIRE(dict_fold_layers_ok(z, 1, 0, nullptr));
    const uint64_t a[] = {1, 10};
    REQUIRE(!dict_fold_layers_ok(a, 1, 10, &bad) && bad == 0);   // first[0] != 0
    const uint64_t b[] = {0, 4, 9};
    REQUIRE(!dict_fold_layers_ok(b, 2, 10, &bad) && bad == 1);   // does not end at n
    const uint64_t c[] = {0, 6, 4, 10};
    REQUIRE(!dict_fold_layers_ok(c, 3, 10, &bad) && bad == 1);   // a decreasing entry
    const uint64_t d[] = {0, 11, 10};
    REQUIRE(!dict_fold_layers_ok(d, 2, 10, &bad) && bad == 0);   // past n
    const uint64_t e[] = {0, 4, 12};
    REQUIRE(!dict_fold_layers_ok(e, 2, 10, nullptr));
  }
  // ---- kinds that are no dedup outcome ----
  for (uint32_t bad_kind : {3u, 4u, 7u, 0xFFFFFFFFu}) {
    std::vector<uint32_t> kinds(200, 0);
    for (uint64_t at : {(uint64_t)0, (uint64_t)100, (uint64_t)199}) {
      kinds.assign(200, 1);
      kinds[at] = bad_kind;
      kinds[199] = kinds[199] == 1 ? 5 : kinds[199];  // a later one: the first is named
      const DictFoldMap f = dict_fold_map(kinds.data(), 200, nullptr, 1);
      REQUIRE(!f.ok && f.bad_chunk == at);
    }
  }
  // ---- positions and blob ranks against the brute-force walk ----
  for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 1000ull, 16383ull, 16384ull,
                     16385ull, 32769ull}) {
    for (int pattern = 0; pattern < 7; ++pattern) {
      std::vector<uint32_t> kinds(n);
      for (uint64_t c = 0; c < n; ++c) {
        const uint32_t other = 1 + (uint32_t)(rnd() & 1);  // INTRA or DICT
        const bool is_new = pattern == 0 ? true : pattern == 1 ? false : pattern == 2 ? (c & 1) == 0
                            : pattern == 3 ? ((c >> 6) & 1) == 0 : pattern == 4 ? c == 0
                            : pattern == 5 ? c == n - 1 : rnd() % 10 < 3;
        kinds[c] = is_new ? 0 : other;
      }
      for (uint64_t L : {1ull, 2ull, 3ull, 64ull, 257ull, 1025ull}) {
        // random cuts, with empty layers in front, in the middle and at the end
        std::vector<uint64_t> first(L + 1, 0);
        for (uint64_t l = 1; l < L; ++l) first[l] = n ? rnd() % (n + 1) : 0;
        first[L] = n;
        for (uint64_t l = 1; l < L; ++l)  // sort (insertion: L is small)
          for (uint64_t j = l; j > 1 && first[j - 1] > first[j]; --j) {
            const uint64_t t = first[j];
            first[j] = first[j - 1], first[j - 1] = t;
          }
        if (L >= 3) first[1] = 0, first[L - 1] = n;  // an empty first and last layer
        if (L >= 64) first[L / 2] = first[L / 2 + 1];
        if (L >= 64 && n >= 128) first[2] = 64, first[3] = 64 + 37 < n ? 64 + 37 : n;  // on / inside a keep word
        for (uint64_t l = 1; l <= L; ++l)
          if (first[l] < first[l - 1]) first[l] = first[l - 1];
        first[L] = n;
        for (uint64_t l = L; l-- > 0;)
          if (first[l] > first[l + 1]) first[l] = first[l + 1];
        if (check_map(kinds, first)) return 1;
      }
    }
  }
  // what the numbers are, spelled out once: N I N | (empty) | D I | N
  {
    const uint32_t kinds[] = {0, 1, 0, 2, 1, 0};
    const uint64_t first[] = {0, 3, 3, 5, 6};
    const DictFoldMap f = dict_fold_map(kinds, 6, first, 4);
    REQUIRE(f.ok && f.k == 3 && f.b == 2 && f.words[0] == 0x25);
    REQUIRE(f.lrank[0] == 0 && f.lrank[1] == 1 && f.lrank[2] == 1 && f.lrank[3] == 1);
    REQUIRE(f.position(0) == 0 && f.position(2) == 1 && f.position(5) == 2);
    REQUIRE(DictFoldMap::layer_of(first, 4, 2) == 0 && DictFoldMap::layer_of(first, 4, 3) == 2 &&
            DictFoldMap::layer_of(first, 4, 5) == 3);
  }
  // ---- the scratch layout: the offsets written out by hand ----
  for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 16383ull, 16384ull, 16385ull})
    for (uint64_t L : {1ull, 2ull, 1000ull})
      for (uint64_t cb : {8ull * kFoldCtrWords, 8ull * kFoldCtrWords + 4 * 64}) {  // dict fold's, node fold's
        const uint64_t nw = (n + 63) / 64, nt = (nw + 255) / 256;
        const FoldScratch s = fold_scratch_layout(n, L, cb);
        REQUIRE(dict_retire_scan_tiles(n) == nt);
        REQUIRE(s.words == 0 && s.sums == 8 * nw && s.ctr == 8 * nw + 8 * (nt + 1));
        REQUIRE(s.cnt == 8 * nw + 8 * (nt + 1) + cb && s.rank == 8 * nw + 8 * (nt + 1) + cb + 4 * nw);
        REQUIRE(s.bytes == 8 * nw + 8 * (nt + 1) + cb + 4 * nw + 4 * L);
        REQUIRE(s.words % 8 == 0 && s.sums % 8 == 0 && s.ctr % 8 == 0 && s.cnt % 4 == 0 && s.rank % 4 == 0);
        REQUIRE(s.words + 8 * nw <= s.sums && s.sums + 8 * (nt + 1) <= s.ctr && s.ctr + cb <= s.cnt &&
                s.cnt + 4 * nw <= s.rank && s.rank + 4 * L <= s.bytes);
      }
  // ---- the counters' verdict: layer, then kind, then length, then insane ----
  {
    const uint64_t n = 100, L = 7;
    auto ctr_of = [](uint64_t k, uint64_t b, bool layer, bool kind, bool len) {
      std::vector<uint64_t> c(kFoldCtrWords, 0);
      c[kFoldK] = k, c[kFoldBlobs] = b;
      if (layer) c[kFoldBadLayer1] = ~5ull;
      if (kind) c[kFoldBadKind] = 3, c[kFoldBadKind1] = ~41ull;
      if (len) c[kFoldBadLen] = 2, c[kFoldBadLen1] = ~0ull;  // chunk 0: ~0 is not "none"
      return c;
    };
    FoldVerdict v = fold_counts_verdict(ctr_of(10, 3, false, false, false).data(), n, L);
    REQUIRE(v.why == FoldVerdict::ok && v.k == 10 && v.b == 3);
    v = fold_counts_verdict(ctr_of(10, 3, true, false, false).data(), n, L);
    REQUIRE(v.why == FoldVerdict::bad_layer && v.which == 5);
    v = fold_counts_verdict(ctr_of(10, 3, false, true, false).data(), n, L);
    REQUIRE(v.why == FoldVerdict::bad_kind && v.which == 41 && v.count == 3);
    v = fold_counts_verdict(ctr_of(10, 3, false, false, true).data(), n, L);
    REQUIRE(v.why == FoldVerdict::bad_len && v.which == 0 && v.count == 2 && v.k == 10 && v.b == 3);
    // pairs (and an insane count under each refusal): the earlier one is named
    REQUIRE(fold_counts_verdict(ctr_of(10, 3, true, true, false).data(), n, L).why == FoldVerdict::bad_layer);
    REQUIRE(fold_counts_verdict(ctr_of(10, 3, true, false, true).data(), n, L).why == FoldVerdict::bad_layer);
    REQUIRE(fold_counts_verdict(ctr_of(10, 3, false, true, true).data(), n, L).why == FoldVerdict::bad_kind);
    REQUIRE(fold_counts_verdict(ctr_of(n + 1, 3, true, false, false).data(), n, L).why == FoldVerdict::bad_layer);
    REQUIRE(fold_counts_verdict(ctr_of(n + 1, 3, false, true, false).data(), n, L).why == FoldVerdict::bad_kind);
    REQUIRE(fold_counts_verdict(ctr_of(n + 1, 3, false, false, true).data(), n, L).why == FoldVerdict::bad_len);
    // the sanity bounds at equality and one past it: k <= n, b <= L, b <= k
    REQUIRE(fold_counts_verdict(ctr_of(n, L, false, false, false).data(), n, L).why == FoldVerdict::ok);
    v = fold_counts_verdict(ctr_of(n + 1, L, false, false, false).data(), n, L);
    REQUIRE(v.why == FoldVerdict::insane && v.k == n + 1 && v.b == L);
    REQUIRE(fold_counts_verdict(ctr_of(n, L + 1, false, false, false).data(), n, L).why == FoldVerdict::insane);
    REQUIRE(fold_counts_verdict(ctr_of(4, 4, false, false, false).data(), n, L).why == FoldVerdict::ok);
    REQUIRE(fold_counts_verdict(ctr_of(4, 5, false, false, false).data(), n, L).why == FoldVerdict::insane);
    REQUIRE(fold_counts_verdict(ctr_of(0, 0, false, false, false).data(), 0, 1).why == FoldVerdict::ok);
    REQUIRE(fold_counts_verdict(ctr_of(1, 0, false, false, false).data(), 0, 1).why == FoldVerdict::insane);
  }
  printf("ok %d\n", checks);
  return 0;
}
