// node_fold_plan_test.cpp — node dict fold's host plan (csrc/node_fold_plan.hpp)
// on the CPU, run by tests/test_node_fold_plan.py under ASan/UBSan: record and
// blob offsets, per-owner totals, both ends of every (source, owner) segment, the
// limits and refusal rules, and the restatement of the stable split by owner
// against a brute-force walk.
// usage: node_fold_plan_test -> "ok <checks>".
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>
#include <vector>

#include "node_fold_plan.hpp"

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

// Digest word 0 whose first two digest bytes are the big-endian prefix p.
static uint32_t word0(uint32_t p, uint32_t noise) { return (p >> 8) | ((p & 0xFF) << 8) | (noise << 16); }

// The plan against the plainest statement: concatenate the parts' rows, walk them.
static int check_plan(uint32_t W, const std::vector<std::vector<uint32_t>> &rows_w0,
                      const std::vector<uint64_t> &b, bool partitioned) {
  std::vector<uint64_t> k(W);
  std::vector<uint32_t> c((size_t)W * W, 0);
  for (uint32_t i = 0; i < W; ++i) {
    k[i] = rows_w0[i].size();
    for (uint32_t w : rows_w0[i]) ++c[(size_t)i * W + owner_of(w, W)];
  }
  const NodeFoldPlan p = node_fold_plan(W, k.data(), b.data(), partitioned ? c.data() : nullptr);
  REQUIRE(p.ok);
  REQUIRE(p.off.size() == W + 1 && p.boff.size() == W + 1 && p.off[0] == 0 && p.boff[0] == 0);
  uint64_t K = 0, B = 0;
  for (uint32_t i = 0; i < W; ++i) {
    if (p.off[i] != K || p.boff[i] != B) REQUIRE(!"offsets");
    K += k[i];
    B += b[i];
  }
  REQUIRE(p.K == K && p.B == B && p.off[W] == K && p.boff[W] == B);
  if (!partitioned) {
    REQUIRE(p.total.empty() && p.src.empty() && p.dst.empty());
    return 0;
  }
  // owner o's new rows in global order: (part, position) pairs
  std::vector<std::vector<uint64_t>> want(W);  // global row number of each of o's rows
  for (uint32_t i = 0; i < W; ++i)
    for (uint64_t r = 0; r < k[i]; ++r) want[owner_of(rows_w0[i][r], W)].push_back(p.off[i] + r);
  // what the copies produce: part i's split rows (owners back to back, stable),
  // segment (i, o) copied to dst[i][o]
  std::vector<std::vector<uint64_t>> got(W);
  for (uint32_t o = 0; o < W; ++o) got[o].assign(p.total[o], ~0ull);
  for (uint32_t i = 0; i < W; ++i) {
    const NodeFoldSplit s = node_fold_split(rows_w0[i].data(), k[i], W);
    std::vector<uint64_t> split(k[i], ~0ull);
    for (uint64_t r = 0; r < k[i]; ++r) {
      if (s.dest[r] >= k[i] || split[s.dest[r]] != ~0ull) REQUIRE(!"split destination");
      split[s.dest[r]] = p.off[i] + r;
    }
    for (uint32_t o = 0; o < W; ++o) {
      const uint64_t n = c[(size_t)i * W + o], from = p.src[(size_t)i * W + o], to = p.dst[(size_t)i * W + o];
      if (s.count[o] != n) REQUIRE(!"owner count");
      if (from + n > k[i] || to + n > p.total[o]) REQUIRE(!"segment bounds");
      for (uint64_t j = 0; j < n; ++j) got[o][to + j] = split[from + j];
    }
  }
  for (uint32_t o = 0; o < W; ++o) {
    REQUIRE(p.total[o] == want[o].size());
    REQUIRE(got[o] == want[o]);
  }
  return 0;
}

// The split's restatement against a walk: owner o's rows start after those of the
// owners below it and keep their order.
static int check_split(const std::vector<uint32_t> &w0, uint32_t W) {
  const uint64_t k = w0.size();
  const NodeFoldSplit s = node_fold_split(w0.data(), k, W);
  REQUIRE(s.T == (k + 255) / 256 && s.base.size() == (size_t)W * s.T && s.dest.size() == k);
  std::vector<uint64_t> tot(W, 0), start(W, 0), seen(W, 0);
  for (uint32_t w : w0) ++tot[owner_of(w, W)];
  for (uint32_t o = 1; o < W; ++o) start[o] = start[o - 1] + tot[o - 1];
  for (uint64_t r = 0; r < k; ++r) {
    const uint32_t o = owner_of(w0[r], W);
    if (s.dest[r] != start[o] + seen[o]++) REQUIRE(!"stable destination");
  }
  for (uint32_t o = 0; o < W; ++o)
    if (s.count[o] != tot[o]) REQUIRE(!"owner total");
  ++checks;
  return 0;
}

int main() {
  const uint32_t Ws[] = {1, 2, 3, 5, 8, 64};
  const uint64_t sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, 1025};
  // the split: random prefixes, all rows on one owner, prefixes on both sides of
  // every owner boundary and 0xFFFF, runs of one owner as long as a wave
  for (uint32_t W : Ws)
    for (uint64_t k : sizes) {
      std::vector<uint32_t> w0(k);
      for (uint32_t &w : w0) w = (uint32_t)rnd();
      if (check_split(w0, W)) return 1;
      for (uint32_t one : {0u, W - 1}) {
        for (uint64_t r = 0; r < k; ++r) {
          // a prefix owner `one` owns: the smallest p with (p * W) >> 16 == one
          const uint32_t p = (uint32_t)((((uint64_t)one << 16) + W - 1) / W);
          w0[r] = word0(p, (uint32_t)rnd() & 0xFFFF);
        }
        if (check_split(w0, W)) return 1;
      }
      for (uint64_t r = 0; r < k; ++r) {
        const uint32_t o = (uint32_t)(rnd() % W);
        const uint32_t lo = (uint32_t)((((uint64_t)o << 16) + W - 1) / W);
        const uint32_t edge[] = {lo, lo ? lo - 1 : 0, 0xFFFFu};
        w0[r] = word0(edge[rnd() % 3], (uint32_t)rnd() & 0xFFFF);
      }
      if (check_split(w0, W)) return 1;
      for (uint64_t r = 0; r < k; ++r) {
        const uint32_t o = (uint32_t)((r / 64) % W);
        w0[r] = word0((uint32_t)((((uint64_t)o << 16) + W - 1) / W), (uint32_t)r);
      }
      if (check_split(w0, W)) return 1;
    }
  // the boundary prefixes really sit on both sides
  for (uint32_t W : Ws)
    for (uint32_t o = 1; o < W; ++o) {
      const uint32_t lo = (uint32_t)((((uint64_t)o << 16) + W - 1) / W);
      REQUIRE(owner_of(word0(lo, 7), W) == o && owner_of(word0(lo - 1, 7), W) == o - 1);
      REQUIRE(owner_of(word0(0xFFFF, 7), W) == W - 1);
    }

  // the plan: every part size against every other, an empty part, both modes
  for (uint32_t W : Ws) {
    for (int round = 0; round < 6; ++round) {
      std::vector<std::vector<uint32_t>> rows(W);
      std::vector<uint64_t> b(W);
      for (uint32_t i = 0; i < W; ++i) {
        const uint64_t k = round == 0 ? 0 : sizes[(i + round) % 9];
        rows[i].resize(i == 1 && round == 2 ? 0 : k);  // an empty part among full ones
        for (uint32_t &w : rows[i])
          w = round == 3 ? word0(0, (uint32_t)rnd() & 0xFFFF) : (uint32_t)rnd();  // all on owner 0
        b[i] = rows[i].empty() ? 0 : 1 + rnd() % (rows[i].size() < 4 ? rows[i].size() : 4);
      }
      if (check_plan(W, rows, b, false) || check_plan(W, rows, b, true)) return 1;
    }
  }
  {  // owner counts that do not add up to k name the part
    const uint64_t k[3] = {4, 5, 6}, b[3] = {1, 1, 1};
    uint32_t c[9] = {1, 1, 2, 2, 2, 1, 3, 2, 1};
    REQUIRE(node_fold_plan(3, k, b, c).ok);
    c[8] = 2;
    const NodeFoldPlan p = node_fold_plan(3, k, b, c);
    REQUIRE(!p.ok && p.bad == 2);
    c[3] = 0;
    const NodeFoldPlan q = node_fold_plan(3, k, b, c);
    REQUIRE(!q.ok && q.bad == 1);
  }

  // limits
  REQUIRE(node_fold_limits(0, 0, 0, 0) == kNodeFoldFits);
  REQUIRE(node_fold_limits(100, 3, 0xFFFFFFFFull - 101, 1) == kNodeFoldFits);
  REQUIRE(node_fold_limits(100, 3, 0xFFFFFFFFull - 100, 1) == kNodeFoldEntries);
  REQUIRE(node_fold_limits(0xFFFFFFFFull, 0, 0, 0) == kNodeFoldEntries);
  REQUIRE(node_fold_limits(10, 5, 10, (1u << 20) - 5) == kNodeFoldFits);
  REQUIRE(node_fold_limits(10, 5, 10, (1u << 20) - 4) == kNodeFoldBlobs);
  REQUIRE(node_fold_limits(10, 0, 10, (1ull << 20) + 1) == kNodeFoldBlobs);
  REQUIRE(node_fold_limits(10, 0, 10, 1ull << 33) == kNodeFoldBlobs);

  // the refusal rules are dict fold's, over the sums
  {
    const uint64_t k[2] = {3, 4}, b[2] = {1, 2};
    const NodeFoldPlan p = node_fold_plan(2, k, b, nullptr);
    REQUIRE(node_fold_place_rule(10, true, true, 7, p) == kPlaceKept);
    REQUIRE(node_fold_place_rule(10, true, true, 3, p) == kPlaceCount);   // one part's k is not enough
    REQUIRE(node_fold_place_rule(10, true, true, 4, p) == kPlaceCount);
    REQUIRE(node_fold_place_rule(10, true, false, 0, p) == kPlaceMissing);
    REQUIRE(node_fold_place_rule(10, false, true, 7, p) == kPlaceUnwanted);
    REQUIRE(node_fold_place_rule(10, false, false, 0, p) == kPlaceNone);
    REQUIRE(node_fold_place_rule(0, false, true, 7, p) == kPlaceKept);    // an empty base goes with either
    REQUIRE(node_fold_place_rule(0, false, false, 0, p) == kPlaceNone);
    REQUIRE(node_fold_table_rows_ok(true, 3, p) && !node_fold_table_rows_ok(true, 2, p) &&
            !node_fold_table_rows_ok(true, 1, p) && node_fold_table_rows_ok(false, 0, p));
    REQUIRE(node_fold_table_rule(2, true, true, 3, p) == kTableKept);
    REQUIRE(node_fold_table_rule(2, true, false, 0, p) == kTableBaseOnly);
    REQUIRE(node_fold_table_rule(2, false, true, 3, p) == kTableCallOnly);
    REQUIRE(node_fold_table_rule(2, false, false, 0, p) == kTableNone);
    REQUIRE(node_fold_table_rule(0, false, true, 3, p) == kTableKept);
    const uint64_t z[2] = {0, 0};
    const NodeFoldPlan e = node_fold_plan(2, z, z, nullptr);
    REQUIRE(e.K == 0 && e.B == 0);
    REQUIRE(node_fold_place_rule(10, true, false, 0, e) == kPlaceBase);
    REQUIRE(node_fold_place_rule(10, true, true, 0, e) == kPlaceBase);
    REQUIRE(node_fold_place_rule(10, true, true, 1, e) == kPlaceCount);
    REQUIRE(node_fold_table_rule(2, true, false, 0, e) == kTableKept);   // nothing added: base's table
  }
  printf("ok %d\n", checks);
  return 0;
}
