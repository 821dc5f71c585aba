// verity_verify_plan_test.cpp — where a stored hash block sits and what it
// answers for (csrc/verity_verify_plan.hpp) on the CPU, run by
// tests/test_verity_verify_oracle.py under ASan/UBSan.  Every tree block's
// (level, index, parent offset, digests used, covered data range) against a
// brute-force walk: for random image sizes up to 2^62 the first, last and a few
// random blocks of every level (128-bit arithmetic on the reference side); for
// small trees every block, with the covered range gathered from every data
// block's own chain of ancestors.  usage: verity_verify_plan_test SEED ->
// "ok <cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "verity_verify_plan.hpp"

using namespace ngpu;
typedef unsigned __int128 u128;

#define REQUIRE(c)                                                                       \
  do {                                                                                   \
    if (!(c)) {                                                                          \
      printf("FAILED %s (line %d, %llu blocks, tree block %llu)\n", #c, __LINE__,        \
             (unsigned long long)p.data_blocks, (unsigned long long)t);                  \
      return false;                                                                      \
    }                                                                                    \
  } while (0)

// Tree block t of plan p against a walk down the levels from the top.
static bool check_block(const VerityPlan &p, const VerityGeom &g, uint64_t t) {
  uint64_t at = 0, parent_first = 0;
  uint32_t l = p.levels;
  bool found = false;
  while (l-- > 0) {  // the top level first
    if (t < at + p.blocks[l]) {
      found = true;
      break;
    }
    parent_first = at;
    at += p.blocks[l];
  }
  REQUIRE(found);
  const uint64_t j = t - at;
  const VerityBlockLoc b = verity_locate(g, t);
  REQUIRE(b.level == l && b.index == j);
  if (l + 1 == p.levels)
    REQUIRE(b.parent_off == kVerityNoParent && t == 0);
  else
    REQUIRE((u128)b.parent_off == (u128)parent_first * 4096 + (u128)32 * j);
  // the slot lies inside a block of the level above that exists
  if (l + 1 < p.levels) REQUIRE(b.parent_off / 4096 == p.first[l + 1] + j / 128 && j / 128 < p.blocks[l + 1]);
  const u128 below = l ? p.blocks[l - 1] : p.data_blocks;
  const u128 rest = below - (u128)128 * j;
  REQUIRE(rest >= 1 && (u128)b.used == (rest < 128 ? rest : 128));
  REQUIRE(b.last_of_level == (j + 1 == p.blocks[l]));
  if (!b.last_of_level) REQUIRE(b.used == 128);
  u128 span = 1;
  for (uint32_t i = 0; i <= l; ++i) span *= 128;
  const u128 end = (u128)(j + 1) * span;
  REQUIRE((u128)b.first_data == (u128)j * span);
  REQUIRE((u128)b.last_data == (end < p.data_blocks ? end : (u128)p.data_blocks) - 1);
  REQUIRE(b.first_data <= b.last_data && b.last_data < p.data_blocks);
  return true;
}

// Every block of a small tree; the covered ranges from the data blocks' side.
static bool check_small(uint64_t blocks) {
  VerityPlan p;
  uint64_t t = 0;
  REQUIRE(verity_plan(blocks * 512, &p));
  const VerityGeom g = verity_geom(p);
  REQUIRE(g.tree_blocks == p.tree_blocks && g.levels == p.levels && g.data_blocks == blocks);
  std::vector<uint64_t> lo(p.tree_blocks, ~0ull), hi(p.tree_blocks, 0), used(p.tree_blocks, 0);
  for (uint64_t d = 0; d < blocks; ++d) {
    uint64_t c = d;  // index of the ancestor's child in the level below
    for (uint32_t l = 0; l < p.levels; ++l) {
      const uint64_t blk = p.first[l] + c / 128;
      if (d < lo[blk]) lo[blk] = d;
      if (d > hi[blk]) hi[blk] = d;
      c /= 128;
    }
  }
  for (uint32_t l = 0; l < p.levels; ++l) {
    const uint64_t below = l ? p.blocks[l - 1] : blocks;
    for (uint64_t c = 0; c < below; ++c) ++used[p.first[l] + c / 128];
  }
  for (t = 0; t < p.tree_blocks; ++t) {
    if (!check_block(p, g, t)) return false;
    const VerityBlockLoc b = verity_locate(g, t);
    REQUIRE(b.first_data == lo[t] && b.last_data == hi[t] && b.used == used[t]);
  }
  return true;
}

int main(int argc, char **argv) {
  std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
  int tc = 0;
  for (; tc < 20000; ++tc) {
    uint64_t blocks = (rng() >> (rng() % 64)) % (kVerityMaxData / 512);
    if (tc % 8 == 1) {
      uint64_t q = 1;
      for (uint64_t k = rng() % 8; k; --k) q *= 128;
      blocks = q + rng() % 3 - 1;
    }
    if (tc % 16 == 2) blocks = kVerityMaxData / 512 - 1 - rng() % 4;
    if (blocks == 0) blocks = 1;
    VerityPlan p;
    if (!verity_plan(blocks * 512, &p)) {
      printf("FAILED verity_plan(%llu blocks)\n", (unsigned long long)blocks);
      return 1;
    }
    const VerityGeom g = verity_geom(p);
    for (uint32_t l = 0; l < p.levels; ++l) {
      const uint64_t n = p.blocks[l];
      const uint64_t picks[] = {0, n - 1, n / 2, n > 1 ? n - 2 : 0, rng() % n, rng() % n};
      for (uint64_t j : picks)
        if (!check_block(p, g, p.first[l] + j)) return 1;
    }
  }
  // small trees: every block; the sizes at which a block or a level begins or ends
  for (uint64_t blocks = 1; blocks <= 700; ++blocks)
    if (!check_small(blocks)) return 1;
  for (uint64_t blocks : {16383ull, 16384ull, 16385ull, 16514ull, 32769ull, 2097151ull, 2097152ull, 2097153ull})
    if (!check_small(blocks)) return 1;
  printf("ok %d\n", tc);
  return 0;
}
