// verity_plan_test.cpp — the dm-verity tree geometry (csrc/verity_plan.hpp) on
// the CPU, run by tests/test_verity_oracle.py under ASan/UBSan: random image
// sizes up to 2^62, the levels contiguous and top first, their sum the tree,
// nothing overflowing (the reference values are computed in 128-bit
// arithmetic).  usage: verity_plan_test SEED -> "ok <cases>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "verity_plan.hpp"

using namespace ngpu;
typedef unsigned __int128 u128;

#define REQUIRE(c)                                                \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s (line %d, case %d)\n", #c, __LINE__, tc); \
      return 1;                                                   \
    }                                                             \
  } while (0)

int main(int argc, char **argv) {
  std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
  int tc = 0;
  for (; tc < 20000; ++tc) {
    // sizes of every magnitude; every 8th next to a power of 128 blocks, every
    // 16th just below the 2^62 limit
    uint64_t blocks = (rng() >> (rng() % 64)) % (kVerityMaxData / 512);
    if (tc % 8 == 1) {
      uint64_t p = 1;
      for (uint64_t k = rng() % 8; k; --k) p *= 128;
      blocks = p + rng() % 3 - 1;
    }
    if (tc % 16 == 2) blocks = kVerityMaxData / 512 - 1 - rng() % 4;
    if (blocks == 0) blocks = 1;
    const uint64_t bytes = blocks * 512;
    VerityPlan p;
    REQUIRE(verity_plan(bytes, &p));
    REQUIRE(p.data_blocks == blocks);
    REQUIRE(p.hash_offset >= bytes && p.hash_offset - bytes < 4096 && p.hash_offset % 4096 == 0);
    // levels: the smallest L with (blocks - 1) >> 7L == 0
    uint32_t L = 0;
    while (L < 10 && ((u128)(blocks - 1) >> (7 * L)) != 0) ++L;
    REQUIRE(p.levels == L && L <= kVerityMaxLevels);
    // level i has ceil(blocks / 128^(i+1)) hash blocks
    u128 div = 1, sum = 0;
    for (uint32_t i = 0; i < L; ++i) {
      div *= 128;
      const u128 want = ((u128)blocks + div - 1) / div;
      REQUIRE((u128)p.blocks[i] == want);
      REQUIRE(p.blocks[i] >= 1);
      sum += want;
    }
    if (L) REQUIRE(p.blocks[L - 1] == 1);
    for (uint32_t i = L; i < kVerityMaxLevels; ++i) REQUIRE(p.blocks[i] == 0 && p.first[i] == 0);
    // contiguous, top first: the top level at block 0, each lower level right
    // after the one above it, level 0 ending the tree
    if (L) {
      REQUIRE(p.first[L - 1] == 0);
      for (uint32_t i = L - 1; i > 0; --i) REQUIRE(p.first[i - 1] == p.first[i] + p.blocks[i]);
      REQUIRE(p.first[0] + p.blocks[0] == p.tree_blocks);
    }
    REQUIRE((u128)p.tree_blocks == sum);
    REQUIRE((u128)p.tree_bytes == sum * 4096);
    // the whole file (data, padding, tree) still fits 64 bits
    REQUIRE((u128)p.hash_offset + (u128)p.tree_bytes < ((u128)1 << 64));
  }
  // what is not an image
  VerityPlan p;
  const uint64_t bad[] = {0, 1, 511, 513, 4095, kVerityMaxData, kVerityMaxData + 512, ~0ull, ~0ull - 511};
  for (uint64_t b : bad) {
    REQUIRE(!verity_plan(b, &p));
    REQUIRE(p.data_blocks == 0 && p.tree_bytes == 0 && p.levels == 0);
  }
  REQUIRE(verity_plan(kVerityMaxData - 512, &p) && p.levels == 8);
  printf("ok %d\n", tc);
  return 0;
}
