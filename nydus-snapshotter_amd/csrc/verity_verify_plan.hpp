// verity_verify_plan.hpp — where a stored hash block of a dm-verity tree sits
// and what it answers for (verity.hip, "Verify"): tree block -> level, index
// in the level, the tree offset of the digest slot that holds its hash, how
// many of its 128 slots hold digests, and the data blocks it covers.  The
// verify kernel and the host's findings list both go through verity_locate, so
// they cannot disagree.  Checked on the CPU by
// tests/cpp/verity_verify_plan_test.cpp (no GPU).
// Header-only, host and device; needs verity_plan.hpp.
#pragma once
#include "verity_plan.hpp"

#if defined(__HIPCC__)
#define NGPU_VERITY_HD __host__ __device__ __forceinline__
#else
#define NGPU_VERITY_HD inline
#endif

namespace ngpu {

// The plan as a kernel takes it by value.  below[l]: digests level l holds
// (the data blocks for level 0, the hash blocks of level l - 1 above it).
struct VerityGeom {
  uint64_t tree_blocks;
  uint64_t data_blocks;
  uint32_t levels;
  uint32_t reserved;
  uint64_t first[kVerityMaxLevels];
  uint64_t blocks[kVerityMaxLevels];
  uint64_t below[kVerityMaxLevels];
};

inline VerityGeom verity_geom(const VerityPlan &p) {
  VerityGeom g{};
  g.tree_blocks = p.tree_blocks;
  g.data_blocks = p.data_blocks;
  g.levels = p.levels;
  for (uint32_t l = 0; l < p.levels; ++l) {
    g.first[l] = p.first[l];
    g.blocks[l] = p.blocks[l];
    g.below[l] = l ? p.blocks[l - 1] : p.data_blocks;
  }
  return g;
}

constexpr uint64_t kVerityNoParent = ~0ull;  // the top block: its hash is the root

struct VerityBlockLoc {
  uint32_t level;       // 0 = the level above the data
  uint32_t used;        // digest slots of the block that hold a digest, 1..128
  uint64_t index;       // block `index` of its level
  uint64_t parent_off;  // tree byte offset of the 32 bytes that hold its hash
  uint64_t first_data;  // the data blocks whose digests it answers for,
  uint64_t last_data;   // inclusive
  bool last_of_level;   // only such a block can have a spare area
};

// t < g.tree_blocks.  Every array index is a constant once the loop is
// unrolled, so a kernel reads the by-value struct with scalar loads only.
NGPU_VERITY_HD VerityBlockLoc verity_locate(const VerityGeom &g, uint64_t t) {
  uint32_t l = 0;
  uint64_t first = 0, nblk = 0, below = 0, up = 0;
  bool top = true;
  // the levels lie top first: the level of t is the lowest one that starts at
  // or before t
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = (int)kVerityMaxLevels - 1; i >= 0; --i) {
    if ((uint32_t)i < g.levels && t >= g.first[i]) {
      l = (uint32_t)i;
      first = g.first[i];
      nblk = g.blocks[i];
      below = g.below[i];
      top = (uint32_t)(i + 1) == g.levels;
      up = g.first[i + 1 < (int)kVerityMaxLevels ? i + 1 : i];  // not used for the top level
    }
  }
  VerityBlockLoc r;
  r.level = l;
  r.index = t - first;
  r.last_of_level = r.index + 1 == nblk;
  r.used = r.last_of_level ? (uint32_t)(below - kVerityFanout * r.index) : (uint32_t)kVerityFanout;
  r.parent_off = top ? kVerityNoParent : up * kVerityHashBlock + kVerityDigest * r.index;
  // 128^(l+1) <= 2^56 and index * span < data_blocks + span < 2^57: no wrap
  const uint32_t sh = kVerityFanoutLog2 * (l + 1);
  r.first_data = r.index << sh;
  const uint64_t end = (r.index + 1) << sh;
  r.last_data = (end < g.data_blocks ? end : g.data_blocks) - 1;
  return r;
}

}  // namespace ngpu
