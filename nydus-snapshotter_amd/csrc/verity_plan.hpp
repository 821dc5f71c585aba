// verity_plan.hpp — the geometry of a dm-verity hash tree (verity.hip,
// ngpu_verity_layout): format 1, no superblock, 512-byte data blocks,
// 4096-byte hash blocks of up to 128 SHA-256 digests, the layout
// `veritysetup format --no-superblock --data-block-size=512
// --hash-block-size=4096` writes and the kernel's dm-verity reads.  Checked on
// the CPU by tests/cpp/verity_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h>.
#pragma once
#include <stdint.h>

namespace ngpu {

constexpr uint64_t kVerityDataBlock = 512;
constexpr uint64_t kVerityHashBlock = 4096;
constexpr uint32_t kVerityDigest = 32;
constexpr uint32_t kVerityFanoutLog2 = 7;  // 4096 / 32 digests per hash block
constexpr uint64_t kVerityFanout = 1ull << kVerityFanoutLog2;
constexpr uint64_t kVerityMaxData = 1ull << 62;  // data_bytes below this: nothing overflows
// (2^62 / 512 - 1) >> (7 * 8) == 0: at most 8 levels
constexpr uint32_t kVerityMaxLevels = 8;

// Level i (0 = the one above the data) has blocks[i] hash blocks, the first of
// which is hash block first[i] of the tree: the top level comes first, level 0
// last.  levels == 0: one data block, no tree (its digest is the root).
struct VerityPlan {
  uint64_t data_blocks = 0;
  uint64_t hash_offset = 0;  // data_bytes rounded up to a hash block
  uint64_t tree_blocks = 0;  // hash blocks of all levels
  uint64_t tree_bytes = 0;   // 4096 * tree_blocks
  uint32_t levels = 0;
  uint64_t blocks[kVerityMaxLevels] = {};
  uint64_t first[kVerityMaxLevels] = {};
};

// false: data_bytes is 0, not a multiple of 512, or 2^62 and above (*p is
// left zero).
inline bool verity_plan(uint64_t data_bytes, VerityPlan *p) {
  *p = VerityPlan{};
  if (data_bytes == 0 || data_bytes % kVerityDataBlock || data_bytes >= kVerityMaxData) return false;
  p->data_blocks = data_bytes / kVerityDataBlock;
  // < 2^62 + 4096: no wrap
  p->hash_offset = (data_bytes + kVerityHashBlock - 1) / kVerityHashBlock * kVerityHashBlock;
  uint32_t L = 0;
  while (L < kVerityMaxLevels && ((p->data_blocks - 1) >> (kVerityFanoutLog2 * L)) != 0) ++L;
  if (((p->data_blocks - 1) >> (kVerityFanoutLog2 * L)) != 0) {  // unreachable below 2^62
    *p = VerityPlan{};
    return false;
  }
  p->levels = L;
  uint64_t below = p->data_blocks, total = 0;
  for (uint32_t i = 0; i < L; ++i) {
    // ceil(below / 128) without the + 127 that could wrap
    p->blocks[i] = below / kVerityFanout + (below % kVerityFanout != 0);
    total += p->blocks[i];  // a geometric series below data_blocks / 64: no wrap
    below = p->blocks[i];
  }
  uint64_t at = 0;
  for (uint32_t i = L; i-- > 0;) {
    p->first[i] = at;
    at += p->blocks[i];
  }
  p->tree_blocks = total;
  p->tree_bytes = total * kVerityHashBlock;  // < 2^53 / 64 * 2^12: no wrap
  return true;
}

}  // namespace ngpu
