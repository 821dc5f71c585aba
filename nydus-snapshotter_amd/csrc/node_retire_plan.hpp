// node_retire_plan.hpp — the host plan of retiring a partitioned node dict
// (node.hip, ngpu_node_dict_retire_parts): the layout of a part's one scratch
// allocation, the verdict over what the parts' kernels (node_retire.hip) counted,
// and the capacities of the result's storages.
//
// The parts of a partitioned dict tile its global ids [0, m): part o keeps m_o
// rows, each with its global id.  A part's new global ids are ranks over ALL
// parts' keep bits, so every part builds a keep bitmap over [0, m) of its own
// rows, gathers the other parts' bitmaps, ORs them and scans the popcounts: the
// same global prefix on every part, with no lead device and no second exchange.
//
// Scratch bytes of a part with m_o rows of a dict of m entries on W parts, for
// nw = ceil(m_o / 64) and gnw = ceil(m / 64):
//   8 (W + 2) gnw + 4 gnw      own bitmap, W gathered bitmaps, their OR; its counts
//   + 8 nw + 4 nw              local keep words; their counts
//   + 8 (tiles(m_o) + tiles(m) + 2 + kNodeRetireCtrWords) + 4 (bitmap + remap words)
// i.e. about (W + 2.5) m / 8 + 0.19 m_o bytes: 263 MB at m = 200M and W = 8,
// next to the part's 1.6 GB of records.
// Checked on the CPU by tests/cpp/node_retire_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h> and <vector>.
#pragma once
#include <stdint.h>

#include <vector>

#include "dict_retire_plan.hpp"

namespace ngpu {

// The counter block of a part (u64 words), zeroed before the keep pass and read
// back in one copy after the global scan.
enum : int {
  kNodeRetireBadGid = 0,   // kept rows whose global id is >= m (their bit is not written)
  kNodeRetireDupBit = 1,   // atomic ORs that found one of their bits already set
  kNodeRetireOverlap = 2,  // global words whose W popcounts do not add up to the OR's
  kNodeRetireLocal = 3,    // s_o: the part's own survivors
  kNodeRetireGlobal = 4,   // S: the survivors of all parts
  kNodeRetireCtrWords = 5
};

// Byte offsets into a part's scratch; the u64 arrays first, then the u32 ones.
struct NodeRetireScratch {
  uint64_t words = 0;   // u64 x nw: local keep words
  uint64_t sums = 0;    // u64 x (tiles(m_o) + 1): local tile sums + s_o
  uint64_t own = 0;     // u64 x gnw: this part's bitmap over the global ids
  uint64_t gather = 0;  // u64 x W x gnw: every part's bitmap, part p's at p * gnw
  uint64_t gwords = 0;  // u64 x gnw: their OR, the global keep words
  uint64_t gsums = 0;   // u64 x (tiles(m) + 1): global tile sums + S
  uint64_t ctr = 0;     // u64 x kNodeRetireCtrWords
  uint64_t cnt = 0;     // u32 x nw: local counts -> prefixes
  uint64_t gcnt = 0;    // u32 x gnw: global counts -> prefixes
  uint64_t bits = 0;    // u32 x bitmap_words: the retire bitmap (one bit per blob)
  uint64_t remap = 0;   // u32 x remap_words: the blob remap
  uint64_t bytes = 0;
};
inline NodeRetireScratch node_retire_scratch_layout(uint64_t m_o, uint64_t m, uint32_t W,
                                                    uint64_t bitmap_words, uint64_t remap_words) {
  const uint64_t nw = (m_o + 63) / 64, gnw = (m + 63) / 64;
  NodeRetireScratch s;
  s.sums = s.words + 8 * nw;
  s.own = s.sums + 8 * (dict_retire_scan_tiles(m_o) + 1);
  s.gather = s.own + 8 * gnw;
  s.gwords = s.gather + 8 * (uint64_t)W * gnw;
  s.gsums = s.gwords + 8 * gnw;
  s.ctr = s.gsums + 8 * (dict_retire_scan_tiles(m) + 1);
  s.cnt = s.ctr + 8 * (uint64_t)kNodeRetireCtrWords;
  s.gcnt = s.cnt + 4 * nw;
  s.bits = s.gcnt + 4 * gnw;
  s.remap = s.bits + 4 * bitmap_words;
  s.bytes = s.remap + 4 * remap_words;
  return s;
}

// ---- the verdict ----------------------------------------------------------------
// ctr: W x kNodeRetireCtrWords words, part o's block at o * kNodeRetireCtrWords.
// The parts tile the dict's ids when no part saw an id >= m or a bit set twice,
// no global word was set by two parts, every part computed the same S <= m, and
// the parts' own survivors add up to it (a global id held twice, in one part or
// in two, makes the sum larger than the number of distinct bits).
enum NodeRetireRefusal : int {
  kNodeRetireOk = 0,
  kNodeRetireCounter = 1,  // part `bad`: counter `which` is not zero
  kNodeRetireSum = 2,      // sum of s_o != S (bad: the first part whose S differs, W: none does)
  kNodeRetireTooMany = 3   // S > m
};
struct NodeRetireVerdict {
  NodeRetireRefusal refusal = kNodeRetireOk;
  uint32_t bad = 0;
  int which = 0;
  uint64_t S = 0;             // survivors of all parts
  std::vector<uint64_t> s;    // per part
  bool ok() const { return refusal == kNodeRetireOk; }
};
inline NodeRetireVerdict node_retire_verdict(uint32_t W, const uint64_t *ctr, uint64_t m) {
  NodeRetireVerdict v;
  v.s.assign(W, 0);
  uint64_t sum = 0;
  for (uint32_t o = 0; o < W; ++o) {
    const uint64_t *c = ctr + (uint64_t)o * kNodeRetireCtrWords;
    for (int k = kNodeRetireBadGid; k <= kNodeRetireOverlap; ++k)
      if (c[k] && v.ok()) {
        v.refusal = kNodeRetireCounter;
        v.bad = o;
        v.which = k;
      }
    v.s[o] = c[kNodeRetireLocal];
    sum += v.s[o];
  }
  v.S = W ? ctr[kNodeRetireGlobal] : 0;
  if (!v.ok()) return v;
  for (uint32_t o = 0; o < W; ++o)
    if (ctr[(uint64_t)o * kNodeRetireCtrWords + kNodeRetireGlobal] != v.S) {
      v.refusal = kNodeRetireSum;
      v.bad = o;
      return v;
    }
  if (sum != v.S) {
    v.refusal = kNodeRetireSum;
    v.bad = W;
    return v;
  }
  if (v.S > m) v.refusal = kNodeRetireTooMany;
  return v;
}

// ---- capacities -----------------------------------------------------------------
// Every part of the result sits on a storage of its own with a fork's room for
// its s_o survivors, the node handle on placement rows for S (dict_retire_plan.hpp).
struct NodeRetireCaps {
  std::vector<uint64_t> rec_cap, table_cap;  // per part
  uint64_t place_cap = 0;                    // the node handle's rows
};
inline NodeRetireCaps node_retire_caps(const NodeRetireVerdict &v) {
  NodeRetireCaps c;
  for (uint64_t s : v.s) {
    c.rec_cap.push_back(dict_retire_rec_cap(s));
    c.table_cap.push_back(dict_retire_table_cap(s));
  }
  c.place_cap = dict_retire_rec_cap(v.S);
  return c;
}

// ---- what the compaction computes -------------------------------------------------
// The new global id of old id g < m: the rank of its keep bit among all set bits.
inline uint64_t node_retire_new_gid(const uint64_t *gwords, const uint32_t *gprefix, uint64_t g) {
  return (uint64_t)gprefix[g >> 6] +
         (uint64_t)__builtin_popcountll(gwords[g >> 6] & ((1ull << (g & 63)) - 1));
}

}  // namespace ngpu
