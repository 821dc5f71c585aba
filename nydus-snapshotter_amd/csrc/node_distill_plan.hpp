// node_distill_plan.hpp — the host plan of distilling a partitioned node dict
// (node.hip, ngpu_node_dict_distill_parts): the layout of a part's one scratch
// allocation, and the step from what the W parts' kernels (node_distill.hip)
// counted to the info and the live blobs of the whole dict.
//
// All rows of a digest live on one part, so a part counts its own rows
// (dict_distill.hip) and the whole dict's counters are sums (max_refs: the
// maximum) over the parts.  The survivors' global ranks need every part's keep
// bits (node_retire_plan.hpp), and a blob is live when ANY part holds a survivor
// in it: the OR of the parts' live bitmaps goes through distill_blob_plan
// (dict_distill_plan.hpp), which knows the three blob rules.
//
// A part's scratch is a retire's (NodeRetireScratch; the retire bitmap has no
// words here, the remap one word per blob) plus one u32 of refs per row, the
// distill counters right after the retire counters (one copy brings the
// kNodeDistillBackWords of them back) and the live words.
// Checked on the CPU by tests/cpp/node_distill_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h> and <vector>.
#pragma once
#include <stdint.h>

#include <vector>

#include "dict_distill_plan.hpp"
#include "node_retire_plan.hpp"

namespace ngpu {

// The counters one copy brings back from a part: the retire block, then the
// distill block.
constexpr int kNodeDistillBackWords = kNodeRetireCtrWords + kDistillStatWords;

// Byte offsets into a part's scratch; the u64 arrays first, then the u32 ones.
// r holds a retire's arrays (r.bits: no words; r.bytes: the whole allocation's).
// Zeroed before the launches: r.own, [r.ctr, r.ctr + 8 kNodeDistillBackWords)
// and [live, live + zero_bytes) -- the live words and refs, which follow them.
struct NodeDistillScratch {
  NodeRetireScratch r;
  uint64_t stats = 0;  // u64 x kDistillStatWords, right after r.ctr's words
  uint64_t live = 0;   // u32 x distill_live_words(n_blobs)
  uint64_t refs = 0;   // u32 x m_o, right after the live words
  uint64_t zero_bytes = 0;
  uint64_t bytes = 0;
};
inline NodeDistillScratch node_distill_scratch_layout(uint64_t m_o, uint64_t m, uint32_t W,
                                                      uint32_t n_blobs) {
  const uint64_t nw = (m_o + 63) / 64, gnw = (m + 63) / 64, lw = distill_live_words(n_blobs);
  NodeDistillScratch s;
  NodeRetireScratch &r = s.r;
  r.sums = r.words + 8 * nw;
  r.own = r.sums + 8 * (dict_retire_scan_tiles(m_o) + 1);
  r.gather = r.own + 8 * gnw;
  r.gwords = r.gather + 8 * (uint64_t)W * gnw;
  r.gsums = r.gwords + 8 * gnw;
  r.ctr = r.gsums + 8 * (dict_retire_scan_tiles(m) + 1);
  s.stats = r.ctr + 8 * (uint64_t)kNodeRetireCtrWords;
  r.cnt = s.stats + 8 * (uint64_t)kDistillStatWords;
  r.gcnt = r.cnt + 4 * nw;
  r.bits = r.gcnt + 4 * gnw;
  r.remap = r.bits;
  s.live = r.remap + 4 * (uint64_t)n_blobs;
  s.refs = s.live + 4 * lw;
  s.zero_bytes = 4 * lw + 4 * m_o;
  s.bytes = s.refs + 4 * m_o;
  r.bytes = s.bytes;
  return s;
}

// What the parts counted, on the whole dict.  back: W x kNodeDistillBackWords
// words, part o's block at o * kNodeDistillBackWords (the retire counters, then
// the distill counters); live: W x lw words, part o's bitmap at o * lw, lw =
// distill_live_words(n_blobs); m_o: the parts' row counts, s_o: their survivors
// as the scan counted them (the verdict's).  bad_part: the first part whose
// counters cannot be those of m_o rows with s_o survivors (W: none).
struct NodeDistillSum {
  uint32_t bad_part = 0;
  uint64_t stats[kDistillStatWords] = {};
  std::vector<uint32_t> live;  // lw words: the OR of the parts'
  bool ok(uint32_t W) const { return bad_part == W; }
};
inline NodeDistillSum node_distill_sum(uint32_t W, const uint64_t *back, const uint32_t *live,
                                       uint32_t n_blobs, const uint64_t *m_o, const uint64_t *s_o) {
  const uint64_t lw = distill_live_words(n_blobs);
  NodeDistillSum x;
  x.bad_part = W;
  x.live.assign(lw, 0);
  for (uint32_t o = 0; o < W; ++o) {
    const uint64_t *st = back + (uint64_t)o * kNodeDistillBackWords + kNodeRetireCtrWords;
    if (!distill_stats_sane(st, m_o[o], s_o[o])) {
      if (x.ok(W)) x.bad_part = o;
      continue;
    }
    for (int k = 0; k < kDistillStatWords; ++k) {
      if (k == kDistillMaxRefs)
        x.stats[k] = st[k] > x.stats[k] ? st[k] : x.stats[k];
      else
        x.stats[k] += st[k];
    }
    for (uint64_t j = 0; j < lw; ++j) x.live[j] |= live[(uint64_t)o * lw + j];
  }
  return x;
}

}  // namespace ngpu
