// node_remode_plan.hpp — the host plan of node dict remode (node.hip,
// ngpu_node_dict_remode): a node dict switched between replicated and partitioned
// on the GPUs.  Here are the scratch layout of a part for each direction, the
// window cuts of the join, the capacities of the result's storages and the two
// verdicts over what the kernels (node_remode.hip) counted, with their refusals.
//
// Split (replicated -> partitioned): part o keeps the rows of the replica on its
// own device whose digest it owns; global id = the row's position in the replica.
// The verdict: the parts' survivors add up to the replica's m rows.
//
// Join (partitioned -> replicated): every replica gets all m rows, row g at
// position g.  The global ids are walked in windows of c ids; a part's rows ascend
// by id, so a window is one slice per part (off[t], off[t + 1] from a binary
// search).  The slices of a window must hold exactly the window's ids, so their
// row counts must add up to its width: that is checked on the host BEFORE a row is
// copied, and it is what bounds the staging window (c rows).  The scatter then sets
// one bit per id and counts what cannot be: an id past the end, an id outside its
// window, a bit found set.  The verdict: no counter, and m bits set.
//
// Scratch bytes of a part: split 12 ceil(m / 64) + 8 (tiles(m) + 1); join
// 128 c + 8 ceil(m / 64) + 8 kRemodeCtrWords + 8 (windows + 1), whatever m is.
// Checked on the CPU by tests/cpp/node_remode_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h> and <vector>.
#pragma once
#include <stdint.h>

#include <vector>

#include "dict_retire_plan.hpp"

namespace ngpu {

constexpr uint64_t kRemodeRowBytes = 64;             // one dict row in HBM (DictRec)
constexpr uint64_t kRemodeDefaultWindow = 1u << 20;  // ids per window: 2 x 64 MiB of staging

// ---- the join's windows -----------------------------------------------------------
// Ids per window: the caller's, else the default, at least 1 and no more than the m
// ids there are (m == 0: 1).
inline uint64_t remode_window_records(uint64_t requested, uint64_t m) {
  uint64_t c = requested ? requested : kRemodeDefaultWindow;
  if (m && c > m) c = m;
  if (!m) c = 1;
  return c;
}
inline uint64_t remode_windows(uint64_t m, uint64_t c) { return m / c + (m % c ? 1 : 0); }
// Window t holds the ids [cut(t), cut(t + 1)); cut(windows) == m.
inline uint64_t remode_cut(uint64_t m, uint64_t c, uint64_t t) {
  return t >= remode_windows(m, c) ? m : t * c;
}

// ---- scratch ------------------------------------------------------------------------
// Byte offsets into a part's one scratch allocation; the u64 arrays first.
struct RemodeSplitScratch {
  uint64_t words = 0;  // u64 x nw: keep words over the replica's rows
  uint64_t sums = 0;   // u64 x (tiles(m) + 1): tile sums, then s_o
  uint64_t cnt = 0;    // u32 x nw: counts -> prefixes
  uint64_t bytes = 0;
};
inline RemodeSplitScratch remode_split_scratch_layout(uint64_t m) {
  const uint64_t nw = (m + 63) / 64;
  RemodeSplitScratch s;
  s.sums = s.words + 8 * nw;
  s.cnt = s.sums + 8 * (dict_retire_scan_tiles(m) + 1);
  s.bytes = s.cnt + 4 * nw;
  return s;
}
// Where s_o lies after the scan.
inline uint64_t remode_split_total_at(const RemodeSplitScratch &s, uint64_t m) {
  return s.sums + 8 * dict_retire_scan_tiles(m);
}

// The counter block of a replica of the join (u64 words), zeroed before the first
// window and read back in one copy after the last.
enum : int {
  kRemodeBadGid = 0,   // rows whose global id is >= m (not written)
  kRemodeOutside = 1,  // rows whose id is not in the window their slice belongs to (not written)
  kRemodeDupBit = 2,   // rows that found their id's bit already set
  kRemodeSet = 3,      // set bits of the bitmap after the last window
  kRemodeCtrWords = 4
};
struct RemodeJoinScratch {
  uint64_t stage[2] = {0, 0};  // c rows of 64 B each: the other parts' slices of a window
  uint64_t bits = 0;           // u64 x ceil(m / 64): one bit per id written
  uint64_t ctr = 0;            // u64 x kRemodeCtrWords
  uint64_t off = 0;            // u64 x (windows + 1): this part's rows at every cut (as a source)
  uint64_t bytes = 0;
};
inline RemodeJoinScratch remode_join_scratch_layout(uint64_t m, uint64_t c) {
  RemodeJoinScratch s;
  s.stage[1] = s.stage[0] + kRemodeRowBytes * c;
  s.bits = s.stage[1] + kRemodeRowBytes * c;
  s.ctr = s.bits + 8 * ((m + 63) / 64);
  s.off = s.ctr + 8 * (uint64_t)kRemodeCtrWords;
  s.bytes = s.off + 8 * (remode_windows(m, c) + 1);
  return s;
}

// ---- capacities ---------------------------------------------------------------------
// A part of s rows sits on a storage of its own with ngpu_dict_retire's room, the
// node handle on placement rows with the same room for all m.
struct RemodeCaps { uint64_t rec_cap = 0, table_cap = 0; };
inline RemodeCaps remode_caps(uint64_t s) {
  RemodeCaps c;
  c.rec_cap = dict_retire_rec_cap(s);
  c.table_cap = dict_retire_table_cap(s);
  return c;
}

// ---- verdicts -----------------------------------------------------------------------
enum RemodeRefusal : int {
  kRemodeOk = 0,
  kRemodeSplitSum,    // the parts' survivors do not add up to the replica's rows
  kRemodeSliceOrder,  // part `bad`: its rows at the cuts do not ascend (ids out of order)
  kRemodeSliceSum,    // window `window`: the parts' slices do not hold exactly its ids
  kRemodePastEnd,     // replica `bad`: an id past the dict's entries
  kRemodeOutsideWin,  // replica `bad`: an id outside its window
  kRemodeHeldTwice,   // replica `bad`: an id held twice
  kRemodeMissing      // replica `bad`: a position never written
};
struct RemodeVerdict {
  RemodeRefusal refusal = kRemodeOk;
  uint32_t bad = 0;     // the part or replica the refusal names
  uint64_t window = 0;  // kRemodeSliceSum / kRemodeSliceOrder: the window
  uint64_t got = 0;     // the count that should have been `want`
  uint64_t want = 0;
  bool ok() const { return refusal == kRemodeOk; }
};
inline const char *remode_refusal(RemodeRefusal r) {
  switch (r) {
    case kRemodeOk: return "";
    case kRemodeSplitSum: return "the parts' rows do not add up to the replica's";
    case kRemodeSliceOrder: return "a part's ids do not ascend";
    case kRemodeSliceSum: return "a window's slices do not hold exactly its ids";
    case kRemodePastEnd: return "an id past the dict's entries";
    case kRemodeOutsideWin: return "an id outside its window";
    case kRemodeHeldTwice: return "an id held twice";
    case kRemodeMissing: return "a position never written";
  }
  return "";
}

// The split: s[o] rows kept by part o of a replica of m rows.
inline RemodeVerdict remode_split_verdict(uint32_t W, const uint64_t *s, uint64_t m) {
  RemodeVerdict v;
  uint64_t sum = 0;
  for (uint32_t o = 0; o < W; ++o) {
    if (s[o] > m) {  // (also keeps the sum from wrapping)
      v.refusal = kRemodeSplitSum;
      v.bad = o;
      v.got = s[o];
      v.want = m;
      return v;
    }
    sum += s[o];
  }
  if (sum != m) {
    v.refusal = kRemodeSplitSum;
    v.bad = W;
    v.got = sum;
    v.want = m;
  }
  return v;
}

// The join before any copy: off[o] = part o's windows + 1 row offsets at the cuts,
// m_o[o] its rows.  Every part's offsets must start at 0, ascend and end at or
// below m_o; the slices of window t must add up to its width, which is at most c.
// A pass means that no window stages more than c rows and no slice leaves its part.
inline RemodeVerdict remode_join_slices(uint32_t W, uint64_t m, uint64_t c,
                                        const std::vector<std::vector<uint64_t>> &off,
                                        const uint64_t *m_o) {
  RemodeVerdict v;
  const uint64_t nw = remode_windows(m, c);
  for (uint32_t o = 0; o < W; ++o) {
    bool good = off[o].size() == nw + 1 && off[o][0] == 0 && off[o][nw] <= m_o[o];
    uint64_t t = 0;
    for (; good && t < nw; ++t) good = off[o][t] <= off[o][t + 1];
    if (!good) {
      v.refusal = kRemodeSliceOrder;
      v.bad = o;
      v.window = t;
      return v;
    }
  }
  for (uint64_t t = 0; t < nw; ++t) {
    const uint64_t want = remode_cut(m, c, t + 1) - remode_cut(m, c, t);
    uint64_t got = 0;
    for (uint32_t o = 0; o < W; ++o) {
      const uint64_t n = off[o][t + 1] - off[o][t];
      got = n > want || got > want ? want + 1 : got + n;  // (saturates: no wrap)
    }
    if (got != want) {
      v.refusal = kRemodeSliceSum;
      v.window = t;
      v.got = got;
      v.want = want;
      return v;
    }
  }
  return v;
}

// The join after the last window: ctr = W x kRemodeCtrWords words, replica j's
// block at j * kRemodeCtrWords.
inline RemodeVerdict remode_join_verdict(uint32_t W, const uint64_t *ctr, uint64_t m) {
  RemodeVerdict v;
  for (uint32_t j = 0; j < W; ++j) {
    const uint64_t *c = ctr + (uint64_t)j * kRemodeCtrWords;
    const RemodeRefusal r = c[kRemodeBadGid]    ? kRemodePastEnd
                            : c[kRemodeOutside] ? kRemodeOutsideWin
                            : c[kRemodeDupBit]  ? kRemodeHeldTwice
                            : c[kRemodeSet] != m ? kRemodeMissing
                                                 : kRemodeOk;
    if (r != kRemodeOk) {
      v.refusal = r;
      v.bad = j;
      v.got = r == kRemodeMissing ? c[kRemodeSet]
              : c[r == kRemodePastEnd ? kRemodeBadGid : r == kRemodeOutsideWin ? kRemodeOutside : kRemodeDupBit];
      v.want = r == kRemodeMissing ? m : 0;
      return v;
    }
  }
  return v;
}

}  // namespace ngpu
