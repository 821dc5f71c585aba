// dict_retire_plan.hpp — the bookkeeping of dict retire (dict.hip,
// ngpu_dict_retire): which inner blobs leave, what index each kept blob gets,
// and how large the storage of the result is.  The kernels (dict_retire.hip)
// read the two tables built here: one retire bit per blob and one new index
// per blob.  Also the host half of the compaction: the placement rows moved by
// the keep words and prefixes the kernels computed.  Checked on the CPU by tests/cpp/dict_retire_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h> and <vector>.
#pragma once
#include <stdint.h>

#include <vector>

#include "dict_grow_plan.hpp"

namespace ngpu {

constexpr uint32_t kDictMaxBlobs = 1u << 20;        // as ngpu_dict_create
constexpr uint32_t kRetiredBlob = 0xFFFFFFFFu;      // remap[] of a blob that leaves

struct DictRetirePlan {
  bool ok = false;      // false: `bad` is not a blob of the base (or it has too many blobs)
  uint32_t bad = 0;     // the first index >= n_blobs in the list
  uint32_t n_kept = 0;  // blobs of the result
  // bit b of bitmap[b / 32]: blob b leaves; (n_blobs + 31) / 32 words, at least one
  std::vector<uint32_t> bitmap;
  // remap[b]: the rank of blob b among the kept ones, kRetiredBlob when it leaves
  std::vector<uint32_t> remap;
};

// blobs[0, n): inner blob indices of a dict of n_blobs blobs, in any order,
// duplicates allowed.
inline DictRetirePlan dict_retire_plan(uint32_t n_blobs, const uint32_t *blobs, uint32_t n) {
  DictRetirePlan p;
  if (n_blobs > kDictMaxBlobs) {
    p.bad = n_blobs;
    return p;
  }
  for (uint32_t i = 0; i < n; ++i)
    if (blobs[i] >= n_blobs) {
      p.bad = blobs[i];
      return p;
    }
  p.ok = true;
  p.bitmap.assign(n_blobs ? (n_blobs + 31) / 32 : 1, 0);
  for (uint32_t i = 0; i < n; ++i) p.bitmap[blobs[i] >> 5] |= 1u << (blobs[i] & 31);
  p.remap.resize(n_blobs);
  for (uint32_t b = 0; b < n_blobs; ++b)
    p.remap[b] = (p.bitmap[b >> 5] >> (b & 31)) & 1 ? kRetiredBlob : p.n_kept++;
  return p;
}

// The storage of a retire's result with s survivors: what a fork of an extend
// with k = 0 would allocate (dict_grow_plan), s + s / 2 record slots and the
// table dict_alloc gives for that many, so that the next extends of up to s / 2
// records in all append in place.
inline uint64_t dict_retire_rec_cap(uint64_t s) {
  uint64_t want = s + s / 2;
  if (want > kDictMaxEntries - 1) want = kDictMaxEntries - 1;  // no slot past the last valid id
  return want;
}
inline uint64_t dict_retire_table_cap(uint64_t s) { return dict_table_cap(dict_retire_rec_cap(s)); }

// The host side of the compaction (the placement rows): the rows of src[0, m)
// whose keep bit is set, for keep words [w_lo, w_hi), to dst[prefix[w] + rank in
// word w], as the device kernel places the records.  words / prefix: what the
// device computed, (m + 63) / 64 of each; bits at or past m are ignored, no row
// at or past s is written.  Disjoint word ranges write disjoint rows, so
// several threads may each take a range.
template <class Row>
inline void dict_retire_compact_rows(const uint64_t *words, const uint32_t *prefix, uint64_t w_lo,
                                     uint64_t w_hi, uint64_t m, const Row *src, Row *dst,
                                     uint64_t s) {
  for (uint64_t w = w_lo; w < w_hi && w * 64 < m; ++w) {
    const uint64_t i0 = w * 64, n = m - i0 < 64 ? m - i0 : 64;
    uint64_t x = words[w], j = prefix[w];
    if (n < 64) x &= (1ull << n) - 1;
    if (x == ~0ull && j + 64 <= s) {  // a whole word of survivors: one copy
      for (int b = 0; b < 64; ++b) dst[j + b] = src[i0 + b];
      continue;
    }
    for (; x; x &= x - 1, ++j)
      if (j < s) dst[j] = src[i0 + (uint64_t)__builtin_ctzll(x)];
  }
}
constexpr uint64_t kRetireHostPiece = 4096;  // keep words per host work item: 262,144 rows

// ---- device scratch ---------------------------------------------------------------
// One scan tile (dict_retire.hip) is kRetireScanTile keep words: 16,384 records.
constexpr uint64_t kRetireScanTile = 256;
inline uint64_t dict_retire_scan_tiles(uint64_t m) {
  return ((m + 63) / 64 + kRetireScanTile - 1) / kRetireScanTile;
}

// A retire's one scratch allocation, byte offsets: keep words (u64 per 64
// records, at 0), tile sums + the total (u64), word counts / prefixes (u32), the
// retire bitmap and the blob remap (u32 each).
struct RetireScratch { uint64_t words = 0, sums = 0, cnt = 0, bits = 0, remap = 0, bytes = 0; };
inline RetireScratch retire_scratch_layout(uint64_t m, uint64_t bitmap_words, uint64_t remap_words) {
  const uint64_t nw = (m + 63) / 64;
  RetireScratch s;
  s.sums = 8 * nw;
  s.cnt = s.sums + 8 * (dict_retire_scan_tiles(m) + 1);
  s.bits = s.cnt + 4 * nw;
  s.remap = s.bits + 4 * bitmap_words;
  s.bytes = s.remap + 4 * remap_words;
  return s;
}

}  // namespace ngpu
