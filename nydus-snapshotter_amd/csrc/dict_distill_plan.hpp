// dict_distill_plan.hpp — the host half of dict distill (dict.hip,
// ngpu_dict_distill): the layout of its one scratch allocation, the step from
// the blob-live bitmap the kernels (dict_distill.hip) bring back to the blob
// remap the compaction reads, under the two flags, and the assembly of
// ngpu_dict_distill_info from the device's counters.  Checked on the CPU by
// tests/cpp/dict_distill_plan_test.cpp (no GPU).
// Header-only, host-only but for distill_bucket, which the stats kernel calls too.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "dict_hash.hpp"
#include "dict_retire_plan.hpp"
#include "nydus_gpu.h"

namespace ngpu {

// The counters of distill_keep_words, u64 each: rows that win their digest,
// winners held by fewer than min_refs rows, the largest count, and the winners
// by floor(log2(refs)).
constexpr int kDistillDistinct = 0, kDistillBelowMin = 1, kDistillMaxRefs = 2, kDistillHist = 3;
constexpr int kDistillStatWords = kDistillHist + 32;

// refs >= 1 -> the bucket b with 2^b <= refs < 2^(b + 1).
NGPU_HD uint32_t distill_bucket(uint32_t refs) { return 31u - (uint32_t)__builtin_clz(refs | 1u); }

// The 256-row tiles a workgroup of the distill kernels runs over: at least 4, and
// as many as it takes for kDistillGrid workgroups to cover the dict.
constexpr uint64_t kDistillGrid = 2048;
inline uint64_t distill_tiles_per_wg(uint64_t m) {
  const uint64_t per = ((m + 255) / 256 + kDistillGrid - 1) / kDistillGrid;
  return per < 4 ? 4 : per;
}

inline uint64_t distill_live_words(uint32_t n_blobs) { return n_blobs ? (n_blobs + 31) / 32 : 1; }

// A distill's one scratch allocation, byte offsets.  words / sums / cnt are the
// arrays of a retire (dict_retire_plan.hpp).  What the one mid-way copy brings
// back is contiguous from `back`: the scan's total (the last word of sums), the
// counters, the blob-live bitmap (one bit per blob of the base, u32 words).
// refs: one u32 per row.  stats, live and refs are zeroed before the launches.
struct DistillScratch {
  uint64_t words = 0, sums = 0, back = 0, stats = 0, live = 0, cnt = 0, remap = 0, refs = 0, bytes = 0;
  uint64_t back_bytes = 0;
};
inline DistillScratch distill_scratch_layout(uint64_t m, uint32_t n_blobs) {
  const uint64_t nw = (m + 63) / 64, lw = distill_live_words(n_blobs);
  DistillScratch s;
  s.sums = 8 * nw;
  s.back = s.sums + 8 * dict_retire_scan_tiles(m);
  s.stats = s.back + 8;
  s.live = s.stats + 8 * kDistillStatWords;
  s.back_bytes = s.live + 4 * lw - s.back;
  s.cnt = s.live + 4 * lw;
  s.remap = s.cnt + 4 * nw;
  s.refs = s.remap + 4 * (uint64_t)n_blobs;
  s.bytes = s.refs + 4 * m;
  return s;
}

// What becomes of the blobs.  remap[b]: the index rows of blob b get in the
// result (what the compaction reads; kRetiredBlob: no surviving row points at
// it).  rows[b]: kRetiredBlob when blob b's row leaves the blob table, else its
// new position (what dict_retire_blob_table reads).  The two differ only under
// NGPU_DICT_DISTILL_MERGE_BLOB_IDS, where a later blob of an id keeps a remap
// (the first blob's) and loses its row.
struct DistillBlobPlan {
  bool ok = false;  // false: more than kDictMaxBlobs blobs
  uint32_t n_kept = 0;
  std::vector<uint32_t> remap, rows;
};

// live: distill_live_words(n_blobs) words, bit b: a surviving row points at blob
// b.  table: the base's 256-B blob rows, n_blobs of them (read only under
// MERGE_BLOB_IDS; null there: nothing is merged).
inline DistillBlobPlan distill_blob_plan(uint32_t n_blobs, const uint32_t *live, uint32_t flags,
                                         const uint8_t *table) {
  DistillBlobPlan p;
  if (n_blobs > kDictMaxBlobs) return p;
  p.ok = true;
  if (flags & NGPU_DICT_DISTILL_KEEP_BLOBS) {
    p.n_kept = n_blobs;
    p.remap.resize(n_blobs);
    for (uint32_t b = 0; b < n_blobs; ++b) p.remap[b] = b;
    p.rows = p.remap;
    return p;
  }
  // rep[b]: the earliest blob with b's 64 id bytes (b itself without the flag)
  std::vector<uint32_t> rep(n_blobs);
  for (uint32_t b = 0; b < n_blobs; ++b) rep[b] = b;
  if ((flags & NGPU_DICT_DISTILL_MERGE_BLOB_IDS) && table) {
    std::unordered_map<std::string, uint32_t> first;
    first.reserve(n_blobs);
    for (uint32_t b = 0; b < n_blobs; ++b)
      rep[b] = first.emplace(std::string((const char *)table + 256ull * b, 64), b).first->second;
  }
  std::vector<uint8_t> alive(n_blobs, 0);
  for (uint32_t b = 0; b < n_blobs; ++b)
    if ((live[b >> 5] >> (b & 31)) & 1) alive[rep[b]] = 1;
  std::vector<uint32_t> leaving;
  for (uint32_t b = 0; b < n_blobs; ++b)
    if (rep[b] != b || !alive[b]) leaving.push_back(b);
  const DictRetirePlan r = dict_retire_plan(n_blobs, leaving.data(), (uint32_t)leaving.size());
  p.n_kept = r.n_kept;
  p.rows = r.remap;
  p.remap.resize(n_blobs);
  for (uint32_t b = 0; b < n_blobs; ++b) p.remap[b] = r.remap[rep[b]];
  return p;
}

// The counters as the device left them, against what must hold of them for a
// dict of m rows whose scan counted s survivors.
inline bool distill_stats_sane(const uint64_t *st, uint64_t m, uint64_t s) {
  uint64_t h = 0;
  for (int b = 0; b < 32; ++b) h += st[kDistillHist + b];
  return st[kDistillDistinct] <= m && st[kDistillBelowMin] <= st[kDistillDistinct] &&
         s == st[kDistillDistinct] - st[kDistillBelowMin] && h == st[kDistillDistinct] &&
         st[kDistillMaxRefs] <= m && (st[kDistillMaxRefs] != 0) == (st[kDistillDistinct] != 0);
}

inline void distill_info_fill(ngpu_dict_distill_info *info, uint64_t m, const uint64_t *st,
                              uint32_t blobs_in, uint32_t blobs_out) {
  memset(info, 0, sizeof *info);
  info->entries_in = m;
  info->distinct = st[kDistillDistinct];
  info->shadowed = m - st[kDistillDistinct];
  info->below_min = st[kDistillBelowMin];
  info->entries_out = st[kDistillDistinct] - st[kDistillBelowMin];
  info->blobs_in = blobs_in;
  info->blobs_out = blobs_out;
  info->max_refs = (uint32_t)st[kDistillMaxRefs];
  for (int b = 0; b < 32; ++b) info->refs_hist[b] = st[kDistillHist + b];
}

}  // namespace ngpu
