// dict_fold_plan.hpp — the bookkeeping of dict fold (dict.hip, ngpu_dict_fold
// and ngpu_dict_extend_device): which blob table and which placement rows the
// result keeps (or why the call is refused), and a CPU restatement of what the
// kernels (dict_fold.hip) compute from the kinds and the layer cuts: keep words,
// their prefixes, every NEW chunk's record position and every layer's blob rank.
// Checked on the CPU by tests/cpp/dict_fold_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h> and <vector>.
#pragma once
#include <stdint.h>

#include <vector>

#include "dict_retire_plan.hpp"  // the scan tiles of the keep words

namespace ngpu {

// ---- blob table: extend's rule --------------------------------------------------
// The result has a table iff both sides have one; when neither does it has only a
// blob count; exactly one side with a table is refused.  A base of 0 blobs goes
// with either, and so does a call that adds nothing (k == 0 and n_blobs == 0),
// which keeps what the base has.
enum DictTableRule : int {
  kTableNone = 0,      // ok: a blob count only
  kTableKept = 1,      // ok: base's rows ++ the call's
  kTableBaseOnly = -1, // refused: the base has a table, the new records come without one
  kTableCallOnly = -2  // refused: the base has none, the new records come with one
};
inline DictTableRule dict_table_rule(uint32_t base_blobs, bool base_has, bool call_has, uint64_t k,
                                     uint32_t n_blobs) {
  if (base_blobs == 0 && !base_has) return call_has ? kTableKept : kTableNone;
  if (k == 0 && n_blobs == 0) return base_has ? kTableKept : kTableNone;
  if (base_has != call_has) return base_has ? kTableBaseOnly : kTableCallOnly;
  return base_has ? kTableKept : kTableNone;
}

// ---- placements of a fold -------------------------------------------------------
// base_m: the base's entries; base_keeps: it keeps compressed placements; given:
// the call passes rows, n_placements of them; k: NEW chunks counted on the device.
enum DictFoldPlace : int {
  kPlaceNone = 0,        // ok: the result keeps no placements
  kPlaceKept = 1,        // ok: base's rows (if any) ++ the call's
  kPlaceBase = 2,        // ok: nothing is added, the result is the base
  kPlaceCount = -1,      // refused: n_placements != k
  kPlaceMissing = -2,    // refused: the base keeps placements, k > 0 and none are given
  kPlaceUnwanted = -3    // refused: the base has records and keeps none, some are given
};
inline DictFoldPlace dict_fold_place_rule(uint64_t base_m, bool base_keeps, bool given,
                                          uint64_t n_placements, uint64_t k) {
  if (given && n_placements != k) return kPlaceCount;
  if (k == 0) return kPlaceBase;
  if (base_keeps && !given) return kPlaceMissing;
  if (base_m && !base_keeps && given) return kPlaceUnwanted;
  return given ? kPlaceKept : kPlaceNone;
}

// ---- device scratch and counters ------------------------------------------------
// ctr: kFoldCtrWords u64 the kernels (dict_fold.hip) fill, zeroed on the fold's
// stream by the caller before launch_fold_keep_scan.
constexpr int kFoldK = 0;         // NEW chunks of the call
constexpr int kFoldBlobs = 1;     // layers with a NEW chunk
constexpr int kFoldBadKind = 2;   // chunks whose kind is none of NEW / INTRA / DICT
constexpr int kFoldBadKind1 = 3;  // ~(the smallest such chunk id) (atomic max), 0 = none
constexpr int kFoldBadLen = 4;    // NEW chunks of length 0 or > chunk_size
constexpr int kFoldBadLen1 = 5;   // ~(the smallest such chunk id), 0 = none
constexpr int kFoldBadLayer1 = 6; // ~(the smallest layer whose bounds are out of order), 0 = none
constexpr int kFoldCtrWords = 8;

// A fold's scratch, byte offsets: keep words (u64 per 64 chunks, at 0), tile sums
// + the total (u64), ctr_bytes of counters (u64; a node fold's are followed by
// its owner counts), word counts / prefixes (u32), L layer ranks (u32).
struct FoldScratch { uint64_t words = 0, sums = 0, ctr = 0, cnt = 0, rank = 0, bytes = 0; };
inline FoldScratch fold_scratch_layout(uint64_t n, uint64_t L, uint64_t ctr_bytes) {
  const uint64_t nw = (n + 63) / 64;
  FoldScratch s;
  s.sums = 8 * nw;
  s.ctr = s.sums + 8 * (dict_retire_scan_tiles(n) + 1);
  s.cnt = s.ctr + ctr_bytes;
  s.rank = s.cnt + 4 * nw;
  s.bytes = s.rank + 4 * L;
  return s;
}

// What the counters of a fold over n chunks in L layers say: the first refusal in
// the order layer cut, kind, length, then counts no table can give.
struct FoldVerdict {
  enum Why { ok, bad_layer, bad_kind, bad_len, insane } why = ok;
  uint64_t k = 0, b = 0;          // NEW chunks; layers with one
  uint64_t which = 0, count = 0;  // the first bad layer / chunk; how many such chunks
};
inline FoldVerdict fold_counts_verdict(const uint64_t *ctr, uint64_t n, uint64_t L) {
  FoldVerdict v;
  v.k = ctr[kFoldK];
  v.b = ctr[kFoldBlobs];
  if (ctr[kFoldBadLayer1])
    v.why = FoldVerdict::bad_layer, v.which = ~ctr[kFoldBadLayer1];
  else if (ctr[kFoldBadKind])
    v.why = FoldVerdict::bad_kind, v.which = ~ctr[kFoldBadKind1], v.count = ctr[kFoldBadKind];
  else if (ctr[kFoldBadLen])
    v.why = FoldVerdict::bad_len, v.which = ~ctr[kFoldBadLen1], v.count = ctr[kFoldBadLen];
  else if (v.k > n || v.b > L || v.b > v.k)
    v.why = FoldVerdict::insane;
  return v;
}

// ---- what the kernels compute ---------------------------------------------------
constexpr uint32_t kFoldKindNew = 0, kFoldKindDict = 2;  // NGPU_NEW, NGPU_DICT (nydus_gpu.h)

// first[0, L + 1) are layer cuts of n chunks: first[0] = 0, first[L] = n, no
// entry smaller than the one before.  false: *bad = the first layer out of order.
inline bool dict_fold_layers_ok(const uint64_t *first, uint64_t L, uint64_t n, uint64_t *bad) {
  for (uint64_t l = 0; l < L; ++l) {
    const uint64_t lo = first[l], hi = first[l + 1];
    if (lo > hi || hi > n || (l == 0 && lo != 0) || (l == L - 1 && hi != n)) {
      if (bad) *bad = l;
      return false;
    }
  }
  return true;
}

struct DictFoldMap {
  bool ok = false;              // false: bad_chunk holds a kind that is no dedup outcome
  uint64_t bad_chunk = 0;
  uint64_t k = 0, b = 0;        // NEW chunks; layers with one
  std::vector<uint64_t> words;  // keep word per 64 chunks (bits past n are 0)
  std::vector<uint32_t> prefix; // NEW chunks before each word
  std::vector<uint32_t> lrank;  // per layer: layers before it with a NEW chunk
  // NEW chunks before chunk c (c <= n)
  uint64_t rank(uint64_t c, uint64_t n) const {
    if (c >= n) return k;
    return (uint64_t)prefix[c >> 6] + (uint64_t)__builtin_popcountll(words[c >> 6] & ((1ull << (c & 63)) - 1));
  }
  // the record position of NEW chunk c among the call's new records
  uint64_t position(uint64_t c) const {
    return (uint64_t)prefix[c >> 6] + (uint64_t)__builtin_popcountll(words[c >> 6] & ((1ull << (c & 63)) - 1));
  }
  // the layer of chunk c: the last one that starts at or before it
  static uint64_t layer_of(const uint64_t *first, uint64_t L, uint64_t c) {
    uint64_t lo = 0, hi = L;
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (first[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
  }
};

// kinds[0, n); first: L + 1 cuts that passed dict_fold_layers_ok (null: one layer).
inline DictFoldMap dict_fold_map(const uint32_t *kinds, uint64_t n, const uint64_t *first, uint64_t L) {
  DictFoldMap f;
  for (uint64_t c = 0; c < n; ++c)
    if (kinds[c] > kFoldKindDict) {
      f.bad_chunk = c;
      return f;
    }
  f.ok = true;
  const uint64_t nw = (n + 63) / 64;
  f.words.assign(nw, 0);
  f.prefix.assign(nw, 0);
  for (uint64_t c = 0; c < n; ++c)
    if (kinds[c] == kFoldKindNew) f.words[c >> 6] |= 1ull << (c & 63);
  for (uint64_t w = 0; w < nw; ++w) {
    f.prefix[w] = (uint32_t)f.k;
    f.k += (uint64_t)__builtin_popcountll(f.words[w]);
  }
  if (!first) L = 1;
  f.lrank.assign(L, 0);
  for (uint64_t l = 0; l < L; ++l) {
    const uint64_t lo = first ? first[l] : 0, hi = first ? first[l + 1] : n;
    f.lrank[l] = (uint32_t)f.b;
    f.b += f.rank(hi, n) > f.rank(lo, n);
  }
  return f;
}

}  // namespace ngpu
