// node_fold_plan.hpp — the host plan of node dict fold (node.hip,
// ngpu_node_dict_fold): from every part's counts (k_i NEW chunks, b_i layers
// with one, c[i][o] of its NEW chunks owned by part o) the record and blob
// offsets of each part's rows, the per-owner totals and where every (source i,
// owner o) segment starts on both sides of the copy; the limits and refusal
// rules (dict_fold_plan.hpp's, over the sums); and a CPU restatement of the
// stable split by owner the kernels (node_fold.hip) run over a part's staged rows.
// Checked on the CPU by tests/cpp/node_fold_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h> and <vector>.
#pragma once
#include <stdint.h>

#include <vector>

#include "dict_fold_plan.hpp"
#include "dict_grow_plan.hpp"
#include "dict_hash.hpp"

namespace ngpu {

constexpr uint32_t kNodeFoldMaxParts = 64;  // W: the owner histogram's bins
constexpr uint64_t kNodeSplitTile = 256;    // rows per tile of the split

// ---- offsets --------------------------------------------------------------------
// The new rows are part 0's, then part 1's, ...: part i's rows take global ids
// entries(base) + off[i] + position and blobs blobs(base) + boff[i] + layer rank.
// Partitioned (c given, W x W): owner o appends total[o] rows, the (i, o)
// segments in source order; segment (i, o) starts at row src[i * W + o] of part
// i's split rows (owners back to back) and lands at row dst[i * W + o] of owner
// o's new rows.
struct NodeFoldPlan {
  bool ok = false;             // false: part `bad` owns k rows but its owner counts add up to another number
  uint32_t bad = 0;
  uint64_t K = 0, B = 0;       // all NEW chunks; all layers with one
  std::vector<uint64_t> off, boff;  // W + 1 each
  std::vector<uint64_t> total;      // W (partitioned)
  std::vector<uint64_t> src, dst;   // W x W (partitioned)
};
inline NodeFoldPlan node_fold_plan(uint32_t W, const uint64_t *k, const uint64_t *b, const uint32_t *c) {
  NodeFoldPlan p;
  p.off.assign(W + 1, 0);
  p.boff.assign(W + 1, 0);
  for (uint32_t i = 0; i < W; ++i) {
    p.off[i + 1] = p.off[i] + k[i];
    p.boff[i + 1] = p.boff[i] + b[i];
  }
  p.K = p.off[W];
  p.B = p.boff[W];
  p.ok = true;
  if (!c) return p;
  p.total.assign(W, 0);
  p.src.assign((size_t)W * W, 0);
  p.dst.assign((size_t)W * W, 0);
  for (uint32_t i = 0; i < W; ++i) {
    uint64_t at = 0;
    for (uint32_t o = 0; o < W; ++o) {
      p.src[(size_t)i * W + o] = at;
      p.dst[(size_t)i * W + o] = p.total[o];
      at += c[(size_t)i * W + o];
      p.total[o] += c[(size_t)i * W + o];
    }
    if (at != k[i] && p.ok) {
      p.ok = false;
      p.bad = i;
    }
  }
  return p;
}

// ---- limits and refusals over the sums ------------------------------------------
enum NodeFoldLimit : int {
  kNodeFoldFits = 0,
  kNodeFoldEntries = -1,  // entries(base) + K reaches the id limit
  kNodeFoldBlobs = -2     // blobs(base) + B passes 2^20
};
inline NodeFoldLimit node_fold_limits(uint64_t base_m, uint32_t base_blobs, uint64_t K, uint64_t B) {
  if (base_m >= kDictMaxEntries || K >= kDictMaxEntries - base_m) return kNodeFoldEntries;
  if (B > (1u << 20) || base_blobs + B > (1u << 20)) return kNodeFoldBlobs;
  return kNodeFoldFits;
}
// dict fold's placement and blob-table rules, stated over the call's totals: the
// placements and the blob-table rows are given in the global order of the rows.
inline DictFoldPlace node_fold_place_rule(uint64_t base_m, bool base_keeps, bool given,
                                          uint64_t n_placements, const NodeFoldPlan &p) {
  return dict_fold_place_rule(base_m, base_keeps, given, n_placements, p.K);
}
inline DictTableRule node_fold_table_rule(uint32_t base_blobs, bool base_has, bool call_has,
                                          uint32_t n_blobs, const NodeFoldPlan &p) {
  return dict_table_rule(base_blobs, base_has, call_has, p.K, n_blobs);
}
// A blob table, when one is passed, has one row per layer with a NEW chunk.
inline bool node_fold_table_rows_ok(bool call_has, uint32_t n_blobs, const NodeFoldPlan &p) {
  return !call_has || n_blobs == p.B;
}

// ---- what the split kernels compute ---------------------------------------------
// w0[r]: digest word 0 of staged row r (k rows).  Launch 1 counts every tile's
// rows per owner (cnt[o * T + t], T tiles of kNodeSplitTile rows), launches 2-4
// scan that array in place (owner-major: owner o's rows start where the owners
// below it end), launch 5 moves row r to base[o * T + t] + its rank among the
// earlier rows of its tile with the same owner.
struct NodeFoldSplit {
  uint64_t T = 0;
  std::vector<uint32_t> base;  // W x T: exclusive scan of the tile x owner counts
  std::vector<uint64_t> dest;  // per row
  std::vector<uint64_t> count; // per owner
};
inline NodeFoldSplit node_fold_split(const uint32_t *w0, uint64_t k, uint32_t W) {
  NodeFoldSplit s;
  s.T = (k + kNodeSplitTile - 1) / kNodeSplitTile;
  s.base.assign((size_t)W * s.T, 0);
  s.dest.assign(k, 0);
  s.count.assign(W, 0);
  for (uint64_t r = 0; r < k; ++r) {
    const uint32_t o = owner_of(w0[r], W);
    ++s.base[(size_t)o * s.T + r / kNodeSplitTile];
    ++s.count[o];
  }
  uint32_t run = 0;
  for (uint32_t &x : s.base) {
    const uint32_t v = x;
    x = run;
    run += v;
  }
  std::vector<uint32_t> seen(W);
  for (uint64_t t = 0; t < s.T; ++t) {
    seen.assign(W, 0);
    for (uint64_t r = t * kNodeSplitTile; r < k && r < (t + 1) * kNodeSplitTile; ++r) {
      const uint32_t o = owner_of(w0[r], W);
      s.dest[r] = (uint64_t)s.base[(size_t)o * s.T + t] + seen[o]++;
    }
  }
  return s;
}

}  // namespace ngpu
