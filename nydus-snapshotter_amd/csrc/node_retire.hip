// node_retire.hip — the device side of retiring a partitioned node dict (node.hip,
// ngpu_node_dict_retire_parts) that dict retire (dict_retire.hip) does not
// already have: the rank of a part's kept rows over ALL parts' keep bits.
//
//   node_keep_words      per part, a lane per local row: dict_keep_words' keep word
//                        and popcount, and bit gid of the part's own bitmap over
//                        the dict's global ids [0, m) for every kept row
//   launch_retire_scan   the local popcounts -> prefixes and s_o (unchanged)
//   (host: every part's bitmap is copied to every part)
//   node_keep_merge      a lane per global word: the OR of the W bitmaps, its
//                        popcount, and a check that no bit came from two parts
//   launch_retire_scan   the global popcounts -> prefixes and S (unchanged)
//   node_retire_totals   s_o and S next to the three refusal counters: one copy back
//   node_dict_compact    dict_compact with gid = the global rank of the row's old id
//
// The table of every part is then built by the existing launch_dict_build.
// Roofline: HBM-bound like dict retire (pass 1 touches every record's line, the
// compaction reads the kept lines whole and writes them); added to it are W m / 8
// bytes of bitmaps copied in and read once, and a scan over m / 64 counts on
// every part (DESIGN.md §3 "Node dict retire across parts").
#include "common.hpp"
#include "node_retire_plan.hpp"

namespace ngpu {
namespace {

// Lanes past m_o vote 0, so every local word is written whole.  A kept row sets
// bit gid of gbits (32-bit words: bit g of the u64 word g / 64 is bit g % 32 of
// the u32 word g / 32).  A part's rows are in ascending gid order, so lanes that
// share a 32-bit word are neighbours: a run of neighbouring lanes with the same
// word index (rows that leave belong to their run too, with no bit) folds its bits
// into its first lane, which issues the run's one atomic OR.  Every kept row's bit
// is in exactly one run, so the fold is right for any order; only the number of
// atomics depends on it, and an OR that finds one of its bits set means an id held
// twice.  A row with gid >= m writes nothing and is counted.
__global__ __launch_bounds__(256) void node_keep_words(const DictRec *__restrict__ rec, uint64_t m_o,
                                                       const uint32_t *__restrict__ bitmap,
                                                       uint32_t n_blobs, uint64_t m,
                                                       uint64_t *__restrict__ words,
                                                       uint32_t *__restrict__ cnt,
                                                       uint32_t *__restrict__ gbits,
                                                       uint64_t *__restrict__ ctr) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  bool keep = false;
  uint32_t g = 0;
  if (i < m_o) {
    const uint4 v = reinterpret_cast<const uint4 *>(rec + i)[2];  // {usize, blob, index, gid}
    keep = v.y >= n_blobs || !((bitmap[v.y >> 5] >> (v.y & 31)) & 1);
    g = v.w;
  }
  const uint64_t w = __ballot(keep);
  if (lane == 0 && i < m_o) {  // i < m_o: word i / 64 exists
    words[i >> 6] = w;
    cnt[i >> 6] = (uint32_t)__popcll(w);
  }
  const bool valid = i < m_o && g < m;
  const uint64_t nbad = __ballot(keep && !valid);
  constexpr uint32_t kNoWord = 0xFFFFFFFFu;  // (word indices are below 2^27)
  const uint32_t wi = valid ? g >> 5 : kNoWord;
  uint32_t bits = keep && valid ? 1u << (g & 31) : 0u;
  const uint32_t left = __shfl_up(wi, 1);
  const bool head = lane == 0 || left != wi;
  // the run of this lane ends before the next head above it
  const uint64_t heads = __ballot(head);
  const uint64_t above = lane == 63 ? 0 : heads >> (lane + 1);
  const uint32_t end = above ? lane + 1 + (uint32_t)__builtin_ctzll(above) : 64;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t ob = __shfl_down(bits, d);
    if (lane + d < end) bits |= ob;
  }
  bool dup = false;
  if (head && bits) dup = (atomicOr(gbits + wi, bits) & bits) != 0;
  const uint64_t ndup = __ballot(dup);
  if (lane == 0) {
    if (nbad) atomicAdd((unsigned long long *)(ctr + kNodeRetireBadGid), (unsigned long long)__popcll(nbad));
    if (ndup) atomicAdd((unsigned long long *)(ctr + kNodeRetireDupBit), (unsigned long long)__popcll(ndup));
  }
}

// Global word j of every part's bitmap (gather: W x gnw, part p's at p * gnw).
__global__ __launch_bounds__(256) void node_keep_merge(const uint64_t *__restrict__ gather, uint32_t W,
                                                       uint64_t gnw, uint64_t *__restrict__ gwords,
                                                       uint32_t *__restrict__ gcnt,
                                                       uint64_t *__restrict__ ctr) {
  const uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  bool over = false;
  if (j < gnw) {
    uint64_t x = 0;
    uint32_t sum = 0;
    for (uint32_t p = 0; p < W; ++p) {
      const uint64_t w = gather[(uint64_t)p * gnw + j];
      x |= w;
      sum += (uint32_t)__popcll(w);
    }
    const uint32_t c = (uint32_t)__popcll(x);
    gwords[j] = x;
    gcnt[j] = c;
    over = sum != c;
  }
  const uint64_t nover = __ballot(over);
  if ((threadIdx.x & 63) == 0 && nover)
    atomicAdd((unsigned long long *)(ctr + kNodeRetireOverlap), (unsigned long long)__popcll(nover));
}

__global__ void node_retire_totals(const uint64_t *__restrict__ s_local,
                                   const uint64_t *__restrict__ s_global, uint64_t *__restrict__ ctr) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    ctr[kNodeRetireLocal] = *s_local;
    ctr[kNodeRetireGlobal] = *s_global;
  }
}

// dict_compact (dict_retire.hip) with one difference: four lanes per record, 16 B
// each, the destination from the LOCAL words and prefixes, the blob through the
// remap, reads bounded by m_o and writes by s_o; the lane holding {usize, blob,
// index, gid} sets gid to the rank of its old id g among all parts' keep bits.
// The global arrays are read only when g < m (a row whose id is not -- the keep
// pass counted it, and the host refuses before this launch -- keeps it).
constexpr int kNodeCompactWords = 4;

__global__ __launch_bounds__(256) void node_dict_compact(const DictRec *__restrict__ rec, uint64_t m_o,
                                                         const uint64_t *__restrict__ words,
                                                         const uint32_t *__restrict__ prefix,
                                                         const uint64_t *__restrict__ gwords,
                                                         const uint32_t *__restrict__ gprefix,
                                                         uint64_t m, const uint32_t *__restrict__ remap,
                                                         uint32_t n_blobs, DictRec *__restrict__ out,
                                                         uint64_t s_o) {
  const uint64_t nw = (m_o + 63) / 64;
  const uint32_t bit = threadIdx.x >> 2, q = threadIdx.x & 3;
#pragma unroll
  for (int k = 0; k < kNodeCompactWords; ++k) {
    const uint64_t wi = blockIdx.x * (uint64_t)kNodeCompactWords + k;
    if (wi >= nw) break;
    const uint64_t word = words[wi];
    const uint64_t r = wi * 64 + bit;
    if (!((word >> bit) & 1) || r >= m_o) continue;
    const uint64_t dst = (uint64_t)prefix[wi] + (uint64_t)__popcll(word & ((1ull << bit) - 1));
    if (dst >= s_o) continue;
    uint4 v = reinterpret_cast<const uint4 *>(rec + r)[q];
    if (q == 2) {
      if (v.y < n_blobs) v.y = remap[v.y];
      const uint64_t g = v.w;
      if (g < m)
        v.w = gprefix[g >> 6] + (uint32_t)__popcll(gwords[g >> 6] & ((1ull << (g & 63)) - 1));
    }
    reinterpret_cast<uint4 *>(out + dst)[q] = v;
  }
}

}  // namespace

void launch_node_keep_scan(const DictRec *rec, uint64_t m_o, const uint32_t *bitmap, uint32_t n_blobs,
                           uint64_t m, uint64_t *words, uint32_t *cnt, uint64_t *sums, uint64_t *gbits,
                           uint64_t *ctr, hipStream_t s) {
  if (m_o)
    hipLaunchKernelGGL(node_keep_words, dim3((unsigned)((m_o + 255) / 256)), dim3(256), 0, s, rec, m_o,
                       bitmap, n_blobs, m, words, cnt, reinterpret_cast<uint32_t *>(gbits), ctr);
  launch_retire_scan(cnt, (m_o + 63) / 64, sums, s);
}

void launch_node_keep_merge(const uint64_t *gather, uint32_t W, uint64_t m, uint64_t *gwords,
                            uint32_t *gcnt, uint64_t *gsums, const uint64_t *s_local, uint64_t *ctr,
                            hipStream_t s) {
  const uint64_t gnw = (m + 63) / 64;
  if (gnw)
    hipLaunchKernelGGL(node_keep_merge, dim3((unsigned)((gnw + 255) / 256)), dim3(256), 0, s, gather, W,
                       gnw, gwords, gcnt, ctr);
  launch_retire_scan(gcnt, gnw, gsums, s);
  hipLaunchKernelGGL(node_retire_totals, dim3(1), dim3(64), 0, s, s_local,
                     gsums + dict_retire_scan_tiles(m), ctr);
}

void launch_node_dict_compact(const DictRec *rec, uint64_t m_o, const uint64_t *words,
                              const uint32_t *prefix, const uint64_t *gwords, const uint32_t *gprefix,
                              uint64_t m, const uint32_t *remap, uint32_t n_blobs, DictRec *out,
                              uint64_t s_o, hipStream_t s) {
  if (m_o == 0 || s_o == 0) return;
  const uint64_t nw = (m_o + 63) / 64;
  hipLaunchKernelGGL(node_dict_compact, dim3((unsigned)((nw + kNodeCompactWords - 1) / kNodeCompactWords)),
                     dim3(256), 0, s, rec, m_o, words, prefix, gwords, gprefix, m, remap, n_blobs, out, s_o);
}

}  // namespace ngpu
