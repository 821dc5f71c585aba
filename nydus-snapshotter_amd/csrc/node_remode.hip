// node_remode.hip — the device side of node dict remode (node.hip,
// ngpu_node_dict_remode) that retire and save do not already have.
//
// Split (replicated -> partitioned), per part o over the replica on its own device:
//   remode_owner_keep_words  a lane per row: keep = owner_of(digest word 0, W) == o,
//                            keep word and popcount by one ballot (dict_keep_words'
//                            shape, dict_retire.hip)
//   launch_retire_scan       the popcounts -> prefixes and s_o (unchanged)
//   remode_split_compact     dict_compact with the blob left alone and gid = the
//                            row's position in the replica, its entry id in base
// Join (partitioned -> replicated), per replica and window of global ids:
//   remode_join_scatter      row -> rec[gid], four lanes x 16 B per row; bit gid of
//                            a bitmap; an id >= m, an id outside the window and a
//                            bit found set are counted (and the row is not written)
//   remode_bitmap_count      the bitmap's set bits, next to those counters
//
// The table of every part is then built by the existing launch_dict_build.
// Roofline: HBM-bound.  The split reads every row's line once for 4 bytes of it and
// the kept lines whole, and writes them: (1 + 2 / W) x 64 B per row and part.  The
// join reads and writes every row once per replica (128 B), the bitmap is one
// atomic per row on a word that 32 neighbouring ids share (a slice ascends by id,
// so the atomics of a wave fall into a few words) (DESIGN.md §3 "Node dict remode").
#include "common.hpp"
#include "dict_hash.hpp"
#include "node_remode_plan.hpp"

namespace ngpu {
namespace {

// Lanes past m vote 0, so every word of (m + 63) / 64 is written whole.
__global__ __launch_bounds__(256) void remode_owner_keep_words(const DictRec *__restrict__ rec, uint64_t m,
                                                               uint32_t W, uint32_t o,
                                                               uint64_t *__restrict__ words,
                                                               uint32_t *__restrict__ cnt) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  bool keep = false;
  if (i < m) keep = owner_of(rec[i].digest[0], W) == o;
  const uint64_t w = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && i < m) {  // i < m: word i / 64 exists
    words[i >> 6] = w;
    cnt[i >> 6] = (uint32_t)__popcll(w);
  }
}

// dict_compact (dict_retire.hip) with two differences: the blob stays as it is, and
// the lane holding {usize, blob, index, gid} sets gid to the row's position r in the
// replica.  Reads are bounded by m, writes by s.
constexpr int kSplitCompactWords = 4;

__global__ __launch_bounds__(256) void remode_split_compact(const DictRec *__restrict__ rec, uint64_t m,
                                                            const uint64_t *__restrict__ words,
                                                            const uint32_t *__restrict__ prefix,
                                                            DictRec *__restrict__ out, uint64_t s) {
  const uint64_t nw = (m + 63) / 64;
  const uint32_t bit = threadIdx.x >> 2, q = threadIdx.x & 3;
#pragma unroll
  for (int k = 0; k < kSplitCompactWords; ++k) {
    const uint64_t wi = blockIdx.x * (uint64_t)kSplitCompactWords + k;
    if (wi >= nw) break;
    const uint64_t word = words[wi];
    const uint64_t r = wi * 64 + bit;
    if (!((word >> bit) & 1) || r >= m) continue;
    const uint64_t dst = (uint64_t)prefix[wi] + (uint64_t)__popcll(word & ((1ull << bit) - 1));
    if (dst >= s) continue;
    uint4 v = reinterpret_cast<const uint4 *>(rec + r)[q];
    if (q == 2) v.w = (uint32_t)r;
    reinterpret_cast<uint4 *>(out + dst)[q] = v;
  }
}

// rows[0, n): one part's slice (or the staged slices of several) of the window of
// ids [a, a + c) of a dict of m entries.  Four lanes per row, 16 B each, as
// split_scatter (node_fold.hip) moves rows; the lane of piece 2 holds the id and
// hands it to the row's other three.  A row is written only when its id is below m,
// inside the window and its bit was clear: out has m rows, bits (m + 63) / 64 words.
__global__ __launch_bounds__(256) void remode_join_scatter(const DictRec *__restrict__ rows, uint64_t n,
                                                           uint64_t a, uint64_t c, uint64_t m,
                                                           DictRec *__restrict__ out,
                                                           uint32_t *__restrict__ bits,
                                                           unsigned long long *__restrict__ ctr) {
  const uint64_t t = blockIdx.x * 256ull + threadIdx.x;
  const uint64_t j = t >> 2;
  const uint32_t q = threadIdx.x & 3;
  uint4 v = make_uint4(0, 0, 0, 0);
  if (j < n) v = reinterpret_cast<const uint4 *>(rows + j)[q];
  int ok = 0;
  if (j < n && q == 2) {
    const uint64_t g = v.w;
    if (g >= m) {
      atomicAdd(ctr + kRemodeBadGid, 1ull);
    } else if (g < a || g - a >= c) {
      atomicAdd(ctr + kRemodeOutside, 1ull);
    } else {
      const uint32_t bit = 1u << (g & 31);
      if (atomicOr(bits + (g >> 5), bit) & bit) atomicAdd(ctr + kRemodeDupBit, 1ull);
      else ok = 1;
    }
  }
  // (every lane of the wave takes part in the shuffles: no early return above)
  const int lane2 = (int)((threadIdx.x & 60) | 2);  // the row's lane of piece 2
  const uint32_t g = __shfl(v.w, lane2);
  ok = __shfl(ok, lane2);
  if (ok) reinterpret_cast<uint4 *>(out + g)[q] = v;
}

// The set bits of words[0, nw) added to *total.
__global__ __launch_bounds__(256) void remode_bitmap_count(const uint64_t *__restrict__ words, uint64_t nw,
                                                           unsigned long long *__restrict__ total) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint32_t c = i < nw ? (uint32_t)__popcll(words[i]) : 0u;
#pragma unroll
  for (int d = 32; d; d >>= 1) c += __shfl_down(c, d);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(total, (unsigned long long)c);
}

}  // namespace

void launch_remode_split_keep_scan(const DictRec *rec, uint64_t m, uint32_t W, uint32_t o, uint64_t *words,
                                   uint32_t *cnt, uint64_t *sums, hipStream_t s) {
  if (m)
    hipLaunchKernelGGL(remode_owner_keep_words, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, rec, m,
                       W, o, words, cnt);
  launch_retire_scan(cnt, (m + 63) / 64, sums, s);
}

void launch_remode_split_compact(const DictRec *rec, uint64_t m, const uint64_t *words,
                                 const uint32_t *prefix, DictRec *out, uint64_t s_o, hipStream_t s) {
  if (m == 0 || s_o == 0) return;
  const uint64_t nw = (m + 63) / 64;
  hipLaunchKernelGGL(remode_split_compact, dim3((unsigned)((nw + kSplitCompactWords - 1) / kSplitCompactWords)),
                     dim3(256), 0, s, rec, m, words, prefix, out, s_o);
}

void launch_remode_join_scatter(const DictRec *rows, uint64_t n, uint64_t a, uint64_t c, uint64_t m,
                                DictRec *out, uint64_t *bits, uint64_t *ctr, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(remode_join_scatter, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, s, rows, n, a,
                     c, m, out, reinterpret_cast<uint32_t *>(bits), reinterpret_cast<unsigned long long *>(ctr));
}

void launch_remode_bitmap_count(const uint64_t *bits, uint64_t m, uint64_t *ctr, hipStream_t s) {
  const uint64_t nw = (m + 63) / 64;
  if (nw)
    hipLaunchKernelGGL(remode_bitmap_count, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, bits, nw,
                       reinterpret_cast<unsigned long long *>(ctr + kRemodeSet));
}

}  // namespace ngpu
