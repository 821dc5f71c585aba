// node_distill.hip — the device side of distilling a partitioned node dict
// (node.hip, ngpu_node_dict_distill_parts) that dict distill (dict_distill.hip)
// and the retire across parts (node_retire.hip) do not already have: one pass
// that does what distill_keep_words and node_keep_words do in two.
//
//   launch_dict_ref_count     per part, over its own table: slots hold local row
//                             indices, rows are in ascending gid order and all
//                             rows of a digest live on one part, so refs[i] > 0
//                             iff local row i wins globally (unchanged)
//   node_distill_keep_words   keep = refs[i] >= min_refs: the keep word and
//                             popcount, the blob-live bit of every survivor, the
//                             counters of ngpu_dict_distill_info, and bit gid of
//                             the part's bitmap over [0, m) for every kept row
//   launch_retire_scan        the local popcounts -> prefixes and s_o (unchanged)
//
// The exchange, the global scan, the compaction and the table build are
// node_retire.hip's and dict.hip's.  Roofline: HBM-bound like dict distill's
// second pass -- 4 B of refs per row and one 16-B quarter of every survivor's
// record line, read once for both its blob and its gid (DESIGN.md §3 "Node dict
// distill across parts").
#include "common.hpp"
#include "node_distill_plan.hpp"

namespace ngpu {
namespace {

__device__ __forceinline__ void live_set(uint32_t *live, uint32_t b) {
  const uint32_t bit = 1u << (b & 31);
  // (a stale read only costs the atomic it would have saved)
  if (!(__hip_atomic_load(live + (b >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
    atomicOr(live + (b >> 5), bit);
}

// The workgroup's counters in LDS: distill's kDistillStatWords, then the two of
// the keep pass of a retire across parts.
constexpr int kShBadGid = kDistillStatWords, kShDupBit = kDistillStatWords + 1;
constexpr int kShWords = kDistillStatWords + 2;

// min_refs >= 1.  Lanes past m_o vote 0, so every word of (m_o + 63) / 64 is
// written whole.  live / stats: as distill_keep_words has them.  gbits / ctr: as
// node_keep_words has them -- a kept row sets bit gid of gbits (32-bit words), a
// run of neighbouring lanes that share a 32-bit word folds its bits into its
// first lane, which issues the run's one atomic OR; a kept row with gid >= m
// writes nothing and is counted, and so is an OR that finds one of its bits set.
// Only a survivor reads its record, so a row that leaves has no word of its own:
// it takes the word of the nearest kept lane below it (one shuffle, the lane
// from the ballot) and so does not cut the run it stands in.  Every kept row's
// bit is in exactly one run, so the fold is right for any order of the gids.
__global__ __launch_bounds__(256) void node_distill_keep_words(
    const DictRec *__restrict__ rec, uint64_t m_o, const uint32_t *__restrict__ refs, uint32_t min_refs,
    uint32_t n_blobs, uint64_t m, uint64_t per, uint64_t *__restrict__ words, uint32_t *__restrict__ cnt,
    uint32_t *__restrict__ live, uint64_t *__restrict__ stats, uint32_t *__restrict__ gbits,
    uint64_t *__restrict__ ctr) {
  __shared__ uint32_t sh[kShWords];
  if (threadIdx.x < kShWords) sh[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  uint32_t last_b = kNone;  // wave-uniform: the blob this wave set last
  const uint64_t t0 = blockIdx.x * per;
  for (uint64_t t = t0; t < t0 + per && t * 256 < m_o; ++t) {  // (uniform in the workgroup)
    const uint64_t i = t * 256 + threadIdx.x;
    const uint32_t r = i < m_o ? refs[i] : 0;
    const bool win = r > 0, keep = r >= min_refs;
    const uint64_t w = __ballot(keep);
    if (lane == 0 && i < m_o) {  // i < m_o: word i / 64 exists
      words[i >> 6] = w;
      cnt[i >> 6] = (uint32_t)__popcll(w);
    }
    if (w) {  // (uniform in the wave)
      // a survivor's {usize, blob, index, gid}: read once for the blob and the gid
      uint32_t b = 0, g = 0;
      if (keep) {
        const uint4 v = reinterpret_cast<const uint4 *>(rec + i)[2];
        b = v.y;
        g = v.w;
      }
      // the survivors' blobs: one OR per wave when they agree
      const bool lb = keep && b < n_blobs;
      const uint64_t lbm = __ballot(lb);
      if (lbm) {
        const uint32_t lead = (uint32_t)__builtin_ctzll(lbm);
        const uint32_t b0 = (uint32_t)__shfl((int)b, (int)lead, 64);
        if (__all(!lb || b == b0)) {
          if (b0 != last_b && lane == lead) live_set(live, b0);
          last_b = b0;
        } else if (lb) {
          live_set(live, b);
        }
      }
      // the survivors' gids: one OR per run of lanes in one 32-bit word
      const bool valid = keep && g < m;
      const uint64_t vm = __ballot(valid);
      const uint64_t nbad = w & ~vm;
      constexpr uint32_t kNoWord = 0xFFFFFFFFu;  // (word indices are below 2^27)
      const uint64_t below = vm & ((1ull << lane) - 1);
      const uint32_t src = valid || !below ? lane : 63u - (uint32_t)__builtin_clzll(below);
      const uint32_t wi = (uint32_t)__shfl((int)(valid ? g >> 5 : kNoWord), (int)src, 64);
      uint32_t bits = valid ? 1u << (g & 31) : 0u;
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
        if (nbad) atomicAdd(&sh[kShBadGid], (uint32_t)__popcll(nbad));
        if (ndup) atomicAdd(&sh[kShDupBit], (uint32_t)__popcll(ndup));
      }
    }
    // the counters: per wave where a ballot or a reduction gives them
    const uint64_t wm = __ballot(win);
    if (wm) {
      const uint64_t bm = __ballot(win && !keep);
      uint32_t mx = r;
#pragma unroll
      for (int o = 32; o; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
      const uint32_t k = win ? distill_bucket(r) : 0;
      const uint32_t lead = (uint32_t)__builtin_ctzll(wm);
      const uint32_t k0 = (uint32_t)__shfl((int)k, (int)lead, 64);
      const bool one = __all(!win || k == k0);
      if (lane == lead) {
        atomicAdd(&sh[kDistillDistinct], (uint32_t)__popcll(wm));
        if (bm) atomicAdd(&sh[kDistillBelowMin], (uint32_t)__popcll(bm));
        atomicMax(&sh[kDistillMaxRefs], mx);
        if (one) atomicAdd(&sh[kDistillHist + k0], (uint32_t)__popcll(wm));
      }
      if (!one && win) atomicAdd(&sh[kDistillHist + k], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < kShWords && sh[threadIdx.x]) {
    const unsigned long long v = sh[threadIdx.x];
    if (threadIdx.x == kDistillMaxRefs)
      atomicMax((unsigned long long *)(stats + threadIdx.x), v);
    else if (threadIdx.x < kDistillStatWords)
      atomicAdd((unsigned long long *)(stats + threadIdx.x), v);
    else
      atomicAdd((unsigned long long *)(ctr + (threadIdx.x == kShBadGid ? kNodeRetireBadGid : kNodeRetireDupBit)), v);
  }
}

}  // namespace

void launch_node_distill_keep_scan(const DictRec *rec, uint64_t m_o, const uint32_t *refs, uint32_t min_refs,
                                   uint32_t n_blobs, uint64_t m, uint64_t *words, uint32_t *cnt,
                                   uint64_t *sums, uint32_t *live, uint64_t *stats, uint64_t *gbits,
                                   uint64_t *ctr, hipStream_t s) {
  if (m_o) {
    const uint64_t per = distill_tiles_per_wg(m_o), tiles = (m_o + 255) / 256;
    hipLaunchKernelGGL(node_distill_keep_words, dim3((unsigned)((tiles + per - 1) / per)), dim3(256), 0, s,
                       rec, m_o, refs, min_refs ? min_refs : 1u, n_blobs, m, per, words, cnt, live, stats,
                       reinterpret_cast<uint32_t *>(gbits), ctr);
  }
  launch_retire_scan(cnt, (m_o + 63) / 64, sums, s);
}

}  // namespace ngpu
