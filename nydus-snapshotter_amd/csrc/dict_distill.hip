// dict_distill.hip — the device side of dict distill (dict.hip,
// ngpu_dict_distill) that dict retire (dict_retire.hip) does not already have:
// how many rows hold each digest, and the keep words that follow from it.
//
//   1. dict_ref_count      a lane per row: walk the table from the row's home slot
//                          to the slot of its digest (dict_hash.hpp's rules,
//                          dict_find's skips) and add 1 to refs[winner]
//   2. distill_keep_words  keep = refs[i] >= min_refs: dict_keep_words' keep word
//                          and popcount, one bit per surviving row's blob, and the
//                          counters of ngpu_dict_distill_info
//      launch_retire_scan  the popcounts -> prefixes and the total (unchanged)
//
// The compaction and the table build are retire's (launch_dict_compact,
// launch_dict_build).  Roofline: HBM-bound, latency-bound where chains are long.
// Pass 1 reads every record's line for its digest and one slot line per row,
// plus the winner's record line for every row that does not win (a winner finds
// its own id in the slot and reads no record); pass 2 reads 4 B of refs per row
// and the record line of every survivor for its blob (DESIGN.md §3 "Dict
// distill").
#include "common.hpp"
#include "dict_distill_plan.hpp"

namespace ngpu {
namespace {

// Both kernels give a workgroup a run of whole 256-row tiles, distill_tiles_per_wg
// of them: at least 4, and as many as it takes for kDistillGrid workgroups to
// cover the dict.  What a workgroup adds to words other workgroups add to (the
// count of a hot digest, the counters) is carried over its tiles and leaves
// once, so the atomics on one address go with the number of workgroups, not with
// the number of waves (16 M rows: 250,000 waves, 2,048 workgroups).
// (distill_tiles_per_wg: dict_distill_plan.hpp; node_distill.hip runs by it too.)

// refs[key] += 1 for the lanes with act set.  Rows of one digest often sit in one
// wave (a zero chunk in every layer, a layer extended twice): the lanes that
// share the first pending lane's key are counted by a ballot and leave as one
// atomic, for up to kAggRounds distinct keys; lanes still pending after that add
// for themselves.  The first key's count does not leave at once: it is carried
// in (ckey, ccnt), wave-uniform, and added to while the next calls meet the same
// key; the caller flushes what is left with wave_add_flush.  The sums are the
// same whichever way a lane's 1 arrives.  Every lane of the wave must call this.
constexpr int kAggRounds = 8;

__device__ __forceinline__ void wave_add_flush(uint32_t *base, uint32_t ckey, uint32_t ccnt) {
  if (ccnt && (threadIdx.x & 63) == 0) atomicAdd(base + ckey, ccnt);
}

__device__ __forceinline__ void wave_add_u32(uint32_t *base, bool act, uint32_t key, uint32_t &ckey,
                                             uint32_t &ccnt) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t pend = __ballot(act);
  for (int r = 0; pend && r < kAggRounds; ++r) {  // (pend is uniform)
    const uint32_t lead = (uint32_t)__builtin_ctzll(pend);
    const uint32_t k0 = (uint32_t)__shfl((int)key, (int)lead, 64);
    const bool hit = act && key == k0;
    const uint64_t same = __ballot(hit);
    const uint32_t c = (uint32_t)__popcll(same);
    if (r == 0) {
      if (k0 != ckey) {
        wave_add_flush(base, ckey, ccnt);
        ckey = k0;
        ccnt = 0;
      }
      ccnt += c;
    } else if (lane == lead) {
      atomicAdd(base + k0, c);
    }
    if (hit) act = false;
    pend &= ~same;
  }
  if (act) atomicAdd(base + key, 1u);
}

// refs: m words, zeroed.  Afterwards refs[i] > 0 iff row i is the first row of
// its digest, and then it is the number of rows of rec[0, m) with that digest.
// The slot of a digest holds the smallest id that has it, so a tag match on the
// row's own id ends the walk with no record read; a match on a smaller id is
// compared on the 32 digest bytes; an id >= m is a row a later in-place extend
// appended (dict.hip "dict extend"), skipped unread.  The walk is bounded by the
// table's size; a row that does not find its digest (no table built by
// launch_dict_build leaves one out) counts as its own winner and stays.
__global__ __launch_bounds__(256) void dict_ref_count(const DictRec *__restrict__ rec, uint64_t m,
                                                      const uint64_t *__restrict__ table,
                                                      uint64_t mask, uint64_t per,
                                                      uint32_t *__restrict__ refs) {
  uint32_t ckey = kNone, ccnt = 0;
  const uint64_t t0 = blockIdx.x * per;
  for (uint64_t t = t0; t < t0 + per && t * 256 < m; ++t) {  // (uniform in the workgroup)
    const uint64_t i = t * 256 + threadIdx.x;
    const bool act = i < m;
    uint32_t win = (uint32_t)i;
    if (act) {
      const uint4 *r = reinterpret_cast<const uint4 *>(rec + i);
      const uint4 a = r[0], b = r[1];
      const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
      const uint32_t tag = digest_tag(d);
      uint64_t p = digest_bucket(d) & mask;
      for (uint64_t step = 0; step <= mask; ++step, p = (p + 1) & mask) {
        const uint64_t s = table[p];
        if (s == kEmpty) break;
        if ((uint32_t)(s >> 32) != tag) continue;
        const uint32_t e = (uint32_t)s;
        if (e == (uint32_t)i) break;
        if (e >= m) continue;
        const uint4 *o = reinterpret_cast<const uint4 *>(rec + e);
        const uint4 x = o[0], y = o[1];
        if (((a.x ^ x.x) | (a.y ^ x.y) | (a.z ^ x.z) | (a.w ^ x.w) | (b.x ^ y.x) | (b.y ^ y.y) |
             (b.z ^ y.z) | (b.w ^ y.w)) == 0) {
          win = e;
          break;
        }
      }
    }
    // self-winning lanes add to neighbouring words: as they are
    const bool self = act && win == (uint32_t)i;
    if (self) atomicAdd(refs + i, 1u);
    wave_add_u32(refs, act && !self, win, ckey, ccnt);
  }
  wave_add_flush(refs, ckey, ccnt);
}

__device__ __forceinline__ void live_set(uint32_t *live, uint32_t b) {
  const uint32_t bit = 1u << (b & 31);
  // (a stale read only costs the atomic it would have saved)
  if (!(__hip_atomic_load(live + (b >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit))
    atomicOr(live + (b >> 5), bit);
}

// min_refs >= 1.  Lanes past m vote 0, so every word of (m + 63) / 64 is written
// whole, in dict_keep_words' format.  live: one bit per blob of the dict, zeroed;
// a surviving row whose blob is not a blob of the dict (dict_keep_words) sets
// none; a wave whose survivors agree on the blob sets it once, and not again
// while its next tiles agree with it.  stats: kDistillStatWords u64, zeroed; a
// workgroup reduces its counters in LDS over all its tiles and issues one atomic
// per counter that is not 0.
__global__ __launch_bounds__(256) void distill_keep_words(const DictRec *__restrict__ rec, uint64_t m,
                                                          const uint32_t *__restrict__ refs,
                                                          uint32_t min_refs, uint32_t n_blobs,
                                                          uint64_t per, uint64_t *__restrict__ words,
                                                          uint32_t *__restrict__ cnt,
                                                          uint32_t *__restrict__ live,
                                                          uint64_t *__restrict__ stats) {
  __shared__ uint32_t sh[kDistillStatWords];
  if (threadIdx.x < kDistillStatWords) sh[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  uint32_t last_b = kNone;  // wave-uniform: the blob this wave set last
  const uint64_t t0 = blockIdx.x * per;
  for (uint64_t t = t0; t < t0 + per && t * 256 < m; ++t) {  // (uniform in the workgroup)
    const uint64_t i = t * 256 + threadIdx.x;
    const uint32_t r = i < m ? refs[i] : 0;
    const bool win = r > 0, keep = r >= min_refs;
    const uint64_t w = __ballot(keep);
    if (lane == 0 && i < m) {  // i < m: word i / 64 exists
      words[i >> 6] = w;
      cnt[i >> 6] = (uint32_t)__popcll(w);
    }
    // the survivors' blobs: one OR per wave when they agree
    uint32_t b = 0;
    bool lb = false;
    if (keep) {
      b = rec[i].blob;
      lb = b < n_blobs;
    }
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
  if (threadIdx.x < kDistillStatWords && sh[threadIdx.x]) {
    unsigned long long *dst = (unsigned long long *)(stats + threadIdx.x);
    if (threadIdx.x == kDistillMaxRefs)
      atomicMax(dst, (unsigned long long)sh[threadIdx.x]);
    else
      atomicAdd(dst, (unsigned long long)sh[threadIdx.x]);
  }
}

}  // namespace

void launch_dict_ref_count(const DictRec *rec, uint64_t m, const uint64_t *table, uint64_t table_cap,
                           uint32_t *refs, hipStream_t s) {
  if (!m) return;
  const uint64_t per = distill_tiles_per_wg(m), tiles = (m + 255) / 256;
  hipLaunchKernelGGL(dict_ref_count, dim3((unsigned)((tiles + per - 1) / per)), dim3(256), 0, s, rec, m,
                     table, table_cap - 1, per, refs);
}

void launch_distill_keep_scan(const DictRec *rec, uint64_t m, const uint32_t *refs, uint32_t min_refs,
                              uint32_t n_blobs, uint64_t *words, uint32_t *cnt, uint64_t *sums,
                              uint32_t *live, uint64_t *stats, hipStream_t s) {
  if (m) {
    const uint64_t per = distill_tiles_per_wg(m), tiles = (m + 255) / 256;
    hipLaunchKernelGGL(distill_keep_words, dim3((unsigned)((tiles + per - 1) / per)), dim3(256), 0, s,
                       rec, m, refs, min_refs ? min_refs : 1u, n_blobs, per, words, cnt, live, stats);
  }
  launch_retire_scan(cnt, (m + 63) / 64, sums, s);
}

}  // namespace ngpu
