// dict_fold.hip — the device side of dict fold (dict.hip, ngpu_dict_fold and
// ngpu_dict_extend_device): the NEW chunks of a dedup call's result table become
// dict records without leaving HBM.
//
//   1. fold_keep_words    one keep bit per chunk (kind == NGPU_NEW), one ballot per
//                         wave64 -> keep word + popcount; the same pass counts
//                         kinds that are no dedup outcome and NEW chunks whose
//                         length no dict record can carry
//   2. launch_retire_scan exclusive scan of the popcounts (dict_retire.hip's
//                         reduce-then-scan, unchanged)
//   3. fold_layer_ranks   a layer's NEW count is rank(first[l + 1]) - rank(first[l]);
//                         the scan of "has one" is its blob rank, the total b
//   4. fold_scatter       NEW chunk c -> rec[m + prefix[c / 64] + popc(word below c)]
//
// The live table is then filled by launch_dict_insert_range (in place) or
// launch_dict_build (fork), as for every extend.  Roofline: launch-bound at a
// layer's size (n <= a few hundred thousand chunks: 4 B of every 64-B result
// row in pass 1, the NEW rows whole in pass 4); DESIGN.md §3 "Dict fold".
#include "common.hpp"

namespace ngpu {
namespace {

// Lanes past n vote 0, so every word of (n + 63) / 64 is written whole.  The
// first offending chunk is kept as ~id under an atomic max (0 = none).
__global__ __launch_bounds__(256) void fold_keep_words(const ngpu_result *__restrict__ res,
                                                       const ngpu_chunk *__restrict__ chunks,
                                                       uint64_t n, uint32_t chunk_size,
                                                       uint64_t *__restrict__ words,
                                                       uint32_t *__restrict__ cnt,
                                                       uint64_t *__restrict__ ctr) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  bool keep = false, bad_kind = false, bad_len = false;
  if (i < n) {
    const uint32_t kind = res[i].kind;
    keep = kind == NGPU_NEW;
    bad_kind = kind > NGPU_DICT;
    if (keep) {
      const uint32_t len = chunks[i].length;
      bad_len = len == 0 || len > chunk_size;
    }
  }
  const uint64_t w = __ballot(keep), bk = __ballot(bad_kind), bl = __ballot(bad_len);
  if ((threadIdx.x & 63) != 0 || i >= n) return;  // i: the wave's first chunk, word i / 64 exists
  words[i >> 6] = w;
  cnt[i >> 6] = (uint32_t)__popcll(w);
  if (bk) {
    atomicAdd((unsigned long long *)(ctr + kFoldBadKind), (unsigned long long)__popcll(bk));
    atomicMax((unsigned long long *)(ctr + kFoldBadKind1),
              (unsigned long long)~(i + (uint64_t)__builtin_ctzll(bk)));
  }
  if (bl) {
    atomicAdd((unsigned long long *)(ctr + kFoldBadLen), (unsigned long long)__popcll(bl));
    atomicMax((unsigned long long *)(ctr + kFoldBadLen1),
              (unsigned long long)~(i + (uint64_t)__builtin_ctzll(bl)));
  }
}

// NEW chunks before chunk c (c <= n; total: all of them).
__device__ __forceinline__ uint64_t fold_rank(const uint64_t *__restrict__ words,
                                              const uint32_t *__restrict__ prefix, uint64_t n,
                                              uint64_t total, uint64_t c) {
  if (c >= n) return total;
  return (uint64_t)prefix[c >> 6] + (uint64_t)__popcll(words[c >> 6] & ((1ull << (c & 63)) - 1));
}

// One workgroup over the L layers.  A layer whose bounds are not 0 <= first[l]
// <= first[l + 1] <= n (first[0] = 0, first[L] = n) is reported and reads no
// keep word; the host refuses the call before anything uses lrank.
__global__ __launch_bounds__(kTileThreads) void fold_layer_ranks(
    const uint64_t *__restrict__ words, const uint32_t *__restrict__ prefix,
    const uint64_t *__restrict__ sums_total, uint64_t n, const uint64_t *__restrict__ first,
    uint64_t L, uint32_t *__restrict__ lrank, uint64_t *__restrict__ ctr) {
  const uint64_t total = *sums_total;
  uint64_t carry = 0;
  for (uint64_t a = 0; a < L; a += kTileThreads) {  // (uniform trip count: barriers inside)
    const uint64_t l = a + threadIdx.x;
    uint64_t has = 0;
    if (l < L) {
      const uint64_t lo = first ? first[l] : 0, hi = first ? first[l + 1] : n;
      if (lo > hi || hi > n || (l == 0 && lo != 0) || (l == L - 1 && hi != n))
        atomicMax((unsigned long long *)(ctr + kFoldBadLayer1), (unsigned long long)~l);
      else
        has = fold_rank(words, prefix, n, total, hi) > fold_rank(words, prefix, n, total, lo);
    }
    uint64_t tot;
    const uint64_t x = block_exclusive_scan(has, &tot);
    if (l < L) lrank[l] = (uint32_t)(carry + x);
    carry += tot;
  }
  if (threadIdx.x == 0) {
    ctr[kFoldK] = total;
    ctr[kFoldBlobs] = carry;
  }
}

// Four lanes per NEW chunk, 16 B each, as dict_compact: a wave writes whole 64-B
// rows back to back.  Lanes 0-1 carry the digest, lane 2 {usize, blob, index,
// gid}, lane 3 the uncompressed offset.  A workgroup takes kFoldWords keep words.
// Reads are bounded by n and L, writes by k.
constexpr int kFoldWords = 4;

__global__ __launch_bounds__(256) void fold_scatter(
    const ngpu_result *__restrict__ res, const ngpu_chunk *__restrict__ chunks, uint64_t n,
    const uint64_t *__restrict__ words, const uint32_t *__restrict__ prefix,
    const uint64_t *__restrict__ first, uint64_t L, const uint32_t *__restrict__ lrank,
    uint32_t blob0, uint32_t gid0, DictRec *__restrict__ out, uint64_t k) {
  const uint64_t nw = (n + 63) / 64;
  const uint32_t bit = threadIdx.x >> 2, q = threadIdx.x & 3;
#pragma unroll
  for (int j = 0; j < kFoldWords; ++j) {
    const uint64_t wi = blockIdx.x * (uint64_t)kFoldWords + j;
    if (wi >= nw) break;
    const uint64_t word = words[wi];
    const uint64_t c = wi * 64 + bit;
    if (!((word >> bit) & 1) || c >= n) continue;
    const uint64_t pos = (uint64_t)prefix[wi] + (uint64_t)__popcll(word & ((1ull << bit) - 1));
    if (pos >= k) continue;
    uint4 v = reinterpret_cast<const uint4 *>(res + c)[q];
    if (q == 2) {  // {kind, index, ref} -> {usize, blob, index, gid}
      uint64_t lo = 0;
      if (first) {  // the last layer that starts at or before c (empty layers share a start)
        uint64_t hi = L;
        while (hi - lo > 1) {
          const uint64_t mid = lo + (hi - lo) / 2;
          if (first[mid] <= c) lo = mid; else hi = mid;
        }
      }
      v = make_uint4(chunks[c].length, blob0 + lrank[lo], v.y, gid0 + (uint32_t)pos);
    } else if (q == 3) {  // {blob_index, dict_blob, uoff} -> {uoff, pad}
      v = make_uint4(v.z, v.w, 0, 0);
    }
    reinterpret_cast<uint4 *>(out + pos)[q] = v;
  }
}

}  // namespace

void launch_fold_keep_scan(const ngpu_result *res, const ngpu_chunk *chunks, uint64_t n,
                           uint32_t chunk_size, const uint64_t *lfirst, uint64_t L, uint64_t *words,
                           uint32_t *cnt, uint64_t *sums, uint32_t *lrank, uint64_t *ctr,
                           hipStream_t s) {
  const uint64_t nw = (n + 63) / 64, nt = dict_retire_scan_tiles(n);
  if (n)
    hipLaunchKernelGGL(fold_keep_words, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, res, chunks,
                       n, chunk_size, words, cnt, ctr);
  launch_retire_scan(cnt, nw, sums, s);
  hipLaunchKernelGGL(fold_layer_ranks, dim3(1), dim3(kTileThreads), 0, s, words, cnt, sums + nt, n,
                     lfirst, lfirst ? L : 1, lrank, ctr);
}

void launch_fold_scatter(const ngpu_result *res, const ngpu_chunk *chunks, uint64_t n,
                         const uint64_t *words, const uint32_t *prefix, const uint64_t *lfirst,
                         uint64_t L, const uint32_t *lrank, uint32_t blob0, uint32_t gid0,
                         DictRec *out, uint64_t k, hipStream_t s) {
  if (n == 0 || k == 0) return;
  const uint64_t nw = (n + 63) / 64;
  hipLaunchKernelGGL(fold_scatter, dim3((unsigned)((nw + kFoldWords - 1) / kFoldWords)), dim3(256), 0,
                     s, res, chunks, n, words, prefix, lfirst, lfirst ? L : 1, lrank, blob0, gid0, out,
                     k);
}

}  // namespace ngpu
