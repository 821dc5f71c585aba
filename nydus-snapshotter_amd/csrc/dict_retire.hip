// dict_retire.hip — the device side of dict retire (dict.hip, ngpu_dict_retire):
// an ordered stream compaction of a dict's 64-B records by inner blob.
//
//   1. dict_keep_words   one keep bit per record (its blob is not in the retire
//                        bitmap), one ballot per wave64 -> keep word + popcount
//   2. retire_tile_sums  \  exclusive scan of the popcounts, reduce-then-scan in
//      retire_scan_sums   > three launches: no workgroup waits for another
//      retire_scan_apply /  (the dedup scan's look-back is not used here)
//   3. dict_compact      survivor i -> out[prefix[i / 64] + popc(word below i)],
//                        blob through the remap table, gid = the new position
//
// The table of the result is then built by the existing launch_dict_build.
// Step 2 has a launcher of its own (launch_retire_scan): dict fold
// (dict_fold.hip) scans the popcounts of its own keep words with it.
// Roofline: HBM-bound.  Pass 1 touches every record's line for 4 bytes of it,
// pass 3 reads the kept lines whole and writes them: 2 reads + 1 write of the
// records against a fork's 1 + 1 (DESIGN.md §3 "Dict retire").
#include "common.hpp"

namespace ngpu {
namespace {

// Lanes past m vote 0, so every word of (m + 63) / 64 is written whole.
// A record whose blob is not a blob of the dict (ngpu_dict_create_device takes
// the caller's word for n_blobs) is kept as it is: the bitmap has no bit for it.
__global__ __launch_bounds__(256) void dict_keep_words(const DictRec *__restrict__ rec, uint64_t m,
                                                       const uint32_t *__restrict__ bitmap,
                                                       uint32_t n_blobs,
                                                       uint64_t *__restrict__ words,
                                                       uint32_t *__restrict__ cnt) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  bool keep = false;
  if (i < m) {
    const uint32_t b = rec[i].blob;
    keep = b >= n_blobs || !((bitmap[b >> 5] >> (b & 31)) & 1);
  }
  const uint64_t w = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && i < m) {  // i < m: word i / 64 exists
    words[i >> 6] = w;
    cnt[i >> 6] = (uint32_t)__popcll(w);
  }
}

// Tile t of the scan: counts [t * kRetireScanTile, (t + 1) * kRetireScanTile).
__global__ __launch_bounds__(kTileThreads) void retire_tile_sums(const uint32_t *__restrict__ cnt,
                                                                 uint64_t nw,
                                                                 uint64_t *__restrict__ sums) {
  const uint64_t j = blockIdx.x * (uint64_t)kRetireScanTile + threadIdx.x;
  uint64_t tot;
  (void)block_exclusive_scan(j < nw ? cnt[j] : 0, &tot);
  if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// One workgroup: sums[0, nt) -> exclusive prefixes in place, the total to sums[nt].
__global__ __launch_bounds__(kTileThreads) void retire_scan_sums(uint64_t *__restrict__ sums,
                                                                 uint64_t nt) {
  uint64_t carry = 0;
  for (uint64_t a = 0; a < nt; a += kTileThreads) {  // (uniform trip count: barriers inside)
    const uint64_t j = a + threadIdx.x;
    const uint64_t v = j < nt ? sums[j] : 0;
    uint64_t tot;
    const uint64_t x = block_exclusive_scan(v, &tot);
    if (j < nt) sums[j] = carry + x;
    carry += tot;
  }
  if (threadIdx.x == 0) sums[nt] = carry;
}

// cnt[j] -> the number of survivors before word j (below 2^32: ids are u32).
__global__ __launch_bounds__(kTileThreads) void retire_scan_apply(uint32_t *__restrict__ cnt,
                                                                  uint64_t nw,
                                                                  const uint64_t *__restrict__ sums) {
  const uint64_t j = blockIdx.x * (uint64_t)kRetireScanTile + threadIdx.x;
  uint64_t tot;
  const uint64_t x = block_exclusive_scan(j < nw ? cnt[j] : 0, &tot);
  if (j < nw) cnt[j] = (uint32_t)(sums[blockIdx.x] + x);
}

// Four lanes per record, 16 B each: a wave reads 16 records as 1 KiB of whole
// lines and writes its survivors back to back.  A workgroup takes
// kCompactWords keep words (256 records), one per pass; the passes are
// independent, so their loads are in flight together.  Lane q == 2 of a record
// holds {usize, blob, index, gid}.  Reads are bounded by m, writes by s.
constexpr int kCompactWords = 4;

__global__ __launch_bounds__(256) void dict_compact(const DictRec *__restrict__ rec, uint64_t m,
                                                    const uint64_t *__restrict__ words,
                                                    const uint32_t *__restrict__ prefix,
                                                    const uint32_t *__restrict__ remap,
                                                    uint32_t n_blobs, DictRec *__restrict__ out,
                                                    uint64_t s) {
  const uint64_t nw = (m + 63) / 64;
  const uint32_t bit = threadIdx.x >> 2, q = threadIdx.x & 3;
#pragma unroll
  for (int k = 0; k < kCompactWords; ++k) {
    const uint64_t wi = blockIdx.x * (uint64_t)kCompactWords + k;
    if (wi >= nw) break;
    const uint64_t word = words[wi];
    const uint64_t r = wi * 64 + bit;
    if (!((word >> bit) & 1) || r >= m) continue;
    const uint64_t dst = (uint64_t)prefix[wi] + (uint64_t)__popcll(word & ((1ull << bit) - 1));
    if (dst >= s) continue;
    uint4 v = reinterpret_cast<const uint4 *>(rec + r)[q];
    if (q == 2) {
      if (v.y < n_blobs) v.y = remap[v.y];
      v.w = (uint32_t)dst;
    }
    reinterpret_cast<uint4 *>(out + dst)[q] = v;
  }
}

}  // namespace

void launch_dict_keep_scan(const DictRec *rec, uint64_t m, const uint32_t *bitmap, uint32_t n_blobs,
                           uint64_t *words, uint32_t *cnt, uint64_t *sums, hipStream_t s) {
  if (m)
    hipLaunchKernelGGL(dict_keep_words, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, rec, m,
                       bitmap, n_blobs, words, cnt);
  launch_retire_scan(cnt, (m + 63) / 64, sums, s);
}

void launch_retire_scan(uint32_t *cnt, uint64_t nw, uint64_t *sums, hipStream_t s) {
  const uint64_t nt = (nw + kRetireScanTile - 1) / kRetireScanTile;
  if (nw)
    hipLaunchKernelGGL(retire_tile_sums, dim3((unsigned)nt), dim3(kTileThreads), 0, s, cnt, nw, sums);
  hipLaunchKernelGGL(retire_scan_sums, dim3(1), dim3(kTileThreads), 0, s, sums, nt);
  if (nw)
    hipLaunchKernelGGL(retire_scan_apply, dim3((unsigned)nt), dim3(kTileThreads), 0, s, cnt, nw, sums);
}

void launch_dict_compact(const DictRec *rec, uint64_t m, const uint64_t *words,
                         const uint32_t *prefix, const uint32_t *remap, uint32_t n_blobs,
                         DictRec *out, uint64_t n_out, hipStream_t s) {
  if (m == 0 || n_out == 0) return;
  const uint64_t nw = (m + 63) / 64;
  hipLaunchKernelGGL(dict_compact, dim3((unsigned)((nw + kCompactWords - 1) / kCompactWords)),
                     dim3(256), 0, s, rec, m, words, prefix, remap, n_blobs, out, n_out);
}

}  // namespace ngpu
