// node_fold.hip — the device side of node dict fold (node.hip,
// ngpu_node_dict_fold) that dict fold (dict_fold.hip) does not already have:
// counting a part's NEW chunks per owner, and splitting its staged 64-B rows by
// owner without changing their order.
//
//   fold_owner_counts  a lane per chunk: owner_of(digest word 0) of the NEW ones
//                      into a per-workgroup LDS histogram (W <= 64 bins), one
//                      atomicAdd per non-empty bin into the part's W counters
//   split_tile_hist    tile t (256 staged rows) -> cnt[o * T + t]
//   launch_retire_scan cnt -> exclusive prefixes in place (dict_retire.hip's
//                      three launches, unchanged); owner-major, so base[o * T + t]
//                      is where tile t's rows of owner o go
//   split_scatter      row r -> out[base[o * T + t] + rank], rank = earlier rows
//                      of the tile with the same owner: a wave64 finds its lanes
//                      of one owner with six ballots, the waves' counts meet in
//                      LDS; the rows then move four lanes x 16 B each
//
// Five launches whatever W is.  The split is stable: a part's rows must reach
// their owner in global table order, since the table insert keeps the smallest
// local position of a digest.  (ngpu_route_digests leaves the order inside a
// segment open and is not used here.)  Roofline: launch-bound at a layer's size;
// the rows are read once whole plus 4 B of each line for the histogram and
// written once (DESIGN.md §3 "Node dict fold").
#include "common.hpp"
#include "node_fold_plan.hpp"

namespace ngpu {
namespace {

constexpr uint32_t kBins = kNodeFoldMaxParts;
static_assert(kNodeSplitTile == 256 && kBins == 64, "one row per lane of a 256-lane workgroup");

__global__ __launch_bounds__(256) void fold_owner_counts(const ngpu_result *__restrict__ res,
                                                         uint64_t n, uint32_t W,
                                                         uint32_t *__restrict__ cnt) {
  __shared__ uint32_t hist[kBins];
  if (threadIdx.x < kBins) hist[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i < n && res[i].kind == NGPU_NEW)
    atomicAdd(&hist[owner_of(*reinterpret_cast<const uint32_t *>(res[i].digest), W)], 1u);
  __syncthreads();
  if (threadIdx.x < W && hist[threadIdx.x]) atomicAdd(cnt + threadIdx.x, hist[threadIdx.x]);
}

__global__ __launch_bounds__(256) void split_tile_hist(const DictRec *__restrict__ rows, uint64_t k,
                                                       uint32_t W, uint64_t T,
                                                       uint32_t *__restrict__ cnt) {
  __shared__ uint32_t hist[kBins];
  if (threadIdx.x < kBins) hist[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t r = blockIdx.x * kNodeSplitTile + threadIdx.x;
  if (r < k) atomicAdd(&hist[owner_of(rows[r].digest[0], W)], 1u);
  __syncthreads();
  if (threadIdx.x < W) cnt[(uint64_t)threadIdx.x * T + blockIdx.x] = hist[threadIdx.x];
}

// base: the scanned counts.  Reads are bounded by k; a destination is below k
// because the counts it comes from are those of these very rows (checked again:
// a row whose destination is not is dropped, never written elsewhere).
__global__ __launch_bounds__(256) void split_scatter(const DictRec *__restrict__ rows, uint64_t k,
                                                     uint32_t W, uint64_t T,
                                                     const uint32_t *__restrict__ base,
                                                     DictRec *__restrict__ out) {
  __shared__ uint32_t wcnt[4][kBins];  // per wave: its rows of each owner
  __shared__ uint32_t dest[kNodeSplitTile];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 4 * kBins) (&wcnt[0][0])[tid] = 0;
  __syncthreads();
  const uint64_t r0 = blockIdx.x * kNodeSplitTile, r = r0 + tid;
  const bool live = r < k;
  const uint32_t o = live ? owner_of(rows[r].digest[0], W) : 0;
  // the lanes of this wave with the same owner
  uint64_t same = __ballot(live);
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const uint64_t v = __ballot((o >> b) & 1);
    same &= ((o >> b) & 1) ? v : ~v;
  }
  const uint32_t below = (uint32_t)__popcll(same & ((1ull << lane) - 1));
  if (live && below == 0) wcnt[wave][o] = (uint32_t)__popcll(same);  // the owner's first lane
  __syncthreads();
  uint32_t d = kNone;
  if (live) {
    uint32_t rank = below;
    for (uint32_t w = 0; w < wave; ++w) rank += wcnt[w][o];
    d = base[(uint64_t)o * T + blockIdx.x] + rank;
  }
  dest[tid] = d;
  __syncthreads();
  const uint32_t q = tid & 3;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t row = j * 64 + (tid >> 2);
    const uint32_t to = dest[row];
    if (r0 + row >= k || to >= k) continue;
    reinterpret_cast<uint4 *>(out + to)[q] = reinterpret_cast<const uint4 *>(rows + r0 + row)[q];
  }
}

}  // namespace

void launch_fold_owner_counts(const ngpu_result *res, uint64_t n, uint32_t W, uint32_t *cnt,
                              hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(fold_owner_counts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, res, n, W,
                     cnt);
}

uint64_t node_split_tiles(uint64_t k) { return (k + kNodeSplitTile - 1) / kNodeSplitTile; }

void launch_node_split(const DictRec *rows, uint64_t k, uint32_t W, uint32_t *cnt, uint64_t *sums,
                       DictRec *out, hipStream_t s) {
  if (k == 0) return;
  const uint64_t T = node_split_tiles(k);
  hipLaunchKernelGGL(split_tile_hist, dim3((unsigned)T), dim3(256), 0, s, rows, k, W, T, cnt);
  launch_retire_scan(cnt, (uint64_t)W * T, sums, s);
  hipLaunchKernelGGL(split_scatter, dim3((unsigned)T), dim3(256), 0, s, rows, k, W, T, cnt, out);
}

}  // namespace ngpu
