// verity.hip — Verity: the dm-verity SHA-256 hash tree of a block image
// (include/nydus_gpu.h, "Verity").
//
// tarfs's `nydus-image export --block --verity` appends this tree to the disk
// image it exports and prints the options that open it (pkg/tarfs/tarfs.go:548,
// docs/tarfs.md:119-145): format 1, no superblock, empty salt, 512-byte data
// blocks, 4096-byte hash blocks.  Here:
//   * verity_leaves: one lane per 512-byte data block -- eight compressions of
//     data (per-lane 16-byte loads, the next 64 bytes in flight during the
//     rounds, as sha256_lane does), then the padding block, which is the same
//     for every lane: its K+W schedule is a compile-time table, so it costs
//     the 64 rounds only.  The digest leaves as two 16-byte stores at
//     level0 + 32 * block, contiguous across lanes.
//   * verity_level: the same with one lane per 4096-byte hash block (64
//     compressions + the padding block of a 32768-bit message); one launch per
//     level above the leaves, and one for the root.
//   Both write zeros to the digest slots between the last digest and the end
//   of the level's last hash block, so every byte of the tree is written and
//   the caller never clears it; lanes past that store nothing.
//   * ngpu_verity_image: the host pipeline (shaped like Check's): reader
//     threads fill one pinned window while the GPU hashes the other into the
//     level-0 region of a tree kept in HBM; the upper levels run after the
//     last window and the tree comes back through the same windows.
// Everything runs on the caller's stream, nothing on the null stream (DESIGN
// §3, "The digest guard").
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "engine_internal.hpp"
#include "sha256_core.hpp"
#include "verity_plan.hpp"

namespace ngpu {
namespace {

// K[t] + W[t] of the one padding block that follows a message of `bits` bits
// when bits is a multiple of 512: 0x80, zeros, the 64-bit length.
struct PadKW {
  uint32_t v[64];
};
constexpr uint32_t crotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
constexpr PadKW pad_kw(uint32_t bits) {
  uint32_t w[64] = {};
  w[0] = 0x80000000u;
  w[15] = bits;
  for (int t = 16; t < 64; ++t) {
    const uint32_t s0 = crotr(w[t - 15], 7) ^ crotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
    const uint32_t s1 = crotr(w[t - 2], 17) ^ crotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
    w[t] = w[t - 16] + s0 + w[t - 7] + s1;
  }
  PadKW r{};
  for (int t = 0; t < 64; ++t) r.v[t] = w[t] + kK[t];
  return r;
}
template <uint32_t BITS>
struct Pad {
  static constexpr PadKW kw = pad_kw(BITS);
};

// The padding block's compression: rounds only (the unrolled loop folds
// K+W into immediates).
template <uint32_t BITS>
__device__ __forceinline__ void sha_pad_block(uint32_t h[8]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
  uint32_t e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    const uint32_t S1 = xor3(rotr32(e, 6), rotr32(e, 11), rotr32(e, 25));
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = hh + Pad<BITS>::kw.v[t] + S1 + ch;
    const uint32_t S0 = xor3(rotr32(a, 2), rotr32(a, 13), rotr32(a, 22));
    const uint32_t mj = (a & b) | (c & (a | b));
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + S0 + mj;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d;
  h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// Lane i < n_in hashes the NB * 64 bytes at in + i * NB * 64 into out + 32 i;
// lane n_in <= i < n_out writes 32 zero bytes there (the tail of the level's
// last hash block); lanes from n_out on do nothing.  `in` is 16-byte aligned.
// vec: out is 16-byte aligned (two 16-byte stores per digest); otherwise byte
// stores -- only a root pointer the caller did not align takes that path.
template <int NB>
__device__ __forceinline__ void verity_hash(const uint8_t *__restrict__ in, uint64_t n_in,
                                            uint8_t *__restrict__ out, uint64_t n_out, bool vec) {
  const uint64_t i = blockIdx.x * 256ull + threadIdx.x;
  if (i >= n_out) return;
  uint8_t *o = out + 32 * i;
  if (i >= n_in) {
    if (vec) {
      reinterpret_cast<uint4 *>(o)[0] = make_uint4(0, 0, 0, 0);
      reinterpret_cast<uint4 *>(o)[1] = make_uint4(0, 0, 0, 0);
    } else {
      for (int k = 0; k < 32; ++k) o[k] = 0;
    }
    return;
  }
  const u32x4 *q = reinterpret_cast<const u32x4 *>(in + i * (uint64_t)(NB * 64));
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  u32x4 pf0 = q[0], pf1 = q[1], pf2 = q[2], pf3 = q[3];
  uint32_t w[16];
  auto take = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = bswap_words(pf0, j); w[4 + j] = bswap_words(pf1, j);
      w[8 + j] = bswap_words(pf2, j); w[12 + j] = bswap_words(pf3, j);
    }
  };
#pragma unroll 1
  for (int b = 1; b < NB; ++b) {
    take();
    q += 4;
    pf0 = q[0]; pf1 = q[1]; pf2 = q[2]; pf3 = q[3];
    sha_block(h, w);
  }
  take();
  sha_block(h, w);
  sha_pad_block<NB * 512>(h);
  if (vec) {
    reinterpret_cast<uint4 *>(o)[0] = make_uint4(bswap(h[0]), bswap(h[1]), bswap(h[2]), bswap(h[3]));
    reinterpret_cast<uint4 *>(o)[1] = make_uint4(bswap(h[4]), bswap(h[5]), bswap(h[6]), bswap(h[7]));
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      o[4 * k] = (uint8_t)(h[k] >> 24); o[4 * k + 1] = (uint8_t)(h[k] >> 16);
      o[4 * k + 2] = (uint8_t)(h[k] >> 8); o[4 * k + 3] = (uint8_t)h[k];
    }
  }
}

__global__ __launch_bounds__(256) void verity_leaves(const uint8_t *__restrict__ in, uint64_t n_in,
                                                     uint8_t *__restrict__ out, uint64_t n_out,
                                                     bool vec) {
  verity_hash<8>(in, n_in, out, n_out, vec);
}

__global__ __launch_bounds__(256) void verity_level(const uint8_t *__restrict__ in, uint64_t n_in,
                                                    uint8_t *__restrict__ out, uint64_t n_out,
                                                    bool vec) {
  verity_hash<64>(in, n_in, out, n_out, vec);
}

constexpr uint64_t kMaxLanes = 0x7FFFFFFFull * 256;  // one launch's grid

// n_in messages at `in` -> n_out digest slots at `out` on s (leaves: 512-byte
// messages; otherwise 4096-byte ones).  1 <= n_in <= n_out <= kMaxLanes.
void launch_verity(bool leaves, const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t n_out,
                   hipStream_t s) {
  const bool vec = ((uintptr_t)out & 15) == 0;
  const dim3 grid((unsigned)((n_out + 255) / 256));
  if (leaves)
    hipLaunchKernelGGL(verity_leaves, grid, dim3(256), 0, s, in, n_in, out, n_out, vec);
  else
    hipLaunchKernelGGL(verity_level, grid, dim3(256), 0, s, in, n_in, out, n_out, vec);
}

// Data blocks [block0, block0 + n) of the image, at d, into the tree's level 0
// (levels == 0: into the root).  last: these are the image's last blocks --
// the zero tail of level 0 is written too.
void enqueue_leaves(const VerityPlan &P, const uint8_t *d, uint64_t block0, uint64_t n, bool last,
                    uint8_t *d_tree, uint8_t *d_root, hipStream_t s) {
  if (P.levels == 0) {
    launch_verity(true, d, 1, d_root, 1, s);
    return;
  }
  uint8_t *out = d_tree + P.first[0] * kVerityHashBlock + kVerityDigest * block0;
  launch_verity(true, d, n, out, last ? P.blocks[0] * kVerityFanout - block0 : n, s);
}

// The levels above level 0, bottom up, then the root.
void enqueue_upper(const VerityPlan &P, uint8_t *d_tree, uint8_t *d_root, hipStream_t s) {
  if (P.levels == 0) return;
  for (uint32_t i = 1; i < P.levels; ++i)
    launch_verity(false, d_tree + P.first[i - 1] * kVerityHashBlock, P.blocks[i - 1],
                  d_tree + P.first[i] * kVerityHashBlock, P.blocks[i] * kVerityFanout, s);
  launch_verity(false, d_tree + P.first[P.levels - 1] * kVerityHashBlock, 1, d_root, 1, s);
}

void info_of(const VerityPlan &P, ngpu_verity_info *out) {
  memset(out, 0, sizeof *out);
  out->data_blocks = P.data_blocks;
  out->hash_offset = P.hash_offset;
  out->tree_bytes = P.tree_bytes;
  out->levels = P.levels;
}

// Everything one ngpu_verity_image call holds, released on every path.  The
// windows are staging slots of the engine (staging_take / staging_give).
struct VerityBufs {
  ngpu_engine *e = nullptr;
  int device = 0;
  hipStream_t s = nullptr;
  ngpu_staging_buf win[2];
  hipEvent_t done[2] = {}, fence = nullptr;
  uint8_t *d_tree = nullptr;  // tree_bytes, then the 32-byte root
  ~VerityBufs() {
    DeviceGuard g(device);
    if (s) (void)hipStreamSynchronize(s);
    for (ngpu_staging_buf &b : win) staging_give(e, b);
    if (d_tree) (void)hipFree(d_tree);
    for (hipEvent_t ev : {done[0], done[1], fence})
      if (ev) (void)hipEventDestroy(ev);
    if (s) (void)hipStreamDestroy(s);
  }
};

bool read_full(ngpu_read_at_fn ra, void *ctx, uint8_t *dst, uint64_t n, uint64_t off) {
  while (n) {
    const int64_t r = ra(ctx, dst, n, off);
    if (r <= 0 || (uint64_t)r > n) return false;
    dst += r;
    off += (uint64_t)r;
    n -= (uint64_t)r;
  }
  return true;
}

constexpr uint64_t kReadPiece = 1ull << 20;  // what one reader thread takes at a time

int verity_image(ngpu_engine *e, ngpu_read_at_fn ra, void *ctx, uint64_t data_bytes,
                 const ngpu_verity_options *opt, ngpu_write_fn w, void *wctx,
                 ngpu_verity_info *info) {
  memset(info, 0, sizeof *info);
  VerityPlan P;
  if (!verity_plan(data_bytes, &P))
    return fail(e, NGPU_EINVAL, "verity: %llu data bytes: not a non-zero multiple of 512 below 2^62",
                (unsigned long long)data_bytes);
  if (P.blocks[0] * kVerityFanout > kMaxLanes)
    return fail(e, NGPU_EINVAL, "verity: %llu data blocks are more than one launch takes",
                (unsigned long long)P.data_blocks);
  ngpu_verity_options o{};
  if (opt) o = *opt;
  if (!o.window_bytes) o.window_bytes = e->cfg.staging_bytes;
  o.window_bytes -= o.window_bytes % kVerityDataBlock;
  if (!o.window_bytes) return fail(e, NGPU_EINVAL, "verity: window below one 512-byte data block");
  if (!o.threads) o.threads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  o.threads = std::min(o.threads, 256u);
  const uint64_t win = std::min(o.window_bytes, data_bytes);
  const uint64_t nwin = data_bytes / win + (data_bytes % win != 0);
  const int nbuf = nwin > 1 ? 2 : 1;

  uint8_t root[32];  // pageable target of an async copy on B.s: declared before B,
                     // whose destructor synchronises the stream on every path
  DeviceGuard dg(e->device);
  VerityBufs B;
  B.e = e;
  B.device = e->device;
  HIP_TRY(e, hipStreamCreateWithFlags(&B.s, hipStreamNonBlocking));
  HIP_TRY(e, hipEventCreateWithFlags(&B.fence, hipEventDisableTiming));
  for (int k = 0; k < nbuf; ++k) {
    HIP_TRY(e, hipEventCreateWithFlags(&B.done[k], hipEventDisableTiming));
    if (!staging_take(e, win, &B.win[k]))
      return fail(e, NGPU_ENOMEM, "verity: two windows of %llu bytes", (unsigned long long)win);
  }
  if (hipMalloc((void **)&B.d_tree, P.tree_bytes + 64) != hipSuccess) {
    (void)hipGetLastError();
    B.d_tree = nullptr;
    return fail(e, NGPU_ENOMEM, "verity: a tree of %llu bytes does not fit the device",
                (unsigned long long)P.tree_bytes);
  }
  uint8_t *d_root = B.d_tree + P.tree_bytes;

  // ---- the image, window by window, into level 0 ---------------------------
  for (uint64_t wi = 0; wi < nwin; ++wi) {
    const int k = (int)(wi % (uint64_t)nbuf);
    if (wi >= (uint64_t)nbuf) HIP_TRY(e, hipEventSynchronize(B.done[k]));
    const uint64_t off = wi * win, n = std::min(win, data_bytes - off);
    uint8_t *h = (uint8_t *)B.win[k].h;
    const uint64_t pieces = (n + kReadPiece - 1) / kReadPiece;
    std::atomic<uint64_t> next{0};
    std::atomic<bool> failed{false};
    auto work = [&]() {
      for (;;) {
        const uint64_t q = next.fetch_add(1, std::memory_order_relaxed);
        if (q >= pieces || failed.load(std::memory_order_relaxed)) return;
        const uint64_t po = q * kReadPiece, pn = std::min(kReadPiece, n - po);
        if (!read_full(ra, ctx, h + po, pn, off + po)) failed.store(true, std::memory_order_relaxed);
      }
    };
    {
      const uint32_t T = (uint32_t)std::min<uint64_t>(o.threads, pieces);
      std::vector<std::thread> pool;
      for (uint32_t t = 1; t < T; ++t) pool.emplace_back(work);
      work();
      for (auto &t : pool) t.join();
    }
    if (failed.load())
      return fail(e, NGPU_EIO, "verity: reading the image at [%llu, %llu) failed",
                  (unsigned long long)off, (unsigned long long)(off + n));
    HIP_TRY(e, hipMemcpyAsync(B.win[k].d, h, n, hipMemcpyHostToDevice, B.s));
    {
      std::lock_guard<std::mutex> g(e->mu);
      enqueue_leaves(P, (const uint8_t *)B.win[k].d, off / kVerityDataBlock, n / kVerityDataBlock,
                     wi + 1 == nwin, B.d_tree, d_root, B.s);
      HIP_TRY(e, hipGetLastError());
    }
    HIP_TRY(e, hipEventRecord(B.done[k], B.s));
  }
  {
    std::lock_guard<std::mutex> g(e->mu);
    enqueue_upper(P, B.d_tree, d_root, B.s);
    HIP_TRY(e, hipGetLastError());
  }
  HIP_TRY(e, hipEventRecord(B.fence, B.s));  // system-scope release before the host's copies
  HIP_TRY(e, hipMemcpyAsync(root, d_root, 32, hipMemcpyDeviceToHost, B.s));

  // ---- the tree back through the pinned windows, in order ------------------
  if (w && P.tree_bytes) {
    const uint64_t nch = P.tree_bytes / win + (P.tree_bytes % win != 0);
    auto issue = [&](uint64_t j) -> int {
      const int k = (int)(j % (uint64_t)nbuf);
      const uint64_t at = j * win;
      HIP_TRY(e, hipMemcpyAsync(B.win[k].h, B.d_tree + at, std::min(win, P.tree_bytes - at),
                                hipMemcpyDeviceToHost, B.s));
      HIP_TRY(e, hipEventRecord(B.done[k], B.s));
      return 0;
    };
    if (int rc = issue(0)) return rc;
    for (uint64_t j = 0; j < nch; ++j) {
      const int k = (int)(j % (uint64_t)nbuf);
      if (nbuf == 2 && j + 1 < nch)
        if (int rc = issue(j + 1)) return rc;
      HIP_TRY(e, hipEventSynchronize(B.done[k]));
      const uint64_t at = j * win;
      if (w(wctx, B.win[k].h, std::min(win, P.tree_bytes - at)))
        return fail(e, NGPU_EIO, "verity: the writer failed at tree byte %llu", (unsigned long long)at);
      if (nbuf == 1 && j + 1 < nch)
        if (int rc = issue(j + 1)) return rc;
    }
  }
  HIP_TRY(e, hipStreamSynchronize(B.s));
  info_of(P, info);
  memcpy(info->root, root, 32);
  return 0;
}

}  // namespace
}  // namespace ngpu

using namespace ngpu;

extern "C" {

int ngpu_verity_layout(uint64_t data_bytes, ngpu_verity_info *out) {
  if (!out) return NGPU_EINVAL;
  VerityPlan P;
  const bool ok = verity_plan(data_bytes, &P);
  info_of(P, out);
  return ok ? 0 : NGPU_EINVAL;
}

int ngpu_verity_device(ngpu_engine *e, const void *d_data, uint64_t data_bytes, void *d_tree,
                       void *d_root, void *stream) {
  if (!e || !d_data || !d_root) return NGPU_EINVAL;
  VerityPlan P;
  if (!verity_plan(data_bytes, &P))
    return fail(e, NGPU_EINVAL, "verity: %llu data bytes: not a non-zero multiple of 512 below 2^62",
                (unsigned long long)data_bytes);
  if (P.tree_bytes && !d_tree) return fail(e, NGPU_EINVAL, "verity: no tree buffer");
  if (((uintptr_t)d_data & 15) || ((uintptr_t)d_tree & 15))
    return fail(e, NGPU_EINVAL, "verity: d_data and d_tree must be 16-byte aligned");
  if (P.blocks[0] * kVerityFanout > kMaxLanes)
    return fail(e, NGPU_EINVAL, "verity: %llu data blocks are more than one launch takes",
                (unsigned long long)P.data_blocks);
  std::lock_guard<std::mutex> g(e->mu);
  DeviceGuard dg(e->device);
  hipStream_t s = (hipStream_t)stream;
  enqueue_leaves(P, (const uint8_t *)d_data, 0, P.data_blocks, true, (uint8_t *)d_tree,
                 (uint8_t *)d_root, s);
  enqueue_upper(P, (uint8_t *)d_tree, (uint8_t *)d_root, s);
  HIP_TRY(e, hipGetLastError());
  return 0;
}

int ngpu_verity_image(ngpu_engine *e, ngpu_read_at_fn ra, void *ctx, uint64_t data_bytes,
                      const ngpu_verity_options *opt, ngpu_write_fn w, void *wctx,
                      ngpu_verity_info *info) {
  if (!e || !ra || !info) return NGPU_EINVAL;
  const int rc = guarded([&]() -> int { return verity_image(e, ra, ctx, data_bytes, opt, w, wctx, info); });
  if (rc == NGPU_ENOMEM) fail(e, rc, "verity: out of memory");
  return rc;
}

}  // extern "C"
