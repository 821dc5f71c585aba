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
//   * ngpu_verity_image: the host pipeline (window_bufs.hpp, host_window.hpp):
//     the GPU hashes each window into the level-0 region of a tree kept in
//     HBM; the upper levels run after the last window and the tree comes back
//     through the same windows.
//   * Verify (ngpu_verity_verify_*): an image against its STORED tree.  Every
//     stored block is compared with its stored parent slot, so no level waits
//     for another: verity_verify_data (one lane per data block against the
//     stored level 0) and verity_verify_tree (one lane per stored hash block,
//     all levels in one launch, against the parent slot or the trusted root;
//     the spare area of a level's last block ORed on the way).  A verdict is
//     one bit: __ballot per wave64 -> bitmap word -> popcount into a counter,
//     as check_digests does.  The geometry of a stored block is
//     verity_verify_plan.hpp's, for the kernel and the host's findings alike.
//     ngpu_verity_verify_image reads the tree into HBM first, then the data
//     window by window; only bitmaps and counts come back.
// Everything runs on the caller's stream, nothing on the null stream (DESIGN
// §3, "The digest guard").
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "host_window.hpp"
#include "sha256_core.hpp"
#include "verity_plan.hpp"
#include "verity_verify_plan.hpp"
#include "window_bufs.hpp"

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

// SHA-256 of the NB * 64 bytes at q into h (the working words, big-endian
// values): per-lane 16-byte loads, the next 64 bytes in flight during the
// rounds, then the constant padding block.  SPARE (the verify kernel on a
// stored hash block): returns the OR of every word from byte 32 * used on,
// taken from the registers the loads fill; 0 otherwise.  The verify kernels'
// copy of verity_hash's hashing: folding the two into one body changed the
// schedule and register count of verity_leaves / verity_level, whose measured
// code stays as it is.
template <int NB, bool SPARE>
__device__ __forceinline__ uint32_t verity_digest(const u32x4 *__restrict__ q, uint32_t h[8],
                                                  uint32_t used) {
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
  u32x4 pf0 = q[0], pf1 = q[1], pf2 = q[2], pf3 = q[3];
  uint32_t w[16], spare = 0;
  auto take = [&](uint32_t b) {  // 64-byte block b = digest slots 2 b and 2 b + 1
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[j] = bswap_words(pf0, j); w[4 + j] = bswap_words(pf1, j);
      w[8 + j] = bswap_words(pf2, j); w[12 + j] = bswap_words(pf3, j);
    }
    if constexpr (SPARE) {
      const u32x4 lo = pf0 | pf1, hi = pf2 | pf3;
      spare |= 2 * b >= used ? lo.x | lo.y | lo.z | lo.w : 0u;
      spare |= 2 * b + 1 >= used ? hi.x | hi.y | hi.z | hi.w : 0u;
    }
  };
#pragma unroll 1
  for (int b = 1; b < NB; ++b) {
    take((uint32_t)b - 1);
    q += 4;
    pf0 = q[0]; pf1 = q[1]; pf2 = q[2]; pf3 = q[3];
    sha_block(h, w);
  }
  take(NB - 1);
  sha_block(h, w);
  sha_pad_block<NB * 512>(h);
  return spare;
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

// ---- Verify: the image against its stored tree ------------------------------
// The trusted root as the eight words a lane would load from its 32 bytes; a
// kernel argument, so nothing is allocated for it.
struct VerityRoot {
  uint32_t w[8];
};

// h (big-endian values) against 32 stored bytes loaded as two 16-byte words.
__device__ __forceinline__ bool verity_differs(const uint32_t h[8], u32x4 a, u32x4 b) {
  return ((bswap(h[0]) ^ a.x) | (bswap(h[1]) ^ a.y) | (bswap(h[2]) ^ a.z) | (bswap(h[3]) ^ a.w) |
          (bswap(h[4]) ^ b.x) | (bswap(h[5]) ^ b.y) | (bswap(h[6]) ^ b.z) | (bswap(h[7]) ^ b.w)) != 0;
}

// The verdicts of a wave64: the ballot is bitmap word k / 64 for the wave's
// first lane k (256 % 64 == 0), stored whole -- zero words and the zero tail
// bits of lanes past n too, which must reach the ballot (they vote 0); a wave
// wholly past n stores nothing.  A non-zero word adds its popcount with one
// atomicAdd, so a clean image issues none.
__device__ __forceinline__ void verity_verdict(bool bad, uint64_t k, uint64_t n,
                                               uint64_t *__restrict__ bitmap,
                                               unsigned long long *__restrict__ count) {
  const uint64_t word = __ballot(bad);
  if ((threadIdx.x & 63u) == 0 && k < n) {
    bitmap[k >> 6] = word;
    if (word) atomicAdd(count, (unsigned long long)__popcll(word));
  }
}

// Lane k < n hashes the 512-byte data block at data + 512 k (verity_leaves'
// work) and compares it with the stored 32 bytes at stored + 32 k, contiguous
// across lanes; stored == nullptr (one data block, no tree): with the root.
__global__ __launch_bounds__(256) void verity_verify_data(const uint8_t *__restrict__ data, uint64_t n,
                                                          const uint8_t *__restrict__ stored,
                                                          VerityRoot root, uint64_t *__restrict__ bitmap,
                                                          unsigned long long *__restrict__ count) {
  const uint64_t k = blockIdx.x * 256ull + threadIdx.x;
  bool bad = false;
  if (k < n) {
    uint32_t h[8];
    verity_digest<8, false>(reinterpret_cast<const u32x4 *>(data + k * kVerityDataBlock), h, 0);
    u32x4 a = {root.w[0], root.w[1], root.w[2], root.w[3]};
    u32x4 b = {root.w[4], root.w[5], root.w[6], root.w[7]};
    if (stored) {
      const u32x4 *s = reinterpret_cast<const u32x4 *>(stored + kVerityDigest * k);
      a = s[0];
      b = s[1];
    }
    bad = verity_differs(h, a, b);
  }
  verity_verdict(bad, k, n, bitmap, count);
}

// Lane t < G.tree_blocks hashes stored hash block t (verity_level's work) and
// compares it with its stored parent slot, or the root for t == 0: every level
// in one launch, and as every lane runs the same 65 compressions whatever its
// level, a wave that holds two levels does not diverge.  A level's last block
// also ORs its words past its last digest; non-zero sets bit `level` of
// counts[1].
__global__ __launch_bounds__(256) void verity_verify_tree(const uint8_t *__restrict__ tree, VerityGeom G,
                                                          VerityRoot root, uint64_t *__restrict__ bitmap,
                                                          unsigned long long *__restrict__ counts) {
  const uint64_t t = blockIdx.x * 256ull + threadIdx.x;
  bool bad = false;
  if (t < G.tree_blocks) {
    const VerityBlockLoc at = verity_locate(G, t);
    uint32_t h[8];
    const uint32_t spare = verity_digest<64, true>(
        reinterpret_cast<const u32x4 *>(tree + t * kVerityHashBlock), h, at.used);
    u32x4 a = {root.w[0], root.w[1], root.w[2], root.w[3]};
    u32x4 b = {root.w[4], root.w[5], root.w[6], root.w[7]};
    if (at.parent_off != kVerityNoParent) {
      const u32x4 *s = reinterpret_cast<const u32x4 *>(tree + at.parent_off);
      a = s[0];
      b = s[1];
    }
    bad = verity_differs(h, a, b);
    if (spare) atomicOr(&counts[1], 1ull << at.level);
  }
  verity_verdict(bad, t, G.tree_blocks, bitmap, &counts[0]);
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

VerityRoot root_words(const uint8_t root[32]) {
  VerityRoot r;
  memcpy(r.w, root, 32);
  return r;
}

// The plan of an image one launch can take, or NGPU_EINVAL.
int checked_plan(ngpu_engine *e, uint64_t data_bytes, VerityPlan *P) {
  if (!verity_plan(data_bytes, P))
    return fail(e, NGPU_EINVAL, "verity: %llu data bytes: not a non-zero multiple of 512 below 2^62",
                (unsigned long long)data_bytes);
  if (P->blocks[0] * kVerityFanout > kMaxLanes)
    return fail(e, NGPU_EINVAL, "verity: %llu data blocks are more than one launch takes",
                (unsigned long long)P->data_blocks);
  return 0;
}

// Every stored hash block of the tree at d_tree: counts zeroed on s, then one
// launch (none without a tree).  The caller holds e->mu.
int enqueue_verify_tree(ngpu_engine *e, const VerityPlan &P, const uint8_t *d_tree, const uint8_t root[32],
                        uint64_t *d_bitmap, uint64_t *d_counts, hipStream_t s) {
  // on the caller's stream, never the null stream ("The digest guard")
  HIP_TRY(e, hipMemsetAsync(d_counts, 0, 2 * sizeof(uint64_t), s));
  if (!P.tree_blocks) return 0;
  hipLaunchKernelGGL(verity_verify_tree, dim3((unsigned)((P.tree_blocks + 255) / 256)), dim3(256), 0, s,
                     d_tree, verity_geom(P), root_words(root), d_bitmap, (unsigned long long *)d_counts);
  HIP_TRY(e, hipGetLastError());
  return 0;
}

// Data blocks [block0, block0 + n) at d against the stored level 0 of d_tree
// (levels == 0: against the root).  block0 + n <= P.data_blocks, n <= kMaxLanes.
int enqueue_verify_data(ngpu_engine *e, const VerityPlan &P, const uint8_t *d, uint64_t block0, uint64_t n,
                        const uint8_t *d_tree, const uint8_t root[32], uint64_t *d_bitmap,
                        uint64_t *d_count, hipStream_t s) {
  HIP_TRY(e, hipMemsetAsync(d_count, 0, sizeof(uint64_t), s));
  if (!n) return 0;
  const uint8_t *stored =
      P.levels ? d_tree + P.first[0] * kVerityHashBlock + kVerityDigest * block0 : nullptr;
  hipLaunchKernelGGL(verity_verify_data, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, n, stored,
                     root_words(root), d_bitmap, (unsigned long long *)d_count);
  HIP_TRY(e, hipGetLastError());
  return 0;
}

constexpr uint64_t kReadPiece = 1ull << 20;  // what one reader thread takes at a time

// The n bytes at `off` of the reader into h, in pieces, on up to `threads`
// threads (the caller's among them).
bool read_window(ngpu_read_at_fn ra, void *ctx, uint8_t *h, uint64_t n, uint64_t off, uint32_t threads) {
  std::atomic<bool> failed{false};
  run_indexed(threads, (n + kReadPiece - 1) / kReadPiece, [&](uint64_t q) {
    if (failed.load(std::memory_order_relaxed)) return;
    const uint64_t po = q * kReadPiece, pn = std::min(kReadPiece, n - po);
    if (!read_exact(ra, ctx, h + po, pn, off + po)) failed.store(true, std::memory_order_relaxed);
  });
  return !failed.load();
}

// opt with its defaults filled in; false: a window below one data block.
bool verity_options(ngpu_engine *e, const ngpu_verity_options *opt, ngpu_verity_options *o) {
  *o = ngpu_verity_options{};
  if (opt) *o = *opt;
  if (!o->window_bytes) o->window_bytes = e->cfg.staging_bytes;
  o->window_bytes -= o->window_bytes % kVerityDataBlock;
  if (!o->window_bytes) return false;
  o->threads = host_threads(o->threads);
  return true;
}

int verity_image(ngpu_engine *e, ngpu_read_at_fn ra, void *ctx, uint64_t data_bytes,
                 const ngpu_verity_options *opt, ngpu_write_fn w, void *wctx,
                 ngpu_verity_info *info) {
  memset(info, 0, sizeof *info);
  VerityPlan P;
  if (int rc = checked_plan(e, data_bytes, &P)) return rc;
  ngpu_verity_options o;
  if (!verity_options(e, opt, &o)) return fail(e, NGPU_EINVAL, "verity: window below one 512-byte data block");
  const uint64_t win = std::min(o.window_bytes, data_bytes);
  const uint64_t nwin = data_bytes / win + (data_bytes % win != 0);
  const int nbuf = nwin > 1 ? 2 : 1;

  uint8_t root[32];  // pageable target of an async copy on B.s: declared before B,
                     // whose destructor synchronises the stream on every path
  DeviceGuard dg(e->device);
  WindowBufs B(e);
  if (int rc = B.open(nbuf, win, "verity")) return rc;
  uint8_t *d_tree = nullptr;  // tree_bytes, then the 32-byte root
  if (!B.dmalloc(&d_tree, P.tree_bytes + 64))
    return fail(e, NGPU_ENOMEM, "verity: a tree of %llu bytes does not fit the device",
                (unsigned long long)P.tree_bytes);
  uint8_t *d_root = d_tree + P.tree_bytes;

  // ---- the image, window by window, into level 0 ---------------------------
  for (uint64_t wi = 0; wi < nwin; ++wi) {
    const int k = (int)(wi % (uint64_t)nbuf);
    if (wi >= (uint64_t)nbuf) HIP_TRY(e, hipEventSynchronize(B.done[k]));
    const uint64_t off = wi * win, n = std::min(win, data_bytes - off);
    uint8_t *h = (uint8_t *)B.win[k].h;
    if (!read_window(ra, ctx, h, n, off, o.threads))
      return fail(e, NGPU_EIO, "verity: reading the image at [%llu, %llu) failed",
                  (unsigned long long)off, (unsigned long long)(off + n));
    HIP_TRY(e, hipMemcpyAsync(B.win[k].d, h, n, hipMemcpyHostToDevice, B.s));
    {
      std::lock_guard<std::mutex> g(e->mu);
      enqueue_leaves(P, (const uint8_t *)B.win[k].d, off / kVerityDataBlock, n / kVerityDataBlock,
                     wi + 1 == nwin, d_tree, d_root, B.s);
      HIP_TRY(e, hipGetLastError());
    }
    HIP_TRY(e, hipEventRecord(B.done[k], B.s));
  }
  {
    std::lock_guard<std::mutex> g(e->mu);
    enqueue_upper(P, d_tree, d_root, B.s);
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
      HIP_TRY(e, hipMemcpyAsync(B.win[k].h, d_tree + at, std::min(win, P.tree_bytes - at),
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

int verity_verify_image(ngpu_engine *e, ngpu_read_at_fn ra, void *ctx, uint64_t data_bytes,
                        uint64_t hash_offset, const uint8_t root[32], const ngpu_verity_options *opt,
                        ngpu_verity_report *rep, ngpu_verity_bad *bad, uint64_t bad_cap) {
  memset(rep, 0, sizeof *rep);
  VerityPlan P;
  if (int rc = checked_plan(e, data_bytes, &P)) return rc;
  if (hash_offset < data_bytes || hash_offset + P.tree_bytes < hash_offset)
    return fail(e, NGPU_EINVAL, "verity: a tree of %llu bytes at %llu does not follow %llu data bytes",
                (unsigned long long)P.tree_bytes, (unsigned long long)hash_offset,
                (unsigned long long)data_bytes);
  ngpu_verity_options o;
  if (!verity_options(e, opt, &o)) return fail(e, NGPU_EINVAL, "verity: window below one 512-byte data block");
  const VerityGeom G = verity_geom(P);
  const uint64_t win = std::min(o.window_bytes, data_bytes);
  const uint64_t nwin = data_bytes / win + (data_bytes % win != 0);
  const uint64_t ntree = P.tree_bytes / win + (P.tree_bytes % win != 0);  // the tree goes through the windows first
  const int nbuf = ntree + nwin > 1 ? 2 : 1;
  // the verdict words, on the device behind the tree and pinned on the host:
  // the tree's two counts and bitmap, then each window's count and bitmap
  const uint64_t tw = (P.tree_blocks + 63) / 64, ww = (win / kVerityDataBlock + 63) / 64;
  const uint64_t at[2] = {2 + tw, 2 + tw + 1 + ww}, words = 2 + tw + (uint64_t)nbuf * (1 + ww);

  DeviceGuard dg(e->device);
  WindowBufs B(e);
  if (int rc = B.open(nbuf, win, "verity")) return rc;
  uint8_t *d_tree = nullptr;  // tree_bytes, then the verdict words
  uint64_t *h_res = nullptr;  // the verdict words on the host, pinned
  if (!B.dmalloc(&d_tree, P.tree_bytes + words * 8))
    return fail(e, NGPU_ENOMEM, "verity: a tree of %llu bytes does not fit the device",
                (unsigned long long)P.tree_bytes);
  if (!B.hmalloc(&h_res, words * 8))
    return fail(e, NGPU_ENOMEM, "verity: %llu pinned verdict bytes", (unsigned long long)(words * 8));
  uint64_t *d_res = (uint64_t *)(d_tree + P.tree_bytes);

  uint64_t listed = 0;
  auto add = [&](uint32_t reason, uint32_t level, uint64_t block, uint64_t lo, uint64_t hi, uint64_t off) {
    if (listed < bad_cap) bad[listed++] = ngpu_verity_bad{reason, level, block, lo, hi, off};
    return listed < bad_cap;
  };
  // The tree's findings, top first; a level's spare area belongs to its last
  // block, so it follows that block's own entry and ends the level.
  bool tree_seen = false;
  auto harvest_tree = [&]() {
    if (tree_seen) return;
    tree_seen = true;
    rep->bad_hash = h_res[0];
    rep->bad_spare = (uint64_t)__builtin_popcountll(h_res[1]);
    for (uint32_t l = P.levels; l-- > 0;) {
      if (rep->bad_hash && listed < bad_cap)
        each_set_bit(h_res + 2, P.first[l], P.first[l] + P.blocks[l], [&](uint64_t t) {
          const VerityBlockLoc b = verity_locate(G, t);
          return add(NGPU_VERITY_BAD_HASH, b.level, t, b.first_data, b.last_data,
                     hash_offset + t * kVerityHashBlock);
        });
      if (h_res[1] >> l & 1) {
        const uint64_t t = P.first[l] + P.blocks[l] - 1;
        const VerityBlockLoc b = verity_locate(G, t);
        add(NGPU_VERITY_BAD_SPARE, l, t, b.first_data, b.last_data, hash_offset + t * kVerityHashBlock);
      }
    }
  };
  // What window k holds verdicts of (n == 0: nothing), read once its `done`
  // event or the whole stream has been waited for.
  struct {
    uint64_t block0 = 0, n = 0;
  } held[2];
  auto harvest = [&](int k) {
    if (!held[k].n) return;
    harvest_tree();  // enqueued before any window: it has landed too
    const uint64_t *r = h_res + at[k];
    rep->bad_data += r[0];
    if (r[0] && listed < bad_cap)  // the bitmap is scanned only when the count says so
      each_set_bit(r + 1, 0, held[k].n, [&](uint64_t i) {
        const uint64_t b = held[k].block0 + i;
        return add(NGPU_VERITY_BAD_DATA, 0, b, b, b, b * kVerityDataBlock);
      });
    held[k].n = 0;
  };
  // The next n bytes of the file into the next pinned window.
  uint64_t fills = 0;
  auto fill = [&](uint64_t off, uint64_t n, int *k) -> int {
    *k = (int)(fills % (uint64_t)nbuf);
    if (fills >= (uint64_t)nbuf) {
      HIP_TRY(e, hipEventSynchronize(B.done[*k]));
      harvest(*k);
    }
    ++fills;
    if (!read_window(ra, ctx, (uint8_t *)B.win[*k].h, n, off, o.threads))
      return fail(e, NGPU_EIO, "verity: reading the image at [%llu, %llu) failed", (unsigned long long)off,
                  (unsigned long long)(off + n));
    return 0;
  };

  // ---- the stored tree into HBM, then all of its blocks in one launch ------
  for (uint64_t j = 0; j < ntree; ++j) {
    const uint64_t off = j * win, n = std::min(win, P.tree_bytes - off);
    int k;
    if (int rc = fill(hash_offset + off, n, &k)) return rc;
    HIP_TRY(e, hipMemcpyAsync(d_tree + off, B.win[k].h, n, hipMemcpyHostToDevice, B.s));
    HIP_TRY(e, hipEventRecord(B.done[k], B.s));
  }
  {
    std::lock_guard<std::mutex> g(e->mu);
    if (int rc = enqueue_verify_tree(e, P, d_tree, root, d_res + 2, d_res, B.s)) return rc;
  }
  HIP_TRY(e, hipEventRecord(B.fence, B.s));  // system-scope release before the host's copy
  HIP_TRY(e, hipMemcpyAsync(h_res, d_res, (2 + tw) * 8, hipMemcpyDeviceToHost, B.s));

  // ---- the image, window by window, against the tree in HBM ----------------
  for (uint64_t wi = 0; wi < nwin; ++wi) {
    const uint64_t off = wi * win, n = std::min(win, data_bytes - off), nb = n / kVerityDataBlock;
    int k;
    if (int rc = fill(off, n, &k)) return rc;
    HIP_TRY(e, hipMemcpyAsync(B.win[k].d, B.win[k].h, n, hipMemcpyHostToDevice, B.s));
    {
      std::lock_guard<std::mutex> g(e->mu);
      if (int rc = enqueue_verify_data(e, P, (const uint8_t *)B.win[k].d, off / kVerityDataBlock, nb,
                                       d_tree, root, d_res + at[k] + 1, d_res + at[k], B.s))
        return rc;
    }
    if (int rc = B.verdict_back(k, h_res + at[k], d_res + at[k], (1 + (nb + 63) / 64) * 8)) return rc;
    held[k].block0 = off / kVerityDataBlock;
    held[k].n = nb;
  }
  HIP_TRY(e, hipStreamSynchronize(B.s));
  for (uint64_t j = fills - std::min<uint64_t>(fills, (uint64_t)nbuf); j < fills; ++j)
    harvest((int)(j % (uint64_t)nbuf));  // the older window first
  harvest_tree();
  rep->data_blocks = P.data_blocks;
  rep->tree_blocks = P.tree_blocks;
  rep->levels = P.levels;
  rep->bad = rep->bad_data + rep->bad_hash + rep->bad_spare;
  rep->bytes = data_bytes + P.tree_bytes;
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
  return guarded_entry(e, "verity",
                       [&]() -> int { return verity_image(e, ra, ctx, data_bytes, opt, w, wctx, info); });
}

int ngpu_verity_verify_tree_device(ngpu_engine *e, uint64_t data_bytes, const void *d_tree,
                                   const uint8_t root[32], uint64_t *d_tree_bitmap, uint64_t *d_counts,
                                   void *stream) {
  if (!e || !root || !d_counts) return NGPU_EINVAL;
  VerityPlan P;
  if (int rc = checked_plan(e, data_bytes, &P)) return rc;
  if (P.tree_bytes && (!d_tree || !d_tree_bitmap)) return fail(e, NGPU_EINVAL, "verity: no tree or no bitmap");
  if (((uintptr_t)d_tree & 15) || ((uintptr_t)d_tree_bitmap & 7) || ((uintptr_t)d_counts & 7))
    return fail(e, NGPU_EINVAL, "verity: d_tree must be 16-byte, the bitmap and counts 8-byte aligned");
  std::lock_guard<std::mutex> g(e->mu);
  DeviceGuard dg(e->device);
  return enqueue_verify_tree(e, P, (const uint8_t *)d_tree, root, d_tree_bitmap, d_counts,
                             (hipStream_t)stream);
}

int ngpu_verity_verify_data_device(ngpu_engine *e, const void *d_data, uint64_t first_block,
                                   uint64_t n_blocks, uint64_t data_bytes, const void *d_tree,
                                   const uint8_t root[32], uint64_t *d_bitmap, uint64_t *d_count,
                                   void *stream) {
  if (!e || !root || !d_count) return NGPU_EINVAL;
  VerityPlan P;
  if (int rc = checked_plan(e, data_bytes, &P)) return rc;
  if (first_block > P.data_blocks || n_blocks > P.data_blocks - first_block)
    return fail(e, NGPU_EINVAL, "verity: blocks [%llu, +%llu) are not within the image's %llu",
                (unsigned long long)first_block, (unsigned long long)n_blocks,
                (unsigned long long)P.data_blocks);
  if (n_blocks &&(!d_data || !d_bitmap || (P.tree_bytes && !d_tree)))
    return fail(e, NGPU_EINVAL, "verity: no data, no tree or no bitmap");
  if (((uintptr_t)d_data & 15) || ((uintptr_t)d_tree & 15) || ((uintptr_t)d_bitmap & 7) ||
      ((uintptr_t)d_count & 7))
    return fail(e, NGPU_EINVAL,
                "verity: d_data and d_tree must be 16-byte, the bitmap and count 8-byte aligned");
  std::lock_guard<std::mutex> g(e->mu);
  DeviceGuard dg(e->device);
  return enqueue_verify_data(e, P, (const uint8_t *)d_data, first_block, n_blocks, (const uint8_t *)d_tree,
                             root, d_bitmap, d_count, (hipStream_t)stream);
}

int ngpu_verity_verify_image(ngpu_engine *e, ngpu_read_at_fn ra, void *ctx, uint64_t data_bytes,
                             uint64_t hash_offset, const uint8_t root[32], const ngpu_verity_options *opt,
                             ngpu_verity_report *report, ngpu_verity_bad *bad, uint64_t bad_cap) {
  if (!e || !ra || !root || !report || (bad_cap && !bad)) return NGPU_EINVAL;
  return guarded_entry(e, "verity", [&]() -> int {
    return verity_verify_image(e, ra, ctx, data_bytes, hash_offset, root, opt, report, bad, bad_cap);
  });
}

}  // extern "C"
