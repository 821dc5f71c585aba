// dict_hash.hpp — the hash rules of the chunk dict and the intra tables, stated
// once: tag, home slot and node owner of a digest.  Callable from kernels and
// from host code; plain C++ when hipcc is not the compiler, so a CPU test
// (tests/cpp/dict_hash_test.cpp) runs the very functions the kernels run.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define NGPU_HD __host__ __device__ __forceinline__
#else
#define NGPU_HD inline
#endif

namespace ngpu {

// 64-bit hash-table slot: tag (digest word 2) in the high half, id in the low.
// Equal digests give equal tags, so an atomic min over a slot keeps the
// smallest id ("first in stream / table order wins").  Word 2 == 0xFFFFFFFF
// is stored as 0xFFFFFFFE so that no slot equals kEmpty: two digests that
// differ only in that word then share a tag and are told apart by the full
// compare (the tagff case of tests/dedup_cases.py).
NGPU_HD uint32_t digest_tag(const uint32_t *w) {
  const uint32_t t = w[2];
  return t == 0xFFFFFFFFu ? 0xFFFFFFFEu : t;
}

// Home slot = digest_bucket(w) & mask.  The low k bits of a product depend
// only on the low k bits of its factors, i.e. on the first digest bytes --
// the bytes owner_of partitions on, so a node part's rows would home on
// 256 / W of the 256 slot residues and chain (DESIGN.md §3 "dict probe").
// Folding the product's high half into the low one makes every masked bit
// depend on all eight bytes.
NGPU_HD uint64_t digest_bucket(const uint32_t *w) {
  const uint64_t x = ((uint64_t)w[1] << 32 | w[0]) * 0x9E3779B97F4A7C15ull;
  return x ^ (x >> 32);
}

// Owner of a digest in a W-part node dict (ABI: include/nydus_gpu.h, and
// nydus_gpu/dist.py's owner_of): its first two bytes as a big-endian 16-bit
// prefix, scaled to [0, W).  Word form: w0 = digest word 0 (little-endian).
NGPU_HD uint32_t owner_of(uint32_t w0, uint32_t W) {
  const uint32_t hi = (w0 & 0xFF) << 8 | ((w0 >> 8) & 0xFF);  // digest bytes 0, 1
  return (uint32_t)(((uint64_t)hi * W) >> 16);
}
NGPU_HD uint32_t owner_of(const uint8_t *d, uint32_t W) {
  return (uint32_t)((((uint64_t)d[0] << 8 | d[1]) * W) >> 16);
}

}  // namespace ngpu
