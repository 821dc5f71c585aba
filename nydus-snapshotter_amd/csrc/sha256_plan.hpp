// sha256_plan.hpp — which SHA-256 digest kernel a call runs (sha256.hip,
// launch_sha256) and with what launch shape: the `mixed` heuristic of the
// digest stage (engine.hip, enqueue_digest), the auto rule over the chunk
// count, the forced variants of ngpu_config.flags bits 11..13, and a name for
// the pick (the engine's path string and its error messages carry it).
// Checked on the CPU by tests/cpp/sha256_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h> and <stdio.h>.
#pragma once
#include <stdint.h>
#include <stdio.h>

namespace ngpu {

// Auto rule (same-box sweep, profiles/r2/sha_variants_lane_r2sl.jsonl, GB/s):
//  * <= 16384 chunks (one 64-chunk workgroup per CU): two lanes per chunk,
//    each round wave alone on its SIMD; 16384 x 1 MiB: pair 786, lane 385.
//  * <= 32768 chunks: two lanes per chunk, four groups per workgroup (one
//    workgroup per CU, a round and a schedule wave on each SIMD); 32768 x
//    512 KiB: 1343, against 950 for two 2-group workgroups per CU.
//  * more: one lane per chunk, every wave doing its own schedule;
//    65536 x 256 KiB lane 1512 / pair-4 1342, 262144 x 64 KiB 1657 / split 1190.
constexpr uint64_t kShaPair2MaxChunks = 256ull * 64;   // 16384
constexpr uint64_t kShaPair4MaxChunks = 256ull * 128;  // 32768

// Mixed lengths unless the data averages >= 15/16 of a full chunk per chunk
// and fills every 32-chunk wave (a raw stream cut at chunk_size, C3); tar
// layers and batches mix file-sized chunks with full ones.  `len` is the
// length of the data buffer, not the sum of the chunk lengths.
inline bool sha_mixed(uint64_t n, uint64_t len, uint32_t chunk_size) {
  return n % 32 != 0 || len < n * (uint64_t)chunk_size / 16 * 15;
}

enum class ShaKernel { Split, Lane, Pair };

struct ShaPick {
  ShaKernel kernel = ShaKernel::Split;
  int R = 0;                   // pair: groups of 32 chunks per workgroup (1, 2, 4); else 0
  bool uniform = false;        // pair: the wave-uniform round loop (U), else the masked one (M)
  uint32_t chunks_per_wg = 0;
  uint32_t threads = 0;        // per workgroup
  uint64_t grid = 0;           // workgroups; 0 when n == 0 (nothing is launched)
};

// variant: -1 auto, else ngpu_config.flags bits 11..13 minus one: 0 split,
// 1 pair (two groups per workgroup), 2 lane, 4 pair with one group, 5 pair
// with four groups; any other value >= 1 runs as 1 (ngpu_create admits none).
// mixed: sha_mixed() of the call.  The round waves of pair<1> and pair<2> run
// wave-uniform for mixed calls (a long chain among short neighbours ran
// 25-45 % slower masked); pair<4> has the masked loop only.
inline ShaPick sha_pick(int variant, uint64_t n, bool mixed) {
  if (variant < 0) variant = n <= kShaPair2MaxChunks ? 1 : n <= kShaPair4MaxChunks ? 5 : 2;
  ShaPick p;
  if (variant == 0) {
    p.kernel = ShaKernel::Split;
    p.chunks_per_wg = 64;
    p.threads = 128;
  } else if (variant == 2) {
    p.kernel = ShaKernel::Lane;
    p.chunks_per_wg = 256;
    p.threads = 256;
  } else {
    p.kernel = ShaKernel::Pair;
    p.R = variant == 4 ? 1 : variant == 5 ? 4 : 2;
    p.uniform = p.R != 4 && mixed;
    p.chunks_per_wg = 32u * (uint32_t)p.R;
    p.threads = 128u * (uint32_t)p.R;
  }
  p.grid = (n + p.chunks_per_wg - 1) / p.chunks_per_wg;
  return p;
}

// "split", "lane", "pair<2,U>", "pair<4,M>", ...; at most 9 characters.
inline void sha_pick_name(const ShaPick &p, char *buf, size_t cap) {
  if (p.kernel == ShaKernel::Pair)
    snprintf(buf, cap, "pair<%d,%c>", p.R, p.uniform ? 'U' : 'M');
  else
    snprintf(buf, cap, "%s", p.kernel == ShaKernel::Lane ? "lane" : "split");
}

}  // namespace ngpu
