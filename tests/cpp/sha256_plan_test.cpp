// The SHA-256 kernel selection rule (csrc/sha256_plan.hpp) on the CPU: the pick
// of every admitted variant around the wave size and the two auto thresholds,
// the launch shape of every pick, and the `mixed` heuristic at its edges.
// Stand-alone: g++ -fsanitize=address,undefined; prints "ok ..." (no GPU).
//
// With arguments, quadruples `variant n len chunk_size`: prints one line
//   pick <variant> <n> <len> <chunk_size> <mixed 0|1> <name> <chunks_per_wg> <threads> <grid>
// per quadruple (tests/test_sha_shapes.py ties its Python mirror to the header
// with these), then "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "sha256_plan.hpp"

using namespace ngpu;

static int fails = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++fails;                                            \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                       \
      fprintf(stderr, "\n");                              \
    }                                                     \
  } while (0)

static std::string name_of(const ShaPick &p) {
  char b[16];
  sha_pick_name(p, b, sizeof b);
  return b;
}

// The rule written out as a table, not as the header's arithmetic.
static std::string expected_name(int variant, uint64_t n, bool mixed) {
  if (variant < 0) {
    if (n <= 16384) return mixed ? "pair<2,U>" : "pair<2,M>";
    if (n <= 32768) return "pair<4,M>";
    return "lane";
  }
  switch (variant) {
    case 0: return "split";
    case 2: return "lane";
    case 4: return mixed ? "pair<1,U>" : "pair<1,M>";
    case 5: return "pair<4,M>";
    default: return mixed ? "pair<2,U>" : "pair<2,M>";  // 1, and today's meaning of 3 and 6
  }
}

struct Shape { uint32_t chunks, threads; };
static Shape expected_shape(const std::string &name) {
  if (name == "split") return {64, 128};
  if (name == "lane") return {256, 256};
  if (name.rfind("pair<1", 0) == 0) return {32, 128};
  if (name.rfind("pair<2", 0) == 0) return {64, 256};
  return {128, 512};  // pair<4,M>
}

static int check_rule() {
  const int variants[] = {-1, 0, 1, 2, 4, 5, 3, 6};
  const uint64_t ns[] = {1, 31, 32, 33, 16384, 16385, 32768, 32769};
  int picks = 0;
  for (int v : variants)
    for (uint64_t n : ns)
      for (int mixed = 0; mixed < 2; ++mixed) {
        const ShaPick p = sha_pick(v, n, mixed != 0);
        const std::string want = expected_name(v, n, mixed != 0), got = name_of(p);
        CHECK(got == want, "variant %d n %llu mixed %d: %s, want %s", v, (unsigned long long)n, mixed,
              got.c_str(), want.c_str());
        const Shape s = expected_shape(want);
        CHECK(p.chunks_per_wg == s.chunks && p.threads == s.threads, "variant %d n %llu: %u chunks %u threads",
              v, (unsigned long long)n, p.chunks_per_wg, p.threads);
        CHECK(p.grid >= 1 && (p.grid - 1) * p.chunks_per_wg < n && n <= p.grid * p.chunks_per_wg,
              "variant %d n %llu: grid %llu x %u", v, (unsigned long long)n, (unsigned long long)p.grid,
              p.chunks_per_wg);
        CHECK((p.kernel == ShaKernel::Pair) == (p.R != 0), "R %d", p.R);
        if (p.kernel == ShaKernel::Pair) {
          CHECK(p.chunks_per_wg == 32u * p.R && p.threads == 128u * p.R, "R %d", p.R);
          CHECK(p.R != 4 || !p.uniform, "pair<4> is always M");
          CHECK(p.R == 4 || p.uniform == (mixed != 0), "U follows mixed for R = 1, 2");
        } else {
          CHECK(!p.uniform, "U is a pair property");
        }
        CHECK(p.grid <= 0xFFFFFFFFull, "grid fits a dim3");
        ++picks;
      }
  CHECK(sha_pick(-1, 0, true).grid == 0, "n = 0 launches nothing");
  CHECK(kShaPair2MaxChunks == 16384 && kShaPair4MaxChunks == 32768, "thresholds");

  // sha_mixed: n % 32, with a buffer that is full either way
  for (uint32_t cs : {0x1000u, 0x1000000u}) {
    for (uint64_t n : {32ull, 64ull, 960ull}) {
      const uint64_t full = n * cs;
      CHECK(!sha_mixed(n, full, cs), "n %% 32 == 0, full buffer");
      CHECK(sha_mixed(n + 1, (n + 1) * cs, cs), "n %% 32 == 1");
      CHECK(sha_mixed(n + 31, (n + 31) * cs, cs), "n %% 32 == 31");
      // the 15/16 threshold: n * cs / 16 * 15 exactly (n * cs is a multiple of 16)
      const uint64_t thr = full / 16 * 15;
      CHECK(thr == n * (uint64_t)cs * 15 / 16, "threshold arithmetic");
      CHECK(sha_mixed(n, thr - 1, cs), "one byte below 15/16, cs %#x n %llu", cs, (unsigned long long)n);
      CHECK(!sha_mixed(n, thr, cs), "at 15/16, cs %#x n %llu", cs, (unsigned long long)n);
      CHECK(!sha_mixed(n, thr + 1, cs), "one byte above 15/16, cs %#x n %llu", cs, (unsigned long long)n);
    }
  }
  // the two buffer sizes the GPU matrix pads its layers to
  CHECK(!sha_mixed(960, 3686400, 0x1000) && sha_mixed(960, 3686399, 0x1000), "layer E threshold");
  CHECK(!sha_mixed(224, 13762560, 0x10000) && sha_mixed(224, 13762559, 0x10000), "layer R threshold");
  CHECK(sha_mixed(32, 0, 0x1000) && !sha_mixed(0, 0, 0x1000), "empty buffer");
  // no 64-bit overflow at the largest admitted chunk size and a 2^32-chunk call
  CHECK(sha_mixed(1ull << 32, (1ull << 56) / 16 * 15 - 1, 0x1000000) &&
            !sha_mixed(1ull << 32, (1ull << 56) / 16 * 15, 0x1000000), "2^56-byte threshold");
  return picks;
}

int main(int argc, char **argv) {
  if (argc > 1) {
    if ((argc - 1) % 4) {
      fprintf(stderr, "usage: %s [variant n len chunk_size]...\n", argv[0]);
      return 2;
    }
    for (int i = 1; i + 3 < argc; i += 4) {
      const int v = (int)strtol(argv[i], nullptr, 10);
      const uint64_t n = strtoull(argv[i + 1], nullptr, 10), len = strtoull(argv[i + 2], nullptr, 10);
      const uint32_t cs = (uint32_t)strtoul(argv[i + 3], nullptr, 10);
      const bool mixed = sha_mixed(n, len, cs);
      const ShaPick p = sha_pick(v, n, mixed);
      printf("pick %d %llu %llu %u %d %s %u %u %llu\n", v, (unsigned long long)n, (unsigned long long)len,
             cs, mixed ? 1 : 0, name_of(p).c_str(), p.chunks_per_wg, p.threads, (unsigned long long)p.grid);
    }
    printf("ok\n");
    return 0;
  }
  const int picks = check_rule();
  if (fails) {
    fprintf(stderr, "%d check(s) failed\n", fails);
    return 1;
  }
  printf("ok %d picks, mixed edges at chunk sizes 0x1000 and 0x1000000\n", picks);
  return 0;
}
