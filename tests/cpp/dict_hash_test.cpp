// dict_hash_test.cpp — csrc/dict_hash.hpp on the CPU (tests/test_dict_hash.py;
// g++, no GPU).  One run prints three sections:
//
//   owners   for W = 1..64: both forms of owner_of against the ABI's formula
//            ((d0 << 8 | d1) * W) >> 16 on every 16-bit prefix (checked here),
//            then "owners W p1 p2 ..." -- the prefixes at which the owner steps
//   digest   "digest <hex> tag s63 s1023 s131071": tag and home slot of a
//            fixed list of digests at three table masks
//   chain    "chain W owner hit miss longest": 60,000 random rows of one owner
//            inserted by sequential linear probing into dict_table_cap(m)
//            slots; mean slots read per hit, mean slots read per miss over
//            20,000 fresh digests of the same owner, longest hit chain
//
// and "ok" as its last line.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "dict_grow_plan.hpp"
#include "dict_hash.hpp"

using namespace ngpu;

static int g_fail = 0;
#define CHECK(c, ...)                       \
  do {                                      \
    if (!(c)) {                             \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fprintf(stderr, "\n");                \
      ++g_fail;                             \
    }                                       \
  } while (0)

static uint64_t g_state;
static uint64_t splitmix() {
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void words_of(const uint8_t d[32], uint32_t w[8]) {
  for (int i = 0; i < 8; ++i)
    w[i] = (uint32_t)d[4 * i] | (uint32_t)d[4 * i + 1] << 8 | (uint32_t)d[4 * i + 2] << 16 |
           (uint32_t)d[4 * i + 3] << 24;
}

static void owners() {
  for (uint32_t W = 1; W <= 64; ++W) {
    printf("owners %u", W);
    uint32_t prev = 0;
    for (uint32_t hi = 0; hi < 65536; ++hi) {
      const uint8_t d[2] = {(uint8_t)(hi >> 8), (uint8_t)hi};
      // word 0 as a kernel loads it (little-endian), with junk in bytes 2, 3
      const uint32_t w0 = (uint32_t)d[0] | (uint32_t)d[1] << 8 | (hi * 2654435761u & 0xFFFF0000u);
      const uint32_t want = (uint32_t)(((uint64_t)hi * W) >> 16);
      CHECK(owner_of(d, W) == want, "byte form: W %u prefix %#x", W, hi);
      CHECK(owner_of(w0, W) == want, "word form: W %u prefix %#x", W, hi);
      CHECK(want < W, "owner %u of %u", want, W);
      if (want != prev) printf(" %u", hi);
      prev = want;
    }
    printf("\n");
  }
}

static void print_digest(const uint8_t d[32]) {
  uint32_t w[8];
  words_of(d, w);
  printf("digest ");
  for (int i = 0; i < 32; ++i) printf("%02x", d[i]);
  const uint64_t b = digest_bucket(w);
  printf(" %u %llu %llu %llu\n", digest_tag(w), (unsigned long long)(b & 63),
         (unsigned long long)(b & 1023), (unsigned long long)(b & ((1u << 17) - 1)));
}

static void digests() {
  g_state = 0x6469676573747321ull;
  uint8_t d[32];
  for (int k = 0; k < 48; ++k) {
    for (int i = 0; i < 4; ++i) {
      const uint64_t r = splitmix();
      memcpy(d + 8 * i, &r, 8);
    }
    if (k % 8 == 1) memset(d + 8, 0xFF, 4);                    // tag 0xFFFFFFFF -> 0xFFFFFFFE
    if (k % 8 == 2) d[8] = 0xFE, memset(d + 9, 0xFF, 3);       // tag 0xFFFFFFFE stays
    if (k % 8 == 3) memset(d + 1, 0, 7);                       // only byte 0 of the bucket words
    if (k % 8 == 4) memset(d, 0, 7);                           // only byte 7
    if (k == 5) memset(d, 0xFF, 32);
    if (k == 6) memset(d, 0, 32), d[4] = 1;                    // word 1 alone
    print_digest(d);
  }
}

// A digest's bucket words (all the table model needs) of owner `o` of W.
static uint64_t fresh_words(uint32_t W, uint32_t o) {
  for (;;) {
    const uint64_t r = splitmix();
    uint8_t d[8];
    memcpy(d, &r, 8);
    if (owner_of(d, W) == o) return r;
  }
}

static uint64_t home(uint64_t words, uint64_t mask) {
  const uint32_t w[3] = {(uint32_t)words, (uint32_t)(words >> 32), 0};
  return digest_bucket(w) & mask;
}

static void chain(uint32_t W, uint32_t o) {
  constexpr uint64_t kRows = 60000, kMiss = 20000, kEmptySlot = ~0ull;
  const uint64_t cap = dict_table_cap(kRows), mask = cap - 1;
  g_state = 0x636861696E000000ull + W * 131 + o;
  std::vector<uint64_t> table(cap, kEmptySlot), rows(kRows);
  for (uint64_t i = 0; i < kRows; ++i) {
    rows[i] = fresh_words(W, o);
    uint64_t p = home(rows[i], mask);
    while (table[p] != kEmptySlot) p = (p + 1) & mask;
    table[p] = i;
  }
  uint64_t hit = 0, miss = 0, longest = 0;
  for (uint64_t i = 0; i < kRows; ++i) {
    uint64_t k = 1;
    for (uint64_t p = home(rows[i], mask); table[p] != i; p = (p + 1) & mask) ++k;
    hit += k;
    longest = k > longest ? k : longest;
  }
  for (uint64_t i = 0; i < kMiss; ++i) {
    uint64_t k = 1;  // the empty slot that ends the walk is read too
    for (uint64_t p = home(fresh_words(W, o), mask); table[p] != kEmptySlot; p = (p + 1) & mask) ++k;
    miss += k;
  }
  printf("chain %u %u %.4f %.4f %llu\n", W, o, (double)hit / kRows, (double)miss / kMiss,
         (unsigned long long)longest);
}

int main() {
  owners();
  digests();
  CHECK(dict_table_cap(60000) == 131072, "table of 60,000 rows");
  chain(1, 0);  // the reference: unconstrained digests
  chain(2, 1);
  chain(3, 1);
  chain(8, 3);
  chain(64, 17);
  if (g_fail) return 1;
  printf("ok\n");
  return 0;
}
