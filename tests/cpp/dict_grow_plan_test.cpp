// dict_grow_plan_test.cpp — dict extend's share / fork decision
// (csrc/dict_grow_plan.hpp) on the CPU, run by tests/test_dict_grow_plan.py
// under ASan/UBSan.  usage: dict_grow_plan_test -> "ok <checks>".
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "dict_grow_plan.hpp"

using namespace ngpu;

static int checks = 0;
#define REQUIRE(c)                                   \
  do {                                               \
    ++checks;                                        \
    if (!(c)) {                                      \
      printf("FAILED %s (line %d)\n", #c, __LINE__); \
      return 1;                                      \
    }                                                \
  } while (0)

int main() {
  // a storage of 1000 record slots and a 4096-slot table, 600 in use by the tip
  {
    const DictGrowPlan p = dict_grow_plan(600, 600, 1000, 4096, 100);
    REQUIRE(p.ok && p.share && p.rec_cap == 1000 && p.table_cap == 4096);
  }
  // not the newest handle on its storage: fork, whatever room there is
  for (uint64_t used : {601ull, 700ull, 1000ull}) {
    const DictGrowPlan p = dict_grow_plan(600, used, 1000, 4096, 1);
    REQUIRE(p.ok && !p.share);
    REQUIRE(p.rec_cap == 601 + 300 && p.table_cap == 2048);  // want = 601 + max(1, 300)
  }
  // used below base_m cannot happen on a live storage; it is no share either
  REQUIRE(!dict_grow_plan(600, 599, 1000, 4096, 1).share);
  // k that exactly fills / overfills the record capacity (the table has room)
  REQUIRE(dict_grow_plan(600, 600, 1000, 4096, 400).share);
  REQUIRE(!dict_grow_plan(600, 600, 1000, 4096, 401).share);
  // k that exactly fills / overfills the table: 2 (m + k) + 16 <= table_cap
  REQUIRE(dict_grow_plan(600, 600, 5000, 4096, 1440).share);   // 2 * 2040 + 16 = 4096
  REQUIRE(!dict_grow_plan(600, 600, 5000, 4096, 1441).share);  // 4098
  // k = 0: a share when the handle is the tip, else a fork of its own size
  {
    DictGrowPlan p = dict_grow_plan(600, 600, 1000, 4096, 0);
    REQUIRE(p.ok && p.share);
    p = dict_grow_plan(600, 601, 1000, 4096, 0);
    REQUIRE(p.ok && !p.share && p.rec_cap == 900 && p.table_cap == 2048);
  }
  // m = 0 on what ngpu_dict_create(n = 0) allocates (no record slot, 16 table slots)
  {
    DictGrowPlan p = dict_grow_plan(0, 0, 0, 16, 0);
    REQUIRE(p.ok && p.share);
    p = dict_grow_plan(0, 0, 0, 16, 1);
    REQUIRE(p.ok && !p.share && p.rec_cap == 2 && p.table_cap == 32);  // 1 + max(1, 0)
    p = dict_grow_plan(0, 0, 0, 16, 100);
    REQUIRE(p.ok && !p.share && p.rec_cap == 200 && p.table_cap == 512);  // 2 * 200 + 16 = 416
    p = dict_grow_plan(0, 0, 200, 512, 200);  // an empty handle on a roomy storage
    REQUIRE(p.ok && p.share);
  }
  // what ngpu_dict_create allocates for m entries never has room: its first extend forks
  for (uint64_t m : {1ull, 7ull, 8ull, 4096ull, 1000000ull}) {
    const DictGrowPlan p = dict_grow_plan(m, m, m, dict_table_cap(m), 1);
    REQUIRE(p.ok && !p.share);
    REQUIRE(p.rec_cap == (m + 1) + ((m + 1) / 2 > 1 ? (m + 1) / 2 : 1));
    REQUIRE(p.table_cap == dict_grow_pow2(2 * p.rec_cap + 16));
    // and the fork has room for everything up to its record capacity
    REQUIRE(dict_grow_plan(m + 1, m + 1, p.rec_cap, p.table_cap, p.rec_cap - m - 1).share);
    REQUIRE(!dict_grow_plan(m + 1, m + 1, p.rec_cap, p.table_cap, p.rec_cap - m).share);
  }
  // k > (m + k) / 2: the fork doubles
  {
    const DictGrowPlan p = dict_grow_plan(100, 100, 100, 256, 300);
    REQUIRE(p.ok && !p.share && p.rec_cap == 700 && p.table_cap == 2048);
  }
  // the entry limit: ids are u32 and 0xFFFFFFFF is the miss
  {
    DictGrowPlan p = dict_grow_plan(0xFFFFFFF0ull, 0xFFFFFFF0ull, 0xFFFFFFF0ull, 1ull << 34, 0xE);
    REQUIRE(p.ok && !p.share);  // m + k = 0xFFFFFFFE
    REQUIRE(p.rec_cap == 0xFFFFFFFEull && p.table_cap == 1ull << 34);
    p = dict_grow_plan(0xFFFFFFF0ull, 0xFFFFFFF0ull, 0xFFFFFFF0ull, 1ull << 34, 0xF);
    REQUIRE(!p.ok);  // 0xFFFFFFFF
    REQUIRE(!dict_grow_plan(0, 0, 0, 16, 0xFFFFFFFFull).ok);
    REQUIRE(dict_grow_plan(0, 0, 0, 16, 0xFFFFFFFEull).ok);
    REQUIRE(!dict_grow_plan(1, 1, 1, 32, ~0ull).ok);  // no wrap-around
    REQUIRE(!dict_grow_plan(~0ull, ~0ull, ~0ull, 32, 1).ok);
    REQUIRE(dict_grow_plan(0xFFFFFFFEull, 0xFFFFFFFEull, 0xFFFFFFFEull, 1ull << 34, 0).share);
  }
  // amortisation: 1,000 one-row extends of an empty dict.  Each fork leaves
  // want = n + max(1, n / 2) slots, so the forks happen at n = 1, 3, 5, 8, 13,
  // 20, 31, 47, 71, 107, 161, 242, 364, 547, 821: 15 of them (log_1.5 1000 =
  // 17.04 bounds the count), and they copy fewer than 3 x 1000 records in all.
  {
    uint64_t m = 0, rec_cap = 0, table_cap = 16, forks = 0, copied = 0, max_cap = 0;
    const uint64_t at[15] = {1, 3, 5, 8, 13, 20, 31, 47, 71, 107, 161, 242, 364, 547, 821};
    for (int i = 0; i < 1000; ++i) {
      const DictGrowPlan p = dict_grow_plan(m, m, rec_cap, table_cap, 1);
      REQUIRE(p.ok);
      if (!p.share) {
        REQUIRE(forks < 15 && m + 1 == at[forks]);
        ++forks;
        copied += m;
        rec_cap = p.rec_cap;
        table_cap = p.table_cap;
      }
      ++m;
      REQUIRE(m <= rec_cap && 2 * m + 16 <= table_cap);
      if (m >= 2) REQUIRE(2 * rec_cap <= 3 * m + 2);  // at most half as many slots again
      max_cap = rec_cap > max_cap ? rec_cap : max_cap;
    }
    REQUIRE(forks == 15);
    REQUIRE(copied < 3000);
    REQUIRE(max_cap == 1231);
  }
  printf("ok %d\n", checks);
  return 0;
}
