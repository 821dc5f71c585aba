// dict_grow_plan.hpp — the bookkeeping of dict extend (dict.hip,
// ngpu_dict_extend): whether k more records go onto the storage a handle sits
// on (share: k record writes and k table inserts, nothing copied) or onto a new,
// larger storage (fork: copy the base's records, rebuild the table).  Checked
// on the CPU by tests/cpp/dict_grow_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h>.
#pragma once
#include <stdint.h>

namespace ngpu {

constexpr uint64_t kDictMaxEntries = 0xFFFFFFFFull;  // entry ids are u32, 0xFFFFFFFF = miss

struct DictGrowPlan {
  bool ok = false;     // false: base_m + k entries are more than a dict holds
  bool share = false;  // append in place on the base's storage
  // the storage the result sits on (share: the base's own, unchanged)
  uint64_t rec_cap = 0, table_cap = 0;
};

inline uint64_t dict_grow_pow2(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// The table capacity dict_alloc gives an m-entry dict: load <= 1/2.
inline uint64_t dict_table_cap(uint64_t m) { return dict_grow_pow2(2 * m + 16); }

// base_m: the handle's entries; used: the highest record slot ever reserved on
// its storage; rec_cap / table_cap: the storage's capacities; k: records to add.
// Share needs the handle to be the newest on its storage (nobody reserved slots
// past it), room for the records, and the table load dict_alloc guarantees
// (2 (m + k) + 16 <= table_cap), so probe chains get no longer than in a dict
// created at that size.  A fork allocates (m + k) + max(k, (m + k) / 2) record
// slots: at least half as many again, so n one-row extends fork O(log_1.5 n)
// times and copy O(n) records in total, and no storage holds more than 1.5x
// the records of its largest handle's (or 2x right after a fork of k >= m).
inline DictGrowPlan dict_grow_plan(uint64_t base_m, uint64_t used, uint64_t rec_cap,
                                   uint64_t table_cap, uint64_t k) {
  DictGrowPlan p;
  if (base_m >= kDictMaxEntries || k >= kDictMaxEntries - base_m) return p;  // m + k >= 0xFFFFFFFF
  p.ok = true;
  const uint64_t n = base_m + k;
  if (base_m == used && n <= rec_cap && 2 * n + 16 <= table_cap) {
    p.share = true;
    p.rec_cap = rec_cap;
    p.table_cap = table_cap;
    return p;
  }
  uint64_t want = n + (k > n / 2 ? k : n / 2);
  if (want > kDictMaxEntries - 1) want = kDictMaxEntries - 1;  // no slot past the last valid id
  p.rec_cap = want;
  p.table_cap = dict_table_cap(want);
  return p;
}

}  // namespace ngpu
