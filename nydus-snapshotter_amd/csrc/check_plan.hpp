// check_plan.hpp — the bookkeeping of Check (check.hip, ngpu_check_image):
// how a layer's chunk records are cut into staging windows, and how the
// verdict kernel's bitmap is read back.  Checked on the CPU by
// tests/cpp/check_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h> and <vector>.
#pragma once
#include <stdint.h>

#include <vector>

#include "host_window.hpp"

namespace ngpu {

// One chunk record to check: its uncompressed size (what it takes in a
// window), the supplied blob it is read from and its ordinal among the
// bootstrap's records (kept so that failures are reported in record order).
struct CheckItem {
  uint32_t usize = 0;
  uint32_t blob = 0;
  uint64_t order = 0;
};

// A window of whole chunks: items [first, first + count) of the list, `bytes`
// of the window used (the end of its last chunk).
struct CheckWindow {
  uint64_t first = 0, count = 0, bytes = 0;
};

constexpr uint64_t kCheckAlign = 16;  // every chunk starts on a 16-B boundary (16-B loads)

// Cut `n` items, in list order, into windows of at most `window` bytes.  Every
// item lands in exactly one window at a 16-byte aligned offset (off[i], relative
// to its window) and is never split; a window is closed when the next item
// would pass its end.  false: an item is empty or larger than the window
// (nothing is planned then; the caller bounds sizes first).
inline bool check_plan_windows(const CheckItem *it, uint64_t n, uint64_t window,
                               std::vector<CheckWindow> *wins, std::vector<uint64_t> *off) {
  wins->clear();
  off->assign(n, 0);
  for (uint64_t i = 0; i < n; ++i)
    if (it[i].usize == 0 || it[i].usize > window) return false;
  CheckWindow w;
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t at = (w.bytes + kCheckAlign - 1) / kCheckAlign * kCheckAlign;
    if (w.count && (at > window || it[i].usize > window - at)) {
      wins->push_back(w);
      w = CheckWindow{i, 0, 0};
      at = 0;
    }
    (*off)[i] = at;
    w.bytes = at + it[i].usize;
    ++w.count;
  }
  if (w.count) wins->push_back(w);
  return true;
}

// The set bits of an n-record bitmap (bit i % 64 of word i / 64), ascending:
// at most `cap` ordinals into out; returns the total number of set bits among
// the first n.  Bits past n in the last word are ignored.
inline uint64_t check_decode_bitmap(const uint64_t *words, uint64_t n, uint64_t *out,
                                    uint64_t cap) {
  uint64_t total = 0;
  each_set_bit(words, 0, n, [&](uint64_t i) {
    if (total < cap) out[total] = i;
    return ++total, true;
  });
  return total;
}

}  // namespace ngpu
