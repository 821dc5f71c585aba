// dict_save_plan.hpp — the host plan of dict save (dict_save.hip,
// ngpu_dict_save / ngpu_node_dict_save): where the blob table and the chunk table
// of the RAFS v6 dict bootstrap lie, its 4096 header bytes, how the records are cut
// into windows, and every refusal that needs no device.  The file is what
// nydus_gpu.rafs.write_v6_bootstrap writes: super block magic at 1024, the
// extended super block at 1152, the blob rows at 4096, the chunk table on the next
// 4096 boundary.  Checked on the CPU by tests/cpp/dict_save_plan_test.cpp (no GPU).
// Header-only, host-only; needs <stdint.h>, <string.h> and nydus_gpu.h.
#pragma once
#include <stdint.h>
#include <string.h>

#include "nydus_gpu.h"

namespace ngpu {

constexpr uint64_t kSaveMaxEntries = 0xFFFFFFFFull;  // entries < this, as ngpu_dict_create
constexpr uint64_t kSaveMaxBlobs = 1u << 20;         // as ngpu_dict_create
constexpr uint64_t kSaveHeaderBytes = 4096;          // the blob table's offset
constexpr uint64_t kSaveRecordBytes = 80, kSaveBlobBytes = 256;
// What a window costs per record in a staging slot: the 80-B record and the 16-B
// placement row that goes up for it.
constexpr uint64_t kSaveWindowRowBytes = 96;

// The layout of a file of k records and b blob rows; windows is left 0.  false:
// k or b past ngpu_dict_create's limits (256 x b would not fit the header's
// 32-bit blob_table_size much later, 80 x k fits 64 bits for every k allowed).
inline bool dict_save_layout(uint64_t k, uint64_t b, ngpu_dict_save_info *out) {
  memset(out, 0, sizeof *out);
  if (k >= kSaveMaxEntries || b > kSaveMaxBlobs) return false;
  out->entries = k;
  out->blobs = b;
  out->blob_table_offset = b ? kSaveHeaderBytes : 0;
  out->blob_table_size = kSaveBlobBytes * b;
  out->chunk_table_offset = kSaveHeaderBytes + (out->blob_table_size + 4095) / 4096 * 4096;
  out->chunk_table_size = kSaveRecordBytes * k;
  out->bytes = out->chunk_table_offset + out->chunk_table_size;
  return true;
}

// Zero bytes between the end of the blob rows and the chunk table.
inline uint64_t dict_save_blob_pad(const ngpu_dict_save_info &l) {
  return l.chunk_table_offset - kSaveHeaderBytes - l.blob_table_size;
}

// The first 4096 bytes.  super_flags: 0x4 blake3, 0x8 sha256.
inline void dict_save_header(const ngpu_dict_save_info &l, uint64_t super_flags, uint32_t chunk_size,
                             uint8_t out[kSaveHeaderBytes]) {
  memset(out, 0, kSaveHeaderBytes);
  const uint32_t magic = 0xE0F5E1E2u, bts = (uint32_t)l.blob_table_size, zero32 = 0;
  const uint64_t zero64 = 0;
  memcpy(out + 1024, &magic, 4);
  uint8_t *x = out + 1152;
  memcpy(x, &super_flags, 8);
  memcpy(x + 8, &l.blob_table_offset, 8);
  memcpy(x + 16, &bts, 4);
  memcpy(x + 20, &chunk_size, 4);
  memcpy(x + 24, &l.chunk_table_offset, 8);
  memcpy(x + 32, &l.chunk_table_size, 8);
  memcpy(x + 40, &zero64, 8);  // prefetch table offset
  memcpy(x + 48, &zero32, 4);  // prefetch table size
}

// Records per window: the caller's, else the library's default, at least 1 and no
// more than the k records there are (k == 0: 1).
inline uint64_t dict_save_window_records(uint64_t requested, uint64_t dflt, uint64_t k) {
  uint64_t w = requested ? requested : dflt;
  if (w < 1) w = 1;
  if (k && w > k) w = k;
  if (!k) w = 1;
  return w;
}
inline uint64_t dict_save_windows(uint64_t k, uint64_t window_records) {
  return k / window_records + (k % window_records ? 1 : 0);
}
// Window w of entries [first, m) holds [cut(w), cut(w + 1)).
inline uint64_t dict_save_cut(uint64_t first, uint64_t m, uint64_t window_records, uint64_t w) {
  const uint64_t k = m - first;
  if (w >= dict_save_windows(k, window_records)) return m;
  return first + w * window_records;
}

// The refusals of the options against a handle of `entries` records and `blobs`
// blobs (has_table: it holds 256-B blob rows).  0: none; else why (dict_save_refusal).
enum DictSaveRefusal {
  kSaveOk = 0,
  kSaveBadFlags,       // a flag bit this build does not know
  kSaveBadReserved,    // a reserved word is not 0
  kSaveBadFirstEntry,  // first_entry > entries
  kSaveBadFirstBlob,   // first_blob > blobs
  kSaveNoBlobTable,    // records, a blob count, no blob table, no NGPU_DICT_SAVE_NO_BLOB_TABLE
  kSaveTooLarge,       // past the layout's limits
};
inline DictSaveRefusal dict_save_check(const ngpu_dict_save_options &o, uint64_t entries,
                                       uint64_t blobs, bool has_table) {
  if (o.flags & ~(uint32_t)NGPU_DICT_SAVE_NO_BLOB_TABLE) return kSaveBadFlags;
  if (o.reserved[0] || o.reserved[1]) return kSaveBadReserved;
  if (o.first_entry > entries) return kSaveBadFirstEntry;
  if (o.first_blob > blobs) return kSaveBadFirstBlob;
  if (entries >= kSaveMaxEntries || blobs > kSaveMaxBlobs) return kSaveTooLarge;
  const bool no_table = (o.flags & NGPU_DICT_SAVE_NO_BLOB_TABLE) != 0;
  if (!no_table && !has_table && blobs && entries) return kSaveNoBlobTable;
  return kSaveOk;
}
inline const char *dict_save_refusal(DictSaveRefusal r) {
  switch (r) {
    case kSaveOk: return "";
    case kSaveBadFlags: return "unknown flags";
    case kSaveBadReserved: return "a reserved word is not 0";
    case kSaveBadFirstEntry: return "first_entry is past the dict's entries";
    case kSaveBadFirstBlob: return "first_blob is past the dict's blobs";
    case kSaveNoBlobTable:
      return "the dict holds records and a blob count but no blob table "
             "(NGPU_DICT_SAVE_NO_BLOB_TABLE writes the file without one)";
    case kSaveTooLarge: return "more entries or blobs than a dict may hold";
  }
  return "";
}
// Blob rows the file carries: the handle's rows [first_blob, blobs), none when it
// holds no table or the flag says so.
inline uint64_t dict_save_blob_rows(const ngpu_dict_save_options &o, uint64_t blobs, bool has_table) {
  if (!has_table || (o.flags & NGPU_DICT_SAVE_NO_BLOB_TABLE)) return 0;
  return blobs - o.first_blob;
}

}  // namespace ngpu
