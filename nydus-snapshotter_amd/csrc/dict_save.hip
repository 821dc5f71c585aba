// dict_save.hip — dict save (ngpu_dict_save, ngpu_node_dict_save): a dict handle
// written out as the chunk-table-only RAFS v6 bootstrap that ngpu_dict_open reads,
// which is ngpu_dict_open's pipeline (dict_load.hip) run backwards.  The host plan
// -- layout, header, window cuts, refusals -- is dict_save_plan.hpp; here are the
// kernels and the windowed pipeline (window_bufs.hpp, as Check and Verity):
//
//   per window [a, a + c) of the handle's rows, on a private stream, in one of two
//   staging slots of the engine's pool:
//     1. its placement rows (16 B each, the handle's host rows) are copied into the
//        slot's pinned half and go H2D (a dict that keeps none: nothing);
//     2. dict_to_records writes the 80-B records into the slot's HBM half;
//     3. one D2H brings 80 x c bytes into the pinned half; an event follows.
//   The host waits for the event of window i after it has enqueued window i + 1 and
//   hands the pinned bytes to the writer as they are: no host work per row.
//
// A partitioned node dict: every part holds its rows in ascending global id order,
// so the rows of [a, b) are one slice per part (node_save_bounds: one launch per
// part finds all cuts).  The slices are DMA-copied to a scratch on the saving
// engine's device and dict_to_records_scatter puts row g at slot g - a, marking a
// bit per slot; a row outside the window or a slot marked twice bumps a counter
// that comes back with the window.
//
// NGPU_DICT_TRACE=1: one stderr line per call with the kernel and D2H times of its
// windows between HIP events (tools/dict_save_bench.py reads it).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "blob.hpp"
#include "dict_save_plan.hpp"
#include "engine_internal.hpp"
#include "window_bufs.hpp"

using namespace ngpu;

static_assert(sizeof(ngpu_dict_save_options) == 40, "ngpu_dict_save_options is 40 bytes");
static_assert(sizeof(ngpu_dict_save_info) == 64, "ngpu_dict_save_info is 64 bytes");
static_assert(sizeof(DictPlace) == 16 && sizeof(RafsV6ChunkInfo) == 80, "row sizes");

namespace ngpu {
namespace {

// 16-byte piece `part` (0..4) of the 80-B RAFS v6 chunk-info record of one dict row:
//   0, 1  block_id
//   2     blob_index, flags, compressed_size, uncompressed_size
//   3     compressed_offset, uncompressed_offset
//   4     file_offset (0), index, reserved (0)
// row: the 16-B placement {compressed_offset, compressed_size, flags}; null: stored
// uncompressed at offset 0 (csize = usize, flags 0), as dict_export_row.  Each lane
// loads one 16-B piece of the 64-B DictRec and at most one placement row.
__device__ __forceinline__ uint4 record_piece(const DictRec *r, const DictPlace *row, uint32_t part,
                                              uint32_t first_blob) {
  const uint4 *r4 = reinterpret_cast<const uint4 *>(r);
  const uint4 x = r4[part < 2 ? part : (part == 3 ? 3 : 2)];  // 2: usize, blob, index, gid; 3: uoff
  if (part < 2) return x;
  if (part == 4) return make_uint4(0, 0, x.z, 0);
  uint4 p = make_uint4(0, 0, 0, 0);
  if (row) p = *reinterpret_cast<const uint4 *>(row);  // coff lo, coff hi, csize, flags
  if (part == 3) return make_uint4(p.x, p.y, x.x, x.y);
  return make_uint4(x.y - first_blob, p.w, row ? p.z : x.x, x.x);
}

// rec[0, c) (+ place[0, c), may be null) -> out[0, 5 c).  One lane per 16-B piece:
// piece q is part q % 5 of record q / 5, so consecutive lanes store consecutive
// 16-B pieces and a wave's store covers 1 KiB of the window in one run (a lane per
// record would store at an 80-B stride).
__global__ void __launch_bounds__(256) dict_to_records(const DictRec *__restrict__ rec,
                                                       const DictPlace *__restrict__ place, uint64_t c,
                                                       uint32_t first_blob, uint4 *__restrict__ out) {
  const uint64_t q = blockIdx.x * 256ull + threadIdx.x;
  if (q >= 5 * c) return;
  const uint64_t i = q / 5;
  const uint32_t part = (uint32_t)(q - 5 * i);
  out[q] = record_piece(rec + i, place ? place + i : nullptr, part, first_blob);
}

// The scatter form: rows[0, n) are the parts' slices of the window of ids [a, a + c),
// row j goes to slot rows[j].gid - a (placement row: place[slot]).  The lane of
// piece 0 sets bit slot of bitmap (zeroed by the caller); a row outside the window
// or a bit already set adds one to *err.  Within a slice the ids ascend, so the
// stores are runs with gaps where other parts' rows go.
__global__ void __launch_bounds__(256) dict_to_records_scatter(
    const DictRec *__restrict__ rows, uint64_t n, const DictPlace *__restrict__ place, uint64_t a,
    uint64_t c, uint32_t first_blob, uint4 *__restrict__ out, uint32_t *__restrict__ bitmap,
    unsigned long long *__restrict__ err) {
  const uint64_t q = blockIdx.x * 256ull + threadIdx.x;
  if (q >= 5 * n) return;
  const uint64_t j = q / 5;
  const uint32_t part = (uint32_t)(q - 5 * j);
  const uint64_t g = rows[j].gid;
  if (g < a || g - a >= c) {
    if (part == 0) atomicAdd(err, 1ull);
    return;
  }
  const uint64_t slot = g - a;
  if (part == 0) {
    const uint32_t bit = 1u << (slot & 31);
    if (atomicOr(bitmap + (slot >> 5), bit) & bit) atomicAdd(err, 1ull);
  }
  out[5 * slot + part] = record_piece(rows + j, place ? place + slot : nullptr, part, first_blob);
}

// One thread per window cut t in [0, nw]: off[t] = the first row of rec[0, m_o)
// whose global id is >= the cut (first + t x window_records; the last cut is m).
__global__ void node_save_bounds(const DictRec *__restrict__ rec, uint64_t m_o, uint64_t first,
                                 uint64_t m, uint64_t window_records, uint64_t nw,
                                 uint64_t *__restrict__ off) {
  const uint64_t t = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (t > nw) return;
  const uint64_t cut = t >= nw ? m : first + t * window_records;
  uint64_t lo = 0, hi = m_o;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (rec[mid].gid < cut) lo = mid + 1;
    else hi = mid;
  }
  off[t] = lo;
}

// The range pre-pass: the smallest entry id >= first_entry among rec[lo, hi) whose
// blob index is below first_blob into *bad (set to ~0 by the caller).  by_gid: the
// entry id is the row's global id (a part of a node dict), else its position.
__global__ void dict_save_tail_check(const DictRec *__restrict__ rec, uint64_t lo, uint64_t hi,
                                     uint64_t first_entry, uint64_t m, int by_gid, uint32_t first_blob,
                                     unsigned long long *__restrict__ bad) {
  const uint64_t i = lo + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= hi) return;
  const uint64_t id = by_gid ? rec[i].gid : i;
  if (id >= first_entry && id < m && rec[i].blob < first_blob) atomicMin(bad, (unsigned long long)id);
}

unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

// *bad = the first entry of `rec[lo, hi)` on `device` that fails the tail check, ~0: none.
int tail_check(ngpu_engine *e, int device, const DictRec *rec, uint64_t lo, uint64_t hi,
               uint64_t first_entry, uint64_t m, bool by_gid, uint32_t first_blob, uint64_t *bad) {
  *bad = ~0ull;
  if (lo >= hi) return 0;
  DeviceGuard dg(device);
  BuildStream bs(device);
  if (!bs.s) return fail(e, NGPU_EHIP, "dict save: no stream");
  unsigned long long *d_bad = nullptr, *h_bad = nullptr;
  int rc = 0;
  if (hipMalloc((void **)&d_bad, 8) != hipSuccess ||
      hipHostMalloc((void **)&h_bad, 8, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    rc = fail(e, NGPU_ENOMEM, "dict save: the range check's counter");
  } else {
    bool ok = hipMemsetAsync(d_bad, 0xFF, 8, bs.s) == hipSuccess;
    if (ok) {
      hipLaunchKernelGGL(dict_save_tail_check, dim3(blocks_of(hi - lo)), dim3(256), 0, bs.s, rec, lo, hi,
                         first_entry, m, by_gid ? 1 : 0, first_blob, d_bad);
      ok = hipGetLastError() == hipSuccess &&
           hipMemcpyAsync(h_bad, d_bad, 8, hipMemcpyDeviceToHost, bs.s) == hipSuccess;
    }
    if (hipStreamSynchronize(bs.s) != hipSuccess || !ok)
      rc = fail(e, NGPU_EHIP, "dict save: the range check failed");
    else
      *bad = *h_bad;
  }
  if (d_bad) (void)hipFree(d_bad);
  if (h_bad) (void)hipHostFree(h_bad);
  return rc;
}

// off[0, nw] of one part (node_save_bounds), on the part's device.
int part_bounds(ngpu_engine *e, const ngpu_dict *p, uint64_t first, uint64_t m, uint64_t wr, uint64_t nw,
                std::vector<uint64_t> *off) {
  off->assign(nw + 1, 0);
  const uint64_t m_o = p->dev.m;
  if (!m_o || !p->st) return 0;
  DeviceGuard dg(p->device);
  BuildStream bs(p->device);
  if (!bs.s) return fail(e, NGPU_EHIP, "dict save: no stream");
  uint64_t *d_off = nullptr;
  if (hipMalloc((void **)&d_off, 8 * (nw + 1)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(e, NGPU_ENOMEM, "dict save: %llu window cuts", (unsigned long long)(nw + 1));
  }
  launch_node_save_bounds(p->st->rec, m_o, first, m, wr, nw, d_off, bs.s);
  // (off's pageable memory: the stream is synchronised before it goes out of scope)
  const bool ok = hipGetLastError() == hipSuccess &&
                  hipMemcpyAsync(off->data(), d_off, 8 * (nw + 1), hipMemcpyDeviceToHost, bs.s) == hipSuccess;
  const bool synced = hipStreamSynchronize(bs.s) == hipSuccess;
  (void)hipFree(d_off);
  if (!ok || !synced) return fail(e, NGPU_EHIP, "dict save: the window cuts of a part failed");
  return 0;
}

int tile_fail(ngpu_engine *e, const char *what) {
  return fail(e, NGPU_EINVAL, "dict save: the parts do not tile the dict's ids (%s)", what);
}

bool trace_on() {
  static const bool t = [] {
    const char *v = getenv("NGPU_DICT_TRACE");
    return v && v[0] == '1';
  }();
  return t;
}

}  // namespace

void launch_node_save_bounds(const DictRec *rec, uint64_t m_o, uint64_t first, uint64_t m,
                             uint64_t window_records, uint64_t nw, uint64_t *off, hipStream_t s) {
  hipLaunchKernelGGL(node_save_bounds, dim3(blocks_of(nw + 1)), dim3(256), 0, s, rec, m_o, first, m,
                     window_records, nw, off);
}

// The body of both entry points.  d: a plain dict or a node dict of e's node;
// partitioned node dicts only when node_call.
int dict_save_run(ngpu_engine *e, const ngpu_dict *d, const ngpu_dict_save_options *opt, bool node_call,
                  ngpu_write_fn w, void *ctx, ngpu_dict_save_info *info) {
  ngpu_dict_save_options o;
  memset(&o, 0, sizeof o);
  if (opt) o = *opt;
  const bool parted = !d->parts.empty() && !d->replicated;
  if (parted && !node_call)
    return fail(e, NGPU_EUNSUPP,
                "dict save: a partitioned node dict's rows lie on its parts (ngpu_node_dict_save takes it)");
  if (int rc = dict_check(e, d)) return rc;
  // the rows of a plain dict or of a replica on e's device
  const ngpu_dict *p = nullptr;
  if (d->parts.empty()) {
    if (d->device != e->device)
      return fail(e, NGPU_EINVAL, "chunk dict lives on device %d, engine on %d", d->device, e->device);
    p = d;
  } else if (d->replicated) {
    for (const ngpu_dict *x : d->parts)
      if (!p && x->device == e->device) p = x;
    if (!p) return fail(e, NGPU_EINVAL, "dict save: no replica on the engine's device %d", e->device);
  }
  const uint64_t m = d->dev.m;
  const uint32_t nb = d->dev.n_blobs;
  const bool has_table = !d->blob_table.empty();
  if (const DictSaveRefusal r = dict_save_check(o, m, nb, has_table))
    return fail(e, NGPU_EINVAL, "dict save: %s (first_entry %llu of %llu entries, first_blob %u of %u blobs, flags 0x%x)",
                dict_save_refusal(r), (unsigned long long)o.first_entry, (unsigned long long)m, o.first_blob,
                nb, o.flags);
  if (has_table && d->blob_table.size() != kSaveBlobBytes * nb)
    return fail(e, NGPU_EINVAL, "dict save: a blob table of %llu rows, %u blobs",
                (unsigned long long)(d->blob_table.size() / kSaveBlobBytes), nb);
  if (p && p->dev.m != m)
    return fail(e, NGPU_EINVAL, "dict save: replica of %llu entries, dict of %llu",
                (unsigned long long)p->dev.m, (unsigned long long)m);
  if (parted) {
    uint64_t total = 0;
    for (const ngpu_dict *x : d->parts) total += x->dev.m;
    if (total != m) return tile_fail(e, "the parts' rows do not add up to its entries");
  }
  const uint64_t first = o.first_entry, k = m - first;
  const uint64_t brows = dict_save_blob_rows(o, nb, has_table);
  ngpu_dict_save_info lay;
  if (!dict_save_layout(k, brows, &lay)) return fail(e, NGPU_EINVAL, "dict save: %s", dict_save_refusal(kSaveTooLarge));
  const DictPlace *place = d->place();
  const uint64_t wr =
      dict_save_window_records(o.window_records, staging_slot_cap(e) / kSaveWindowRowBytes, k);
  const uint64_t nw = dict_save_windows(k, wr);
  lay.windows = nw;

  // ---- the range pre-pass ----------------------------------------------------
  if (o.first_blob && k) {
    uint64_t bad = ~0ull;
    if (p) {
      if (int rc = tail_check(e, p->device, p->st->rec, first, m, first, m, false, o.first_blob, &bad)) return rc;
    } else {
      for (const ngpu_dict *x : d->parts) {
        uint64_t b = ~0ull;
        if (!x->dev.m || !x->st) continue;
        if (int rc = tail_check(e, x->device, x->st->rec, 0, x->dev.m, first, m, true, o.first_blob, &b)) return rc;
        bad = std::min(bad, b);
      }
    }
    if (bad != ~0ull)
      return fail(e, NGPU_EINVAL,
                  "dict save: entry %llu names a blob below first_blob %u (the dict does not descend from "
                  "the saved handle by extends)",
                  (unsigned long long)bad, o.first_blob);
  }

  // ---- a partitioned dict's slices per window ----------------------------------
  const size_t W = d->parts.size();
  std::vector<std::vector<uint64_t>> off;
  if (parted && k) {
    off.resize(W);
    for (size_t q = 0; q < W; ++q)
      if (int rc = part_bounds(e, d->parts[q], first, m, wr, nw, &off[q])) return rc;
    for (uint64_t wi = 0; wi < nw; ++wi) {
      uint64_t rows = 0;
      for (size_t q = 0; q < W; ++q) {
        if (off[q][wi + 1] < off[q][wi] || off[q][wi + 1] > d->parts[q]->dev.m)
          return tile_fail(e, "a part's ids do not ascend");
        rows += off[q][wi + 1] - off[q][wi];
      }
      const uint64_t a = dict_save_cut(first, m, wr, wi), b = dict_save_cut(first, m, wr, wi + 1);
      if (rows != b - a) return tile_fail(e, "the slices of a window do not add up to its ids");
    }
  }

  // ---- the windows -------------------------------------------------------------
  DeviceGuard dg_(e->device);
  WindowBufs B(e);
  const int nbuf = (int)std::min<uint64_t>(nw, 2);
  const uint64_t wcap = k ? wr : 0;  // records a window holds
  struct {
    uint8_t *scr = nullptr;          // partitioned: the parts' slices (64 B x wcap)
    uint32_t *bitmap = nullptr;      //   a bit per slot
    unsigned long long *d_err = nullptr, *h_err = nullptr;
    hipEvent_t t[3] = {};            // trace: before the kernel, after it, after the D2H
  } X[2];
  const bool trace = trace_on();
  if (int rc = B.open(nbuf, kSaveWindowRowBytes * wcap, "dict save")) return rc;
  for (int b = 0; b < nbuf; ++b)
    if (parted && (!B.dmalloc(&X[b].scr, sizeof(DictRec) * wcap) || !B.dmalloc(&X[b].bitmap, 4 * ((wcap + 31) / 32)) ||
                   !B.dmalloc(&X[b].d_err, 8) || !B.hmalloc(&X[b].h_err, 8)))
      return B.no_windows(kSaveWindowRowBytes * wcap, "dict save");
  auto drop_trace = [&] {
    for (auto &x : X)
      for (hipEvent_t &t : x.t)
        if (t) (void)hipEventDestroy(t), t = nullptr;
  };
  for (int b = 0; b < nbuf && trace; ++b)
    for (hipEvent_t &t : X[b].t)
      if (hipEventCreate(&t) != hipSuccess) {
        t = nullptr;
        drop_trace();
        return fail(e, NGPU_EHIP, "dict save: no trace events");
      }

  // Window wi into buffer wi & 1: everything up to its event.
  auto enqueue = [&](uint64_t wi) -> int {
    const int b = (int)(wi & 1);
    const uint64_t a = dict_save_cut(first, m, wr, wi), c = dict_save_cut(first, m, wr, wi + 1) - a;
    uint8_t *h = (uint8_t *)B.win[b].h, *dv = (uint8_t *)B.win[b].d;
    const DictPlace *d_place = nullptr;
    if (place) {
      memcpy(h + kSaveRecordBytes * wcap, place + a, sizeof(DictPlace) * c);
      HIP_TRY(e, hipMemcpyAsync(dv + kSaveRecordBytes * wcap, h + kSaveRecordBytes * wcap, sizeof(DictPlace) * c,
                                hipMemcpyHostToDevice, B.s));
      d_place = reinterpret_cast<const DictPlace *>(dv + kSaveRecordBytes * wcap);
    }
    if (!parted) {
      if (trace) HIP_TRY(e, hipEventRecord(X[b].t[0], B.s));
      hipLaunchKernelGGL(dict_to_records, dim3(blocks_of(5 * c)), dim3(256), 0, B.s, p->st->rec + a, d_place, c,
                         o.first_blob, reinterpret_cast<uint4 *>(dv));
      HIP_TRY(e, hipGetLastError());
    } else {
      HIP_TRY(e, hipMemsetAsync(X[b].bitmap, 0, 4 * ((c + 31) / 32), B.s));
      HIP_TRY(e, hipMemsetAsync(X[b].d_err, 0, 8, B.s));
      uint64_t pos = 0;
      for (size_t q = 0; q < W; ++q) {
        const ngpu_dict *x = d->parts[q];
        const uint64_t lo = off[q][wi], cnt = off[q][wi + 1] - lo;
        if (!cnt) continue;
        void *to = X[b].scr + sizeof(DictRec) * pos;
        const void *from = x->st->rec + lo;
        if (x->device == e->device)
          HIP_TRY(e, hipMemcpyAsync(to, from, sizeof(DictRec) * cnt, hipMemcpyDeviceToDevice, B.s));
        else
          HIP_TRY(e, hipMemcpyPeerAsync(to, e->device, from, x->device, sizeof(DictRec) * cnt, B.s));
        pos += cnt;
      }
      if (trace) HIP_TRY(e, hipEventRecord(X[b].t[0], B.s));
      hipLaunchKernelGGL(dict_to_records_scatter, dim3(blocks_of(5 * pos)), dim3(256), 0, B.s,
                         reinterpret_cast<const DictRec *>(X[b].scr), pos, d_place, a, c, o.first_blob,
                         reinterpret_cast<uint4 *>(dv), X[b].bitmap, X[b].d_err);
      HIP_TRY(e, hipGetLastError());
    }
    HIP_TRY(e, hipEventRecord(trace ? X[b].t[1] : B.fence, B.s));
    HIP_TRY(e, hipMemcpyAsync(h, dv, kSaveRecordBytes * c, hipMemcpyDeviceToHost, B.s));
    if (parted) HIP_TRY(e, hipMemcpyAsync(X[b].h_err, X[b].d_err, 8, hipMemcpyDeviceToHost, B.s));
    if (trace) HIP_TRY(e, hipEventRecord(X[b].t[2], B.s));
    HIP_TRY(e, hipEventRecord(B.done[b], B.s));
    return 0;
  };

  auto run = [&]() -> int {
    // ---- header and blob rows ----
    uint64_t at = 0;
    auto put = [&](const void *buf, uint64_t len) -> int {
      if (len && w(ctx, buf, len) != 0)
        return fail(e, NGPU_EIO, "dict save: the writer failed at byte %llu of %llu", (unsigned long long)at,
                    (unsigned long long)lay.bytes);
      at += len;
      return 0;
    };
    // the first window is on its way while the header goes out
    if (nw)
      if (int rc = enqueue(0)) return rc;
    {
      std::vector<uint8_t> head(kSaveHeaderBytes);
      dict_save_header(lay, d->digester == NGPU_DIGEST_SHA256 ? 0x8 : 0x4, d->chunk_size, head.data());
      if (int rc = put(head.data(), head.size())) return rc;
      if (brows)
        if (int rc = put(d->blob_table.data() + kSaveBlobBytes * o.first_blob, kSaveBlobBytes * brows)) return rc;
      const std::vector<uint8_t> zeros(dict_save_blob_pad(lay), 0);
      if (int rc = put(zeros.data(), zeros.size())) return rc;
    }
    float k_us = 0, c_us = 0, k_max = 0, c_max = 0;
    for (uint64_t wi = 0; wi < nw; ++wi) {
      const int b = (int)(wi & 1);
      if (wi + 1 < nw)
        if (int rc = enqueue(wi + 1)) return rc;
      HIP_TRY(e, hipEventSynchronize(B.done[b]));
      if (parted && *X[b].h_err) return tile_fail(e, "a row outside its window or an id held twice");
      if (trace) {
        float t01 = 0, t12 = 0;
        (void)hipEventElapsedTime(&t01, X[b].t[0], X[b].t[1]);
        (void)hipEventElapsedTime(&t12, X[b].t[1], X[b].t[2]);
        k_us += 1e3f * t01, c_us += 1e3f * t12;
        k_max = std::max(k_max, 1e3f * t01), c_max = std::max(c_max, 1e3f * t12);
      }
      const uint64_t c = dict_save_cut(first, m, wr, wi + 1) - dict_save_cut(first, m, wr, wi);
      if (int rc = put(B.win[b].h, kSaveRecordBytes * c)) return rc;
    }
    if (trace)
      fprintf(stderr,
              "ngpu dict_save k=%llu parts=%zu place=%d windows=%llu window_records=%llu kernel_us=%.1f "
              "d2h_us=%.1f kernel_us_max=%.1f d2h_us_max=%.1f\n",
              (unsigned long long)k, parted ? W : (size_t)0, place ? 1 : 0, (unsigned long long)nw,
              (unsigned long long)wr, k_us, c_us, k_max, c_max);
    return 0;
  };
  const int rc = run();
  if (B.s) (void)hipStreamSynchronize(B.s);  // drained before the trace events go
  drop_trace();
  if (rc) return rc;
  if (info) *info = lay;
  return 0;
}

}  // namespace ngpu

extern "C" {

int ngpu_dict_save_layout(uint64_t entries, uint32_t blobs, ngpu_dict_save_info *out) {
  if (!out) return NGPU_EINVAL;
  if (!dict_save_layout(entries, blobs, out))
    return host_fail(NGPU_EINVAL, "dict save layout: %s", dict_save_refusal(kSaveTooLarge));
  return 0;
}

int ngpu_dict_save(ngpu_engine *e, const ngpu_dict *d, const ngpu_dict_save_options *opt, ngpu_write_fn w,
                   void *ctx, ngpu_dict_save_info *info) {
  if (info) memset(info, 0, sizeof *info);
  if (!e || !d || !w) return NGPU_EINVAL;
  return guarded_entry(e, "dict save", [&] { return dict_save_run(e, d, opt, false, w, ctx, info); });
}

}  // extern "C"
